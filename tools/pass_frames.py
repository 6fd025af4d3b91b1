"""What the per-pass timing tools (tools/<pass>_bench.py) share: their common arguments, the frames they time their call on -- each built in
one place, so two tools that name the same frame run on the same bytes -- the HIP-event loop, the counting call, the streaming floor and
the --out writer.  The frames are stages of one chain over the configs[2] scene of bench.py: main_scene -> draw_main -> decoded_frame ->
shading_terms / light_records / pbr_context (lit_frame: the whole chain under 8 lights), and draw_main -> shadow_frame -> shadow_cull /
draw_shadow_frame.  Two seeded generators run through the chain, s.g (torch: the normals, then the ambient occlusion, resolved and contact
terms) and s.rng (numpy: the materials, then every light record in the order asked for); no stage seeds them again."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from oxylus_amd import lib as L  # noqa: E402
from oxylus_amd.renderer import (CullGeometryContext, ImageAttachment, PBRContext, PreparedFrame, RendererInstance, VirtualShadowmapContext,  # noqa: E402
                                 VisbufferDecodeContext, VsmDrawContext)
from oxylus_amd.synth import SceneSpec, make_scene, pack_clipmaps, pack_lights, pack_materials, virtual_shadow_matrices  # noqa: E402

VSM_SHAPE = {"page_size": 128, "page_table_size": 64, "physical_page_table_size": 8192, "clipmaps": 10}  # the reference shape shadow_frame builds
MAX_SHADOW_DISTANCE = 500.0


def common_arguments(sizes=None):
    """The parser with --size (or, given `sizes`, --sizes with that default), --steps, --warmup and --meshlets; the tool adds its own options."""
    ap = argparse.ArgumentParser()
    if sizes:
        ap.add_argument("--sizes", default=sizes)
    else:
        ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--meshlets", type=int, default=10_000_000)
    return ap


def parse(ap, argv, hbm_help=None):
    """Adds --hbm-tbs (with that help text, for the tools that report a streaming floor) and --out, and parses."""
    if hbm_help:
        ap.add_argument("--hbm-tbs", type=float, default=0.0, help=hbm_help)
    ap.add_argument("--out", default="")
    return ap.parse_args(argv)


def extent(size):
    """(W, H) of "WxH"."""
    W, H = (int(v) for v in size.split("x"))
    return W, H


def renderer():
    return RendererInstance(0), torch.device("cuda:0")


def main_scene(r, meshlets, dev, materials=0):
    """The configs[2] scene of `meshlets` meshlets as r's prepared frame: scene, M, K, the cull camera cam, its projection_view pv (the
    scene's view is the identity, so pv is the projection), inv (pv's inverse, column-major float32) and inv_rows (row-major float64).
    With `materials`: random 10:10:10 vertex normals and that many random materials, which starts the two generators g and rng."""
    K = bench.K_MESHLETS_PER_MESH
    M = max(1, meshlets // K)
    s = SimpleNamespace(M=M, K=K, dev=dev)
    s.scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    if materials:
        s.g = torch.Generator(device=dev)
        s.g.manual_seed(15)
        s.scene.normals = torch.randint(0, 1 << 30, (s.scene.positions.shape[0],), generator=s.g, device=dev, dtype=torch.int32)
        s.rng = rng = np.random.default_rng(15)
        s.scene.materials = pack_materials(rng.random((materials, 4)), rng.random((materials, 3)) * 4.0, rng.random(materials), rng.random(materials)).to(dev)
        s.scene.mesh_instances[:, 2] = (torch.arange(M, device=dev) % materials).to(torch.int32)
        s.scene.bind()
    r.reserve(M, M * K)
    r.prepared_frame = PreparedFrame.create(s.scene, with_triangles=True)
    s.cam = s.scene.cull_camera()
    s.pv = [s.cam.projection_view[i] for i in range(16)]
    s.inv_rows = np.linalg.inv(np.asarray(s.pv, np.float64).reshape(4, 4).T)
    s.inv = s.inv_rows.T.reshape(-1).astype(np.float32)
    return s


def draw_main(r, s, W, H, visbuffer=False):
    """Culls the scene (every test, one pass) and draws it with oxc_draw_visbuffer into a fresh W x H depth image: s.ctx, s.depth and, where
    asked, the visbuffer s.vis."""
    s.W, s.H = W, H
    s.ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=s.cam)
    r.seed_meshlet_instances(s.ctx, s.M * s.K)
    r.cull_geometry(s.ctx)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=s.dev)
    s.depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=s.dev))
    s.vis = torch.zeros((H, W), dtype=torch.int32, device=s.dev) if visbuffer else None
    r.draw_visbuffer(s.ctx, s.pv, W, H, visdepth, clear=True, depth=s.depth, visbuffer=s.vis)
    torch.cuda.synchronize()


def decode_context(s):
    """The oxc_decode_visbuffer context over a frame drawn with its visbuffer."""
    return VisbufferDecodeContext.create(s.vis, s.depth, s.pv, s.M * s.K, s.scene.materials)


def decoded_frame(r, s):
    """The G-buffer of the drawn frame: s.decoded, the decode context after its call."""
    s.decoded = decode_context(s)
    r.decode_visbuffer(s.decoded)
    torch.cuda.synchronize()


def shading_terms(s):
    """Random images in [0, 1] for the ambient occlusion (f16) and the resolved and contact shadow terms, drawn from s.g in that order."""
    unit = lambda: torch.rand((s.H, s.W), generator=s.g, device=s.dev, dtype=torch.float32)  # noqa: E731
    s.ao = unit().to(torch.float16).view(torch.int16)
    s.resolved, s.contact = unit(), unit()
    s.depth_host = s.depth.data.view(s.H, s.W).cpu().numpy()
    s.covered = np.nonzero(s.depth_host != 0)


def light_records(s, count):
    """`count` lights from the running s.rng: each half a unit above the world position behind a random covered pixel, alternately a point
    light with a cutoff, a point light without one and a spot light."""
    W, H, dz, (ys, xs) = s.W, s.H, s.depth_host, s.covered
    lights = []
    for i in range(count):
        k = int(s.rng.integers(0, len(ys))) if len(ys) else 0
        ndc = np.array([(xs[k] + 0.5) / W * 2 - 1, (ys[k] + 0.5) / H * 2 - 1, dz[ys[k], xs[k]], 1.0]) if len(ys) else np.array([0.0, 0.0, 0.5, 1.0])
        h = s.inv_rows @ ndc
        lights.append(dict(kind=(1, 1, 2)[i % 3], position=tuple(h[:3] / h[3] + np.array([0.0, 0.5, 0.0])), range=(4.0, 0.0, 0.0)[i % 3],
                           color=tuple(s.rng.uniform(0.2, 1.0, 3)), intensity=float(s.rng.uniform(1.0, 10.0)), direction=(0.0, -1.0, 0.0), inner_cone_angle=0.3,
                           outer_cone_angle=0.8))
    return lights


def pbr_context(s, lights, transparent):
    """The oxc_apply_pbr context over the decoded frame, the shading terms and `lights`, writing B10G11R11 or, `transparent`, R16G16B16A16."""
    d = s.decoded
    flags = L.SCENE_HAS_DIRECTIONAL_LIGHT | L.SCENE_HAS_CONTACT_SHADOWS | L.SCENE_HAS_SKY | (L.SCENE_TRANSPARENT_BACKGROUND if transparent else 0)
    return PBRContext.create(s.depth, d.albedo_attachment, d.normal_attachment, d.emissive_attachment, d.metallic_roughness_occlusion_attachment, s.ao, s.resolved,
                             s.contact, flags, s.inv_rows.T.reshape(-1), (0.0, 0.0, 0.0), (0.3, 0.8, 0.5), 3.0, lights=pack_lights(lights).to(s.dev) if lights else None,
                             sky_solid_color=(0.25, 0.5, 1.0, 1.0), sky_ambient_color=(0.1, 0.15, 0.2))


def lit_frame(r, W, H, meshlets, transparent, dev):
    """The lit image under 8 lights, 16 materials: the scene drawn, decoded and lit by oxc_apply_pbr, one final attachment per entry of
    `transparent` (the output format)."""
    s = main_scene(r, meshlets, dev, materials=16)
    draw_main(r, s, W, H, visbuffer=True)
    decoded_frame(r, s)
    shading_terms(s)
    lights = light_records(s, 8)
    out = []
    for flag in transparent:
        c = pbr_context(s, lights, flag)
        r.apply_pbr(c)
        torch.cuda.synchronize()
        out.append(c.final_attachment)
    return out


def shadow_light():
    """The direction the sun shines in."""
    light = np.array([0.3, -1.0, 0.2])
    return light / np.linalg.norm(light)


def virtual_shadowmap(s):
    """The reference VSM shape (VSM_SHAPE) over the drawn frame's depth, its table zeroed: (context, clipmap matrices, near plane)."""
    mats, offs, zn = virtual_shadow_matrices(list(s.scene.camera["position"]), shadow_light(), MAX_SHADOW_DISTANCE, 10.0, 10)
    v = VirtualShadowmapContext.create(s.depth.data.view(s.H, s.W), s.inv, (s.W, s.H), pack_clipmaps(mats, offs, zn), with_physical=True)
    return v, mats, zn


def shadow_frame(s):
    """The shadow side of the drawn frame: the virtual shadowmap v, the last clipmap's camera scam and the unexpanded shadow PreparedFrame."""
    v, mats, zn = virtual_shadowmap(s)
    light = shadow_light()
    scam = s.scene.cull_camera()
    for i in range(16):
        scam.projection_view[i] = float(mats[9][i])
    for i in range(3):
        scam.position[i] = float(-light[i])
    scam.near_clip = zn
    return SimpleNamespace(v=v, scam=scam, sframe=PreparedFrame.create(s.scene, expand=False), light=light)


def shadow_cull(r, sh):
    """One frame's page update (with whatever v.dirty_mesh_instance_indices holds, cleared afterwards) and use_hpb shadow cull; the cull context."""
    v = sh.v
    r.update_virtual_shadowmap(v)
    v.dirty_mesh_instance_indices = None
    r.prepared_frame = sh.sframe
    sctx = CullGeometryContext(use_hpb=True, init_cull_meshes=True, cull_flags=L.CULL_TEST_FRUSTUM, cull_camera=sh.scam, hpb_attachment=v.hpb_attachment,
                               vsm_clipmaps_buffer=v.vsm_clipmaps_buffer, vsm_clipmap_dirty_flags_buffer=v.vsm_clipmap_dirty_flags_buffer, vsm_clipmap_count=10)
    r.cull_geometry(sctx)
    return sctx


def draw_shadow_frame(r, sh):
    """One frame of the shadow chain: update -> shadow cull -> oxc_draw_physical_pages."""
    r.draw_physical_pages(VsmDrawContext.create(sh.v, shadow_cull(r, sh)))


def time_call(fn, steps, warmup, before=None):
    """(median, min) ms of fn() over `steps` calls after `warmup`: a new HIP event pair around each call, a synchronise after each.  `before`
    runs ahead of each pair, outside the timed span."""
    times = []
    for i in range(warmup + steps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def counted_call(r, knob, fn, stats):
    """stats() of one fn() with the counting instantiation of its kernel (debug tuning `knob`): one extra call, never a timed one."""
    r.debug_set_tuning(knob, 1)
    fn()
    st = stats()
    r.debug_set_tuning(knob, 0)
    return st


def streaming_floor(row, nbytes, hbm_tbs):
    """row["streaming_floor_ms"]: the time `nbytes` (or each entry of a dict of them) take at `hbm_tbs` TB/s; nothing without a rate."""
    if hbm_tbs > 0:
        ms = lambda n: n / (hbm_tbs * 1e12) * 1e3  # noqa: E731
        row["streaming_floor_ms"] = {k: ms(n) for k, n in nbytes.items()} if isinstance(nbytes, dict) else ms(nbytes)


def report(lines, row):
    """Prints a row as one JSON line and keeps it for write_out."""
    lines.append(json.dumps(row))
    print(lines[-1])


def write_out(path, lines):
    """The JSON lines into --out, where given; returns them (what main returns)."""
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return lines
