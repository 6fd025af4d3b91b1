"""Time oxc_apply_pbr (tools/, not bench.py) on the frame of tools/visbuffer_decode_bench.py: the configs[2] scene, given random 10:10:10 vertex
normals and --materials materials, drawn by oxc_draw_visbuffer and decoded by oxc_decode_visbuffer at 3840 x 2160; the ambient occlusion and
the two shadow terms are random images in [0, 1] (their producers' cost is not this tool's subject).  One row per entry of --lights (0, 8,
64): the lights sit half a unit off surface points sampled from the frame, alternately point lights with a cutoff, point lights without one
and spot lights.  Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after --warmup),
pixels, the pixel classes and light outcomes from one extra call with the counting instantiation of the kernel (never the timed one), and
the streaming floor at the rate given with --hbm-tbs: 34 bytes read and 4 written per pixel.  The vector-issue estimate follows from the
ISA: DESIGN.md section 16."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--meshlets", type=int, default=10_000_000)
    ap.add_argument("--materials", type=int, default=16)
    ap.add_argument("--lights", default="0,8,64")
    ap.add_argument("--transparent", action="store_true", help="the R16G16B16A16 Sfloat output (TransparentBackground)")
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the floor (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PBRContext, PreparedFrame, RendererInstance, VisbufferDecodeContext
    from oxylus_amd.synth import SceneSpec, make_scene, pack_lights, pack_materials

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    K = bench.K_MESHLETS_PER_MESH
    M = max(1, args.meshlets // K)
    scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    g = torch.Generator(device=dev)
    g.manual_seed(15)
    scene.normals = torch.randint(0, 1 << 30, (scene.positions.shape[0],), generator=g, device=dev, dtype=torch.int32)
    rng = np.random.default_rng(15)
    n_mat = args.materials
    scene.materials = pack_materials(rng.random((n_mat, 4)), rng.random((n_mat, 3)) * 4.0, rng.random(n_mat), rng.random(n_mat)).to(dev)
    scene.mesh_instances[:, 2] = (torch.arange(M, device=dev) % n_mat).to(torch.int32)
    scene.bind()
    r.reserve(M, M * K)
    r.prepared_frame = PreparedFrame.create(scene, with_triangles=True)
    cam = scene.cull_camera()
    pv = [cam.projection_view[i] for i in range(16)]
    W, H = (int(v) for v in args.size.split("x"))
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=cam)
    r.seed_meshlet_instances(ctx, M * K)
    r.cull_geometry(ctx)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
    depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=dev))
    vis = torch.zeros((H, W), dtype=torch.int32, device=dev)
    r.draw_visbuffer(ctx, pv, W, H, visdepth, clear=True, depth=depth, visbuffer=vis)
    d = VisbufferDecodeContext.create(vis, depth, pv, M * K, scene.materials)
    r.decode_visbuffer(d)
    torch.cuda.synchronize()
    del visdepth

    unit = lambda: torch.rand((H, W), generator=g, device=dev, dtype=torch.float32)  # noqa: E731
    ao = unit().to(torch.float16).view(torch.int16)
    resolved, contact = unit(), unit()
    inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T)  # row-major inverse
    # surface points for the lights: the world positions behind random covered pixels
    dz = depth.data.view(H, W).cpu().numpy()
    ys, xs = np.nonzero(dz != 0)
    flags = L.SCENE_HAS_DIRECTIONAL_LIGHT | L.SCENE_HAS_CONTACT_SHADOWS | L.SCENE_HAS_SKY | (L.SCENE_TRANSPARENT_BACKGROUND if args.transparent else 0)
    lines = []
    for count in (int(v) for v in args.lights.split(",")):
        lights = []
        for i in range(count):
            k = int(rng.integers(0, len(ys))) if len(ys) else 0
            ndc = np.array([(xs[k] + 0.5) / W * 2 - 1, (ys[k] + 0.5) / H * 2 - 1, dz[ys[k], xs[k]], 1.0]) if len(ys) else np.array([0.0, 0.0, 0.5, 1.0])
            h = inv @ ndc
            p = h[:3] / h[3] + np.array([0.0, 0.5, 0.0])
            kind = (1, 1, 2)[i % 3]
            lights.append(dict(kind=kind, position=tuple(p), range=(4.0, 0.0, 0.0)[i % 3], color=tuple(rng.uniform(0.2, 1.0, 3)), intensity=float(rng.uniform(1.0, 10.0)),
                               direction=(0.0, -1.0, 0.0), inner_cone_angle=0.3, outer_cone_angle=0.8))
        c = PBRContext.create(depth, d.albedo_attachment, d.normal_attachment, d.emissive_attachment, d.metallic_roughness_occlusion_attachment, ao, resolved,
                              contact, flags, inv.T.reshape(-1), (0.0, 0.0, 0.0), (0.3, 0.8, 0.5), 3.0, lights=pack_lights(lights).to(dev) if lights else None,
                              sky_solid_color=(0.25, 0.5, 1.0, 1.0), sky_ambient_color=(0.1, 0.15, 0.2))
        times = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.apply_pbr(c)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        r.debug_set_tuning(L.TUNE_PBR_APPLY_STATS, 1)
        r.apply_pbr(c)
        st = r.debug_pbr_apply_stats()
        r.debug_set_tuning(L.TUNE_PBR_APPLY_STATS, 0)
        out = {"workload": "pbr_apply", "size": args.size, "scene_meshlets": M * K, "lights": count, "format": "rgba16f" if args.transparent else "b10g11r11",
               "pixels": W * H, "ms_median": float(np.median(times)), "ms_min": float(np.min(times)), **st, "image_bytes": (34 + (8 if args.transparent else 4)) * W * H}
        if args.hbm_tbs > 0:
            out["streaming_floor_ms"] = out["image_bytes"] / (args.hbm_tbs * 1e12) * 1e3
        lines.append(json.dumps(out))
        print(lines[-1])
    r.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
