"""Time oxc_apply_eye_adaptation (tools/, not bench.py) on the lit frame of tools/pbr_apply_bench.py: the configs[2] scene drawn, decoded and
lit under 8 lights at 3840 x 2160 (random ambient occlusion and shadow terms), in both formats oxc_apply_pbr writes, and on a constant image
of each format -- every pixel in one bin, the worst case of the counting.  One more row is the same call on a 1 x 1 image: the in-stream
three launches with nothing to do, the cost of an empty call of this shape on the same box.  Prints one JSON line per row: ms
per call (HIP events around the call, median and minimum of --steps after --warmup), pixels, the number of non-empty bins, the fullest bin's
share, and the streaming floor at the rate given with --hbm-tbs: 4 or 8 bytes read per pixel.  --grid caps the histogram kernel's grid
(OXC_TUNE_EYE_ADAPTATION_GRID)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def lit_frame(r, W, H, meshlets, transparent, dev):
    """The lit image of tools/pbr_apply_bench.py under 8 lights."""
    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PBRContext, PreparedFrame, VisbufferDecodeContext
    from oxylus_amd.synth import SceneSpec, make_scene, pack_lights, pack_materials

    K = bench.K_MESHLETS_PER_MESH
    M = max(1, meshlets // K)
    scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    g = torch.Generator(device=dev)
    g.manual_seed(15)
    scene.normals = torch.randint(0, 1 << 30, (scene.positions.shape[0],), generator=g, device=dev, dtype=torch.int32)
    rng = np.random.default_rng(15)
    n_mat = 16
    scene.materials = pack_materials(rng.random((n_mat, 4)), rng.random((n_mat, 3)) * 4.0, rng.random(n_mat), rng.random(n_mat)).to(dev)
    scene.mesh_instances[:, 2] = (torch.arange(M, device=dev) % n_mat).to(torch.int32)
    scene.bind()
    r.reserve(M, M * K)
    r.prepared_frame = PreparedFrame.create(scene, with_triangles=True)
    cam = scene.cull_camera()
    pv = [cam.projection_view[i] for i in range(16)]
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
    unit = lambda: torch.rand((H, W), generator=g, device=dev, dtype=torch.float32)  # noqa: E731
    ao = unit().to(torch.float16).view(torch.int16)
    resolved, contact = unit(), unit()
    inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T)
    dz = depth.data.view(H, W).cpu().numpy()
    ys, xs = np.nonzero(dz != 0)
    lights = []
    for i in range(8):
        k = int(rng.integers(0, len(ys))) if len(ys) else 0
        ndc = np.array([(xs[k] + 0.5) / W * 2 - 1, (ys[k] + 0.5) / H * 2 - 1, dz[ys[k], xs[k]], 1.0]) if len(ys) else np.array([0.0, 0.0, 0.5, 1.0])
        h = inv @ ndc
        lights.append(dict(kind=(1, 1, 2)[i % 3], position=tuple(h[:3] / h[3] + np.array([0.0, 0.5, 0.0])), range=(4.0, 0.0, 0.0)[i % 3],
                           color=tuple(rng.uniform(0.2, 1.0, 3)), intensity=float(rng.uniform(1.0, 10.0)), direction=(0.0, -1.0, 0.0), inner_cone_angle=0.3,
                           outer_cone_angle=0.8))
    base = L.SCENE_HAS_DIRECTIONAL_LIGHT | L.SCENE_HAS_CONTACT_SHADOWS | L.SCENE_HAS_SKY
    out = []
    for flag in transparent:
        c = PBRContext.create(depth, d.albedo_attachment, d.normal_attachment, d.emissive_attachment, d.metallic_roughness_occlusion_attachment, ao, resolved,
                              contact, base | (L.SCENE_TRANSPARENT_BACKGROUND if flag else 0), inv.T.reshape(-1), (0.0, 0.0, 0.0), (0.3, 0.8, 0.5), 3.0,
                              lights=pack_lights(lights).to(dev), sky_solid_color=(0.25, 0.5, 1.0, 1.0), sky_ambient_color=(0.1, 0.15, 0.2))
        r.apply_pbr(c)
        torch.cuda.synchronize()
        out.append(c.final_attachment)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--meshlets", type=int, default=10_000_000)
    ap.add_argument("--grid", type=int, default=0, help="cap of the histogram kernel's grid in blocks (0: uncapped)")
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the floor (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from oxylus_amd import lib as L
    from oxylus_amd.renderer import EyeAdaptationContext, RendererInstance, exposure_buffer

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    W, H = (int(v) for v in args.size.split("x"))
    lit = lit_frame(r, W, H, args.meshlets, (False, True), dev)
    grey16 = int(np.float16(0.18).view(np.int16))
    grey = 0x31C | (0x31C << 11) | (0x18E << 22)  # UF11 / UF11 / UF10 of 0.1796875
    rows = [("lit frame", lit[0]), ("lit frame", lit[1]),
            ("constant", torch.full((H, W), grey, dtype=torch.int32, device=dev)),
            ("constant", torch.tensor([grey16, grey16, grey16, 0x3C00], dtype=torch.int16, device=dev).repeat(H, W, 1)),
            ("empty call", torch.full((1, 1), grey, dtype=torch.int32, device=dev))]
    r.debug_set_tuning(L.TUNE_EYE_ADAPTATION_GRID, args.grid)
    lines = []
    for image_name, image in rows:
        c = EyeAdaptationContext.create(image, exposure_buffer(dev), min_exposure=-11.5, max_exposure=18.0)
        times = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.apply_eye_adaptation(c, delta_time=1.0 / 60.0)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        hist = c.histogram_buffer.cpu().numpy().view(np.uint32)
        adapted, exposure = (float(v) for v in c.exposure_buffer.cpu().numpy())
        texel = 8 if c.source_format else 4
        out = {"workload": "eye_adaptation", "image": image_name, "size": f"{c.width}x{c.height}", "format": "rgba16f" if c.source_format else "b10g11r11",
               "grid_cap": args.grid, "pixels": c.width * c.height, "ms_median": float(np.median(times)), "ms_min": float(np.min(times)),
               "bins_hit": int((hist > 0).sum()), "fullest_bin_share": float(hist.max()) / float(c.width * c.height), "dark_pixels": int(hist[0]),
               "adapted_luminance": adapted, "exposure": exposure, "image_bytes": texel * c.width * c.height}
        assert int(hist.sum()) == c.width * c.height
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
