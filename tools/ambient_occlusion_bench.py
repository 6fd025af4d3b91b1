"""Time oxc_generate_ambient_occlusion (tools/, not bench.py) on the frame of tools/contact_shadows_bench.py: the configs[2] scene drawn by
oxc_draw_visbuffer at 3840 x 2160, normals from synth.normals_from_depth, then the call at the engine's four presets (1 x 2, 2 x 2, 3 x 3,
9 x 3 slices x samples per side) with GPU::VBGTAOSettings' defaults.  Prints one JSON line: per preset, ms per call (HIP events around the
three launches, median and minimum of --steps after --warmup), and from one extra call with the counting instantiation of the main kernel
(never the timed one) the fifteen counters of oxc_debug_ambient_occlusion_stats.  Also the streaming floors from --hbm-tbs: prefilter 4 B
read + 5.33 B written, main 4 + 8 + 4 + 2 B, denoise 2 + 4 + 2 B per pixel (the vector-issue floors follow from the counts and the ISA:
DESIGN.md section 14).  Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (k_ao_prefilter, k_ao_main,
k_ao_denoise)."""
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
    ap.add_argument("--effect-radius", type=float, default=0.5)
    ap.add_argument("--presets", default="low,medium,high,ultra")
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the per-kernel streaming floors (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import AmbientOcclusionContext, CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance
    from oxylus_amd.synth import SceneSpec, hilbert_noise_lut, make_scene, normals_from_depth

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    K = bench.K_MESHLETS_PER_MESH
    M = max(1, args.meshlets // K)
    scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    r.reserve(M, M * K)
    r.prepared_frame = PreparedFrame.create(scene, with_triangles=True)
    cam = scene.cull_camera()
    pv = [cam.projection_view[i] for i in range(16)]  # the scene's camera: view = identity, so projection_view is the projection
    inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    view = np.eye(4, dtype=np.float32).reshape(-1)
    W, H = (int(v) for v in args.size.split("x"))
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=cam)
    r.seed_meshlet_instances(ctx, M * K)
    r.cull_geometry(ctx)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
    depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=dev))
    r.draw_visbuffer(ctx, pv, W, H, visdepth, clear=True, depth=depth)
    torch.cuda.synchronize()
    del visdepth
    normal = normals_from_depth(depth.data.view(H, W), inv, (0.0, 0.0, 0.0))
    hilbert = hilbert_noise_lut().to(dev)
    far = float(np.float64(pv[14]) / np.float64(pv[10]))  # the far plane of the scene's reversed-Z projection
    presets = {"low": (1, 2), "medium": (2, 2), "high": (3, 3), "ultra": (9, 3)}
    bytes_pp = {"prefilter": 4 + 16 / 3, "main": 4 + 8 + 4 + 2, "denoise": 2 + 4 + 2}
    out = {"workload": "ambient_occlusion", "size": args.size, "scene_meshlets": M * K, "pixels": W * H, "effect_radius": args.effect_radius, "configs": {}}
    if args.hbm_tbs > 0:
        out["streaming_floor_ms"] = {k: v * W * H / (args.hbm_tbs * 1e12) * 1e3 for k, v in bytes_pp.items()}
    for kind in args.presets.split(","):
        slices, samples = presets[kind]
        c = AmbientOcclusionContext.create(depth, normal, hilbert, view, pv, far, slice_count=slices, samples_per_slice_side=samples,
                                           effect_radius=args.effect_radius)
        times = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.generate_ambient_occlusion(c)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        r.debug_set_tuning(L.TUNE_AMBIENT_OCCLUSION_STATS, 1)
        r.generate_ambient_occlusion(c)
        st = r.debug_ambient_occlusion_stats()
        r.debug_set_tuning(L.TUNE_AMBIENT_OCCLUSION_STATS, 0)
        ao = c.ambient_occlusion_attachment.view(torch.float16)
        out["configs"][kind] = {"slice_count": slices, "samples_per_slice_side": samples, "ms_median": float(np.median(times)), "ms_min": float(np.min(times)),
                                **st, "mean_ao": float(ao.float().mean())}
        print(kind, out["configs"][kind], flush=True)
    r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
