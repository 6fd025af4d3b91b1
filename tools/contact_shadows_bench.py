"""Time oxc_contact_shadows (tools/, not bench.py) on the frame of tools/vsm_resolve_bench.py: the configs[2] scene drawn by oxc_draw_visbuffer
at 3840 x 2160, then the call -- (a) with the engine's defaults (steps 8, thickness 0.1, shadow_length 0.01: rays under two pixels, n == 2)
and (b) with --long-length, a shadow_length that makes most rays reach n == steps = 8.  Prints one JSON line: per configuration, ms per call
(HIP events around the call, median and minimum of --steps after --warmup), pixels, and from one extra call with the counting instantiation
of the kernel (never the timed one): non-sky pixels, depth taps, pixels per outcome and per step-count class.  Also the streaming floor: 8
bytes per pixel over the rate given with --hbm-tbs (the vector-issue floor follows from these counts and the ISA: DESIGN.md section 13).
Per-kernel time comes from a rocprofv3 --kernel-trace --stats run of this script (k_contact_shadows)."""
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
    ap.add_argument("--long-length", type=float, default=2.0, help="shadow_length of configuration (b)")
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the 8 B/pixel floor (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ContactShadowsContext, CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance
    from oxylus_amd.synth import SceneSpec, make_scene

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
    sun = np.array([-0.3, 1.0, -0.2])  # towards the light of tools/vsm_resolve_bench.py
    W, H = (int(v) for v in args.size.split("x"))
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=cam)
    r.seed_meshlet_instances(ctx, M * K)
    r.cull_geometry(ctx)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
    depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=dev))
    r.draw_visbuffer(ctx, pv, W, H, visdepth, clear=True, depth=depth)
    torch.cuda.synchronize()
    del visdepth
    out = {"workload": "contact_shadows", "size": args.size, "scene_meshlets": M * K, "pixels": W * H, "compulsory_bytes": 8 * W * H, "configs": {}}
    if args.hbm_tbs > 0:
        out["streaming_floor_ms"] = 8 * W * H / (args.hbm_tbs * 1e12) * 1e3
    for kind, kw in (("engine_defaults", dict(steps=8, thickness=0.1, shadow_length=0.01)), ("long_rays", dict(steps=8, thickness=0.1, shadow_length=args.long_length))):
        c = ContactShadowsContext.create(depth, inv, view, pv, float(cam.near_clip), sun, **kw)
        times = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.contact_shadows(c)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        r.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 1)
        r.contact_shadows(c)
        st = r.debug_contact_shadows_stats()
        r.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 0)
        shadow = c.contact_shadows_attachment.data
        out["configs"][kind] = {**kw, "ms_median": float(np.median(times)), "ms_min": float(np.min(times)), **st,
                                "pixels_fully_lit": int((shadow == 1.0).sum()), "pixels_fully_shadowed": int((shadow == 0.0).sum())}
        print(kind, out["configs"][kind], flush=True)
    r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
