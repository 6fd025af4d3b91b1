"""Time oxc_resolve_shadowmap (tools/, not bench.py) on the frame of tools/vsm_draw_bench.py: the configs[2] scene drawn by oxc_draw_visbuffer
at 3840 x 2160, the reference VSM shape (page 128, table 64, physical 8192, 10 clipmaps), page update -> use_hpb shadow cull -> shadow draw,
then the resolve -- on the first frame (zeroed table: every requested page drawn this frame) and on a steady one (same depth: nothing
dirty, the pages of the first frame are read again).  The normal image is synthesised from the depth image (synth.normals_from_depth).
Prints one JSON line: per frame, ms per resolve call (HIP events around the call, median and minimum of --steps after --warmup), pixels,
and from one extra call with the counting instantiation of the kernel (never the timed one): non-sky pixels, taps taken, taps no clipmap
served, taps served by each fallback clipmap, and the pixels per early return.  Also the streaming floor: 16 bytes per pixel over the
rate given with --hbm-tbs (the vector-issue floor follows from these counts and the ISA: DESIGN.md section 12).  Per-kernel time comes
from a rocprofv3 --kernel-trace --stats run of this script (k_vsm_resolve_shadow)."""
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
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the 16 B/pixel floor (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import (CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance, ShadowResolveContext, VirtualShadowmapContext,
                                     VsmDrawContext)
    from oxylus_amd.synth import SceneSpec, make_scene, normals_from_depth, pack_clipmaps, virtual_shadow_matrices

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    K = bench.K_MESHLETS_PER_MESH
    M = max(1, args.meshlets // K)
    scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    r.reserve(M, M * K)
    main_frame = PreparedFrame.create(scene, with_triangles=True)
    r.prepared_frame = main_frame
    cam = scene.cull_camera()
    pv = [cam.projection_view[i] for i in range(16)]
    inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    light = np.array([0.3, -1.0, 0.2])
    light /= np.linalg.norm(light)
    max_shadow_dist = 500.0
    mats, offs, zn = virtual_shadow_matrices(list(scene.camera["position"]), light, max_shadow_dist, 10.0, 10)
    clip = pack_clipmaps(mats, offs, zn)
    W, H = (int(v) for v in args.size.split("x"))
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=cam)
    r.seed_meshlet_instances(ctx, M * K)
    r.cull_geometry(ctx)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
    depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=dev))
    r.draw_visbuffer(ctx, pv, W, H, visdepth, clear=True, depth=depth)
    torch.cuda.synchronize()
    del visdepth, main_frame
    v = VirtualShadowmapContext.create(depth.data.view(H, W), inv, (W, H), clip, with_physical=True)
    scam = scene.cull_camera()
    for i in range(16):
        scam.projection_view[i] = float(mats[9][i])
    for i in range(3):
        scam.position[i] = float(-light[i])
    scam.near_clip = zn
    sframe = PreparedFrame.create(scene, expand=False)
    normal = normals_from_depth(depth.data.view(H, W), inv, scene.camera["position"])
    res = ShadowResolveContext.create(v, normal, light, max_shadow_dist * 2.0)
    out = {"workload": "vsm_resolve_shadowmap", "size": args.size, "shape": {"page_size": 128, "page_table_size": 64, "physical_page_table_size": 8192,
                                                                        "clipmaps": 10}, "scene_meshlets": M * K, "pixels": W * H,
           "compulsory_bytes": 16 * W * H, "frames": {}}
    if args.hbm_tbs > 0:
        out["streaming_floor_ms"] = 16 * W * H / (args.hbm_tbs * 1e12) * 1e3
    for kind in ("first", "steady"):
        r.update_virtual_shadowmap(v)
        r.prepared_frame = sframe
        sctx = CullGeometryContext(use_hpb=True, init_cull_meshes=True, cull_flags=L.CULL_TEST_FRUSTUM, cull_camera=scam, hpb_attachment=v.hpb_attachment,
                                   vsm_clipmaps_buffer=v.vsm_clipmaps_buffer, vsm_clipmap_dirty_flags_buffer=v.vsm_clipmap_dirty_flags_buffer, vsm_clipmap_count=10)
        r.cull_geometry(sctx)
        r.draw_physical_pages(VsmDrawContext.create(v, sctx))
        times = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.resolve_shadowmap(res)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        r.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 1)
        r.resolve_shadowmap(res)
        st = r.debug_vsm_resolve_stats()
        r.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 0)
        shadow = res.resolved_shadows_attachment.data
        out["frames"][kind] = {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "backed_pages": int(((v.virtual_page_table & 4) != 0).sum()),
                               **st, "pixels_fully_lit": int((shadow == 1.0).sum()), "pixels_fully_shadowed": int((shadow == 0.0).sum())}
        print(kind, out["frames"][kind], flush=True)
    r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
