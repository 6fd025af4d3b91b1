"""Time oxc_update_virtual_shadowmap (tools/, not bench.py): the reference shape (page 128, table 64, physical 8192, 10 clipmaps) on a
real raster depth of the configs[2] scene (the bench's 10 M-meshlet scene drawn by oxc_draw_visbuffer) at 3840 x 2160 and 4096^2, first
frame (zeroed table: every visible page allocated, dirty and cleared in the physical image) and steady frame (the same depth again).
Prints one JSON line: per size and frame kind, ms per call (HIP events around the whole call, median of --steps) and the call's pages.
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (k_vsm_*)."""
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
    ap.add_argument("--sizes", default="3840x2160,4096x4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--meshlets", type=int, default=10_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance, VirtualShadowmapContext
    from oxylus_amd.synth import SceneSpec, make_scene, pack_clipmaps, virtual_shadow_matrices

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    K = bench.K_MESHLETS_PER_MESH
    M = max(1, args.meshlets // K)
    scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    r.reserve(M, M * K)
    frame = PreparedFrame.create(scene, with_triangles=True)
    r.prepared_frame = frame
    cam = scene.cull_camera()
    pv = [cam.projection_view[i] for i in range(16)]
    inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    light = np.array([0.3, -1.0, 0.2])
    light /= np.linalg.norm(light)
    mats, offs, zn = virtual_shadow_matrices(list(scene.camera["position"]), light, 500.0, 10.0, 10)
    clip = pack_clipmaps(mats, offs, zn)
    out = {"workload": "vsm_page_update", "shape": {"page_size": 128, "page_table_size": 64, "physical_page_table_size": 8192, "clipmaps": 10},
           "scene_meshlets": M * K, "sizes": {}}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=cam)
        r.seed_meshlet_instances(ctx, M * K)
        r.cull_geometry(ctx)
        visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
        depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=dev))
        r.draw_visbuffer(ctx, pv, W, H, visdepth, clear=True, depth=depth)
        torch.cuda.synchronize()
        covered = int((depth.data != 0).sum())
        v = VirtualShadowmapContext.create(depth.data.view(H, W), inv, (W, H), clip, with_physical=True)
        rec = {"pixels": W * H, "covered_pixels": covered, "depth_bytes": W * H * 4}
        for kind in ("first", "steady"):
            times = []
            for i in range(args.warmup + args.steps):
                if kind == "first":
                    v.virtual_page_table.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                r.update_virtual_shadowmap(v)
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    times.append(a.elapsed_time(b))
            c = v.counters_buffer.cpu().tolist()
            rec[kind] = {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "requests": c[0], "dirty_pages": c[1],
                         "free_pages": c[2], "failed": c[4]}
        out["sizes"][size] = rec
    r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
