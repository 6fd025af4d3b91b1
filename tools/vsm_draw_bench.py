"""Time oxc_draw_physical_pages (tools/, not bench.py): the scene and shape of tools/vsm_pages_bench.py -- the configs[2] scene drawn by
oxc_draw_visbuffer at 3840 x 2160, the reference VSM shape (page 128, table 64, physical 8192, 10 clipmaps), the use_hpb shadow cull with
the last clipmap's camera -- over three frames: the first (zeroed table: every requested page dirty), a steady one (same depth: nothing
dirty) and one with a few invalidated mesh instances.  Prints one JSON line: per frame, ms per draw call (HIP events around the call, median
of --steps), the triangles in the shadow list, the (triangle, clipmap) pairs that survive the page bitmap, the fragments written, and the
big pairs, tiles and clipped pairs with how many of each went past their queue (from one extra call with the counting kernels).
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (k_vsm_draw_*)."""
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
    ap.add_argument("--invalidated", type=int, default=8, help="mesh instances invalidated in the third frame")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance, VirtualShadowmapContext, VsmDrawContext
    from oxylus_amd.synth import SceneSpec, make_scene, pack_clipmaps, virtual_shadow_matrices

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
    mats, offs, zn = virtual_shadow_matrices(list(scene.camera["position"]), light, 500.0, 10.0, 10)
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
    out = {"workload": "vsm_draw_physical_pages", "size": args.size, "shape": {"page_size": 128, "page_table_size": 64, "physical_page_table_size": 8192,
                                                                          "clipmaps": 10}, "scene_meshlets": M * K, "frames": {}}
    g = torch.Generator().manual_seed(5)
    for kind in ("first", "steady", "invalidated"):
        if kind == "invalidated":
            ids = torch.randperm(M, generator=g)[: args.invalidated].to(torch.int32).to(dev)
            v.dirty_mesh_instance_indices = ids
            v.mesh_instances_buffer, v.meshes_buffer = scene.mesh_instances, scene.meshes
            v.transforms_world_buffer = v.transforms_previous_buffer = scene.transforms
        r.update_virtual_shadowmap(v)
        v.dirty_mesh_instance_indices = None
        r.prepared_frame = sframe
        sctx = CullGeometryContext(use_hpb=True, init_cull_meshes=True, cull_flags=L.CULL_TEST_FRUSTUM, cull_camera=scam, hpb_attachment=v.hpb_attachment,
                                   vsm_clipmaps_buffer=v.vsm_clipmaps_buffer, vsm_clipmap_dirty_flags_buffer=v.vsm_clipmap_dirty_flags_buffer, vsm_clipmap_count=10)
        r.cull_geometry(sctx)
        c = r.read_counters(sctx)
        d = VsmDrawContext.create(v, sctx, with_commands=True)
        times = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.draw_physical_pages(d)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        r.debug_set_tuning(L.TUNE_VSM_DRAW_STATS, 1)
        r.draw_physical_pages(d)
        st = r.debug_vsm_draw_stats()
        r.debug_set_tuning(L.TUNE_VSM_DRAW_STATS, 0)
        counters = v.counters_buffer.cpu().tolist()
        out["frames"][kind] = {"ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "triangles": c.draw_index_count // 3,
                               "active_clipmaps": int(d.draw_count_buffer.cpu()[0]), "dirty_pages": counters[1], "pairs_kept": st["pairs"],
                               "fragments": st["fragments"], "big_pairs": st["big_pairs"], "big_pairs_overflowed": st["big_pairs_overflowed"],
                               "tiles": st["tiles"], "tiles_overflowed": st["tiles_overflowed"], "clipped_pairs": st["clipped_pairs"],
                               "clipped_pairs_overflowed": st["clipped_pairs_overflowed"]}
        print(kind, out["frames"][kind], flush=True)
    r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
