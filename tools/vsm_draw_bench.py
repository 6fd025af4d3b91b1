"""Time oxc_draw_physical_pages (tools/, not bench.py) on pass_frames.shadow_frame -- the configs[2] scene drawn by oxc_draw_visbuffer at
3840 x 2160, the reference VSM shape (page 128, table 64, physical 8192, 10 clipmaps), the use_hpb shadow cull with the last clipmap's
camera -- over three frames: the first (zeroed table: every requested page dirty), a steady one (same depth: nothing
dirty) and one with a few invalidated mesh instances.  Prints one JSON line: per frame, ms per draw call (HIP events around the call, median
of --steps), the triangles in the shadow list, the (triangle, clipmap) pairs that survive the page bitmap, the fragments written, and the
big pairs, tiles and clipped pairs with how many of each went past their queue (from one extra call with the counting kernels).
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (k_vsm_draw_*)."""
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import VsmDrawContext


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--invalidated", type=int, default=8, help="mesh instances invalidated in the third frame")
    args = pf.parse(ap, argv)

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev)
    pf.draw_main(r, s, *pf.extent(args.size))
    sh = pf.shadow_frame(s)
    v, scene = sh.v, s.scene
    out = {"workload": "vsm_draw_physical_pages", "size": args.size, "shape": pf.VSM_SHAPE, "scene_meshlets": s.M * s.K, "frames": {}}
    g = torch.Generator().manual_seed(5)
    for kind in ("first", "steady", "invalidated"):
        if kind == "invalidated":
            v.dirty_mesh_instance_indices = torch.randperm(s.M, generator=g)[: args.invalidated].to(torch.int32).to(dev)
            v.mesh_instances_buffer, v.meshes_buffer = scene.mesh_instances, scene.meshes
            v.transforms_world_buffer = v.transforms_previous_buffer = scene.transforms
        sctx = pf.shadow_cull(r, sh)
        c = r.read_counters(sctx)
        d = VsmDrawContext.create(v, sctx, with_commands=True)
        med, mn = pf.time_call(lambda: r.draw_physical_pages(d), args.steps, args.warmup)
        st = pf.counted_call(r, L.TUNE_VSM_DRAW_STATS, lambda: r.draw_physical_pages(d), r.debug_vsm_draw_stats)
        counters = v.counters_buffer.cpu().tolist()
        out["frames"][kind] = {"ms_median": med, "ms_min": mn, "triangles": c.draw_index_count // 3,
                               "active_clipmaps": int(d.draw_count_buffer.cpu()[0]), "dirty_pages": counters[1], "pairs_kept": st["pairs"],
                               "fragments": st["fragments"], "big_pairs": st["big_pairs"], "big_pairs_overflowed": st["big_pairs_overflowed"],
                               "tiles": st["tiles"], "tiles_overflowed": st["tiles_overflowed"], "clipped_pairs": st["clipped_pairs"],
                               "clipped_pairs_overflowed": st["clipped_pairs_overflowed"]}
        print(kind, out["frames"][kind], flush=True)
    r.close()
    lines = []
    pf.report(lines, out)
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
