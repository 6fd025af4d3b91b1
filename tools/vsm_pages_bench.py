"""Time oxc_update_virtual_shadowmap (tools/, not bench.py): the reference shape (page 128, table 64, physical 8192, 10 clipmaps) on a
real raster depth of the configs[2] scene (the bench's 10 M-meshlet scene drawn by oxc_draw_visbuffer) at 3840 x 2160 and 4096^2, first
frame (zeroed table: every visible page allocated, dirty and cleared in the physical image) and steady frame (the same depth again).
Prints one JSON line: per size and frame kind, ms per call (HIP events around the whole call, median of --steps) and the call's pages.
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (k_vsm_*)."""
import pass_frames as pf


def main(argv=None):
    args = pf.parse(pf.common_arguments(sizes="3840x2160,4096x4096"), argv)

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev)
    out = {"workload": "vsm_page_update", "shape": pf.VSM_SHAPE, "scene_meshlets": s.M * s.K, "sizes": {}}
    for size in args.sizes.split(","):
        W, H = pf.extent(size)
        pf.draw_main(r, s, W, H)
        covered = int((s.depth.data != 0).sum())
        v = pf.virtual_shadowmap(s)[0]
        rec = {"pixels": W * H, "covered_pixels": covered, "depth_bytes": W * H * 4}
        for kind in ("first", "steady"):
            med, mn = pf.time_call(lambda: r.update_virtual_shadowmap(v), args.steps, args.warmup, before=v.virtual_page_table.zero_ if kind == "first" else None)
            c = v.counters_buffer.cpu().tolist()
            rec[kind] = {"ms_median": med, "ms_min": mn, "requests": c[0], "dirty_pages": c[1], "free_pages": c[2], "failed": c[4]}
        out["sizes"][size] = rec
    r.close()
    lines = []
    pf.report(lines, out)
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
