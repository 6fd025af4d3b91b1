"""Time oxc_resolve_shadowmap (tools/, not bench.py) on pass_frames.draw_shadow_frame: the configs[2] scene drawn by oxc_draw_visbuffer
at 3840 x 2160, the reference VSM shape (page 128, table 64, physical 8192, 10 clipmaps), page update -> use_hpb shadow cull -> shadow draw,
then the resolve -- on the first frame (zeroed table: every requested page drawn this frame) and on a steady one (same depth: nothing
dirty, the pages of the first frame are read again).  The normal image is synthesised from the depth image (synth.normals_from_depth).
Prints one JSON line: per frame, ms per resolve call (HIP events around the call, median and minimum of --steps after --warmup), pixels,
and from one extra call with the counting instantiation of the kernel (never the timed one): non-sky pixels, taps taken, taps no clipmap
served, taps served by each fallback clipmap, and the pixels per early return.  Also the streaming floor: 16 bytes per pixel over the
rate given with --hbm-tbs (the vector-issue floor follows from these counts and the ISA: DESIGN.md section 12).  Per-kernel time comes
from a rocprofv3 --kernel-trace --stats run of this script (k_vsm_resolve_shadow)."""
import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import ShadowResolveContext
from oxylus_amd.synth import normals_from_depth


def main(argv=None):
    args = pf.parse(pf.common_arguments(), argv, hbm_help="measured streaming rate in TB/s for the 16 B/pixel floor (0: not reported)")

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H)
    sh = pf.shadow_frame(s)
    normal = normals_from_depth(s.depth.data.view(H, W), s.inv, s.scene.camera["position"])
    res = ShadowResolveContext.create(sh.v, normal, sh.light, pf.MAX_SHADOW_DISTANCE * 2.0)
    out = {"workload": "vsm_resolve_shadowmap", "size": args.size, "shape": pf.VSM_SHAPE, "scene_meshlets": s.M * s.K, "pixels": W * H,
           "compulsory_bytes": 16 * W * H, "frames": {}}
    pf.streaming_floor(out, 16 * W * H, args.hbm_tbs)
    for kind in ("first", "steady"):
        pf.draw_shadow_frame(r, sh)
        med, mn = pf.time_call(lambda: r.resolve_shadowmap(res), args.steps, args.warmup)
        st = pf.counted_call(r, L.TUNE_VSM_RESOLVE_STATS, lambda: r.resolve_shadowmap(res), r.debug_vsm_resolve_stats)
        shadow = res.resolved_shadows_attachment.data
        out["frames"][kind] = {"ms_median": med, "ms_min": mn, "backed_pages": int(((sh.v.virtual_page_table & 4) != 0).sum()),
                               **st, "pixels_fully_lit": int((shadow == 1.0).sum()), "pixels_fully_shadowed": int((shadow == 0.0).sum())}
        print(kind, out["frames"][kind], flush=True)
    r.close()
    lines = []
    pf.report(lines, out)
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
