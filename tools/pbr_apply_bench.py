"""Time oxc_apply_pbr (tools/, not bench.py) on pass_frames.decoded_frame: the configs[2] scene, given random 10:10:10 vertex
normals and --materials materials, drawn by oxc_draw_visbuffer and decoded by oxc_decode_visbuffer at 3840 x 2160; the ambient occlusion and
the two shadow terms are random images in [0, 1] (their producers' cost is not this tool's subject).  One row per entry of --lights (0, 8,
64): the lights sit half a unit off surface points sampled from the frame, alternately point lights with a cutoff, point lights without one
and spot lights.  Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after --warmup),
pixels, the pixel classes and light outcomes from one extra call with the counting instantiation of the kernel (never the timed one), and
the streaming floor at the rate given with --hbm-tbs: 34 bytes read and 4 written per pixel.  The vector-issue estimate follows from the
ISA: DESIGN.md section 16."""
import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--materials", type=int, default=16)
    ap.add_argument("--lights", default="0,8,64")
    ap.add_argument("--transparent", action="store_true", help="the R16G16B16A16 Sfloat output (TransparentBackground)")
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the floor (0: not reported)")

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev, materials=args.materials)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H, visbuffer=True)
    pf.decoded_frame(r, s)
    pf.shading_terms(s)
    lines = []
    for count in (int(v) for v in args.lights.split(",")):
        c = pf.pbr_context(s, pf.light_records(s, count), args.transparent)
        med, mn = pf.time_call(lambda: r.apply_pbr(c), args.steps, args.warmup)
        st = pf.counted_call(r, L.TUNE_PBR_APPLY_STATS, lambda: r.apply_pbr(c), r.debug_pbr_apply_stats)
        out = {"workload": "pbr_apply", "size": args.size, "scene_meshlets": s.M * s.K, "lights": count, "format": "rgba16f" if args.transparent else "b10g11r11",
               "pixels": W * H, "ms_median": med, "ms_min": mn, **st, "image_bytes": (34 + (8 if args.transparent else 4)) * W * H}
        pf.streaming_floor(out, out["image_bytes"], args.hbm_tbs)
        pf.report(lines, out)
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
