"""Time oxc_contact_shadows (tools/, not bench.py) on pass_frames.draw_main: the configs[2] scene drawn by oxc_draw_visbuffer
at 3840 x 2160, then the call -- (a) with the engine's defaults (steps 8, thickness 0.1, shadow_length 0.01: rays under two pixels, n == 2)
and (b) with --long-length, a shadow_length that makes most rays reach n == steps = 8.  Prints one JSON line: per configuration, ms per call
(HIP events around the call, median and minimum of --steps after --warmup), pixels, and from one extra call with the counting instantiation
of the kernel (never the timed one): non-sky pixels, depth taps, pixels per outcome and per step-count class.  Also the streaming floor: 8
bytes per pixel over the rate given with --hbm-tbs (the vector-issue floor follows from these counts and the ISA: DESIGN.md section 13).
Per-kernel time comes from a rocprofv3 --kernel-trace --stats run of this script (k_contact_shadows)."""
import numpy as np

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import ContactShadowsContext


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--long-length", type=float, default=2.0, help="shadow_length of configuration (b)")
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the 8 B/pixel floor (0: not reported)")

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H)
    view = np.eye(4, dtype=np.float32).reshape(-1)
    sun = np.array([-0.3, 1.0, -0.2])  # towards the light of pass_frames.shadow_light
    out = {"workload": "contact_shadows", "size": args.size, "scene_meshlets": s.M * s.K, "pixels": W * H, "compulsory_bytes": 8 * W * H, "configs": {}}
    pf.streaming_floor(out, 8 * W * H, args.hbm_tbs)
    for kind, kw in (("engine_defaults", dict(steps=8, thickness=0.1, shadow_length=0.01)), ("long_rays", dict(steps=8, thickness=0.1, shadow_length=args.long_length))):
        c = ContactShadowsContext.create(s.depth, s.inv, view, s.pv, float(s.cam.near_clip), sun, **kw)
        med, mn = pf.time_call(lambda: r.contact_shadows(c), args.steps, args.warmup)
        st = pf.counted_call(r, L.TUNE_CONTACT_SHADOWS_STATS, lambda: r.contact_shadows(c), r.debug_contact_shadows_stats)
        shadow = c.contact_shadows_attachment.data
        out["configs"][kind] = {**kw, "ms_median": med, "ms_min": mn, **st,
                                "pixels_fully_lit": int((shadow == 1.0).sum()), "pixels_fully_shadowed": int((shadow == 0.0).sum())}
        print(kind, out["configs"][kind], flush=True)
    r.close()
    lines = []
    pf.report(lines, out)
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
