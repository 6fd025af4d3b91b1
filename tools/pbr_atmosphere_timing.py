"""Time oxc_apply_pbr_atmosphere (tools/, not bench.py) on the frame and extent of tools/pbr_apply_bench.py -- the configs[2] scene drawn,
decoded and lit under 8 lights -- with the engine's LUT extents (256 x 64, 312 x 192, 32 x 32 x 32) and cube 32, filled by one
generate_sky_luts, one draw_atmosphere and two generate_sky_ibl before the timed calls.  Then oxc_apply_pbr on the same G-buffer and lights,
the point of comparison: the difference is the cost of the branch.  Prints one JSON line per call: ms per call (HIP events around the call,
median and minimum of --steps after --warmup), the pixels and the share of them that are sky."""
import dataclasses

import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import Atmosphere, AtmosphereContext, PBRAtmosphereContext, SkyIblContext
from sky_ibl_timing import hemisphere


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--materials", type=int, default=16)
    ap.add_argument("--lights", type=int, default=8)
    args = pf.parse(ap, argv)

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev, materials=args.materials)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H, visbuffer=True)
    pf.decoded_frame(r, s)
    pf.shading_terms(s)
    plain = pf.pbr_context(s, pf.light_records(s, args.lights), False)
    sky = AtmosphereContext.create(Atmosphere.engine(), dev, sun_dir=plain.sun_dir, sun_intensity=plain.sun_intensity, camera_position=plain.camera_position,
                                   camera_inv_projection_view=tuple(plain.inv_projection_view))
    r.generate_sky_luts(sky.sky_luts(hemisphere(dev)))
    r.draw_atmosphere(sky)
    ibl = SkyIblContext.create(sky, 32)
    for frame_index in (0, 1):
        r.generate_sky_ibl(dataclasses.replace(ibl, frame_index=frame_index))
    branch = PBRAtmosphereContext.create(plain, sky, ibl, scene_flags=plain.scene_flags | L.SCENE_HAS_ATMOSPHERE)
    torch.cuda.synchronize()
    pixels = W * H
    sky_share = 1.0 - len(s.covered[0]) / pixels
    lines = []
    for name, call in (("apply_pbr_atmosphere", lambda: r.apply_pbr_atmosphere(branch)), ("apply_pbr", lambda: r.apply_pbr(plain))):
        med, mn = pf.time_call(call, args.steps, args.warmup)
        pf.report(lines, {"workload": "pbr_atmosphere", "call": name, "size": args.size, "lights": args.lights, "ms_median": med, "ms_min": mn, "pixels": pixels,
                          "sky_share": round(sky_share, 4)})
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
