"""Time oxc_generate_sky_ibl (tools/, not bench.py) at the engine's cube_size 32 and at cube_size 1 -- what the launch and the serial tail of
one texel cost without the texel count -- on the engine's LUT extents (312 x 192, 256 x 64; the AtmosphereComponent defaults scaled by 1e-3,
the camera at the ground, the sun 30 degrees up).  The two LUTs are filled by one generate_sky_luts and one draw_atmosphere before the timed
calls; the cube keeps accumulating across them, frame_index fixed, as a captured graph would replay it.  Prints one JSON line per row: ms per
call (HIP events around the call, median and minimum of --steps after --warmup), the texels written and the samples they take."""
import math

import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd.renderer import Atmosphere, AtmosphereContext, SkyIblContext


def hemisphere(dev):
    i = np.arange(64, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / 64.0
    lon = 2.0 * math.pi * i / ((1.0 + math.sqrt(5.0)) / 2.0)
    rad = np.sqrt(1.0 - z * z)
    return torch.from_numpy(np.stack([rad * np.cos(lon), z, rad * np.sin(lon)], axis=-1).astype(np.float32)).to(dev)


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv)

    r, dev = pf.renderer()
    sun = (math.cos(math.radians(30.0)), math.sin(math.radians(30.0)), 0.0)
    lines = []
    c = AtmosphereContext.create(Atmosphere.engine(), dev, sun_dir=sun, sun_intensity=10.0)
    r.generate_sky_luts(c.sky_luts(hemisphere(dev)))
    r.draw_atmosphere(c)
    for cube_size in (32, 1):
        ibl = SkyIblContext.create(c, cube_size, frame_index=1)
        med, mn = pf.time_call(lambda: r.generate_sky_ibl(ibl), args.steps, args.warmup)
        texels = 6 * cube_size * cube_size
        pf.report(lines, {"workload": "sky_ibl", "call": "generate_sky_ibl", "cube_size": cube_size, "ms_median": med, "ms_min": mn, "texels": texels, "samples": texels * 64})
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
