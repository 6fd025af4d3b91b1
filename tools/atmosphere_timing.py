"""Time oxc_generate_sky_luts and oxc_draw_atmosphere (tools/, not bench.py) at the engine's extents (256 x 64, 32 x 32, 312 x 192, 32^3;
the AtmosphereComponent defaults scaled by 1e-3, the camera at the ground, the sun 30 degrees up) and at 2 x 2 (x 1) extents: what the
launches and the serial chain of one texel cost without the texel count.  The 64 hemisphere directions are a spherical Fibonacci set.
Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after --warmup), the texels written
and the integration steps they run."""
import math

import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd.renderer import Atmosphere, AtmosphereContext


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
    table = hemisphere(dev)
    sun = (math.cos(math.radians(30.0)), math.sin(math.radians(30.0)), 0.0)
    lines = []
    small = dict(transmittance_lut_size=(2, 2, 1), multiscattering_lut_size=(2, 2, 1), sky_view_lut_size=(2, 2, 1), aerial_perspective_lut_size=(2, 2, 1))
    for extents, atmosphere in (("engine", Atmosphere.engine()), ("2 x 2", Atmosphere.engine(**small))):
        c = AtmosphereContext.create(atmosphere, dev, sun_dir=sun, sun_intensity=10.0)
        luts = c.sky_luts(table)
        t, m, v, a = atmosphere.transmittance_lut_size, atmosphere.multiscattering_lut_size, atmosphere.sky_view_lut_size, atmosphere.aerial_perspective_lut_size
        for call, fn, texels, steps in (("generate_sky_luts", lambda: r.generate_sky_luts(luts), t[0] * t[1] + m[0] * m[1], t[0] * t[1] * 1000 + m[0] * m[1] * 64 * 32),
                                        ("draw_atmosphere", lambda: r.draw_atmosphere(c), v[0] * v[1] + a[0] * a[1] * a[2],
                                         v[0] * v[1] * 48 + a[0] * a[1] * sum(2 * (z + 1) for z in range(a[2])))):
            med, mn = pf.time_call(fn, args.steps, args.warmup)
            pf.report(lines, {"workload": "atmosphere", "call": call, "extents": extents, "ms_median": med, "ms_min": mn, "texels": texels, "integration_steps": steps})
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
