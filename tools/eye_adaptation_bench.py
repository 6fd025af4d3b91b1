"""Time oxc_apply_eye_adaptation (tools/, not bench.py) on pass_frames.lit_frame: the configs[2] scene drawn, decoded and
lit under 8 lights at 3840 x 2160 (random ambient occlusion and shadow terms), in both formats oxc_apply_pbr writes, and on a constant image
of each format -- every pixel in one bin, the worst case of the counting.  One more row is the same call on a 1 x 1 image: the in-stream
three launches with nothing to do, the cost of an empty call of this shape on the same box.  Prints one JSON line per row: ms
per call (HIP events around the call, median and minimum of --steps after --warmup), pixels, the number of non-empty bins, the fullest bin's
share, and the streaming floor at the rate given with --hbm-tbs: 4 or 8 bytes read per pixel.  --grid caps the histogram kernel's grid
(OXC_TUNE_EYE_ADAPTATION_GRID)."""
import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import EyeAdaptationContext, exposure_buffer


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--grid", type=int, default=0, help="cap of the histogram kernel's grid in blocks (0: uncapped)")
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the floor (0: not reported)")

    r, dev = pf.renderer()
    W, H = pf.extent(args.size)
    lit = pf.lit_frame(r, W, H, args.meshlets, (False, True), dev)
    grey16 = int(np.float16(0.18).view(np.int16))
    grey = 0x31C | (0x31C << 11) | (0x18E << 22)  # UF11 / UF11 / UF10 of 0.1796875
    rows = [("lit frame", lit[0]), ("lit frame", lit[1]),
            ("constant", torch.full((H, W), grey, dtype=torch.int32, device=dev)),
            ("constant", torch.tensor([grey16, grey16, grey16, 0x3C00], dtype=torch.int16, device=dev).repeat(H, W, 1)),
            ("empty call", torch.full((1, 1), grey, dtype=torch.int32, device=dev))]
    r.debug_set_tuning(L.TUNE_EYE_ADAPTATION_GRID, args.grid)
    lines = []
    for image_name, image in rows:
        c = EyeAdaptationContext.create(image, exposure_buffer(dev), min_exposure=-11.5, max_exposure=18.0)
        med, mn = pf.time_call(lambda: r.apply_eye_adaptation(c, delta_time=1.0 / 60.0), args.steps, args.warmup)
        hist = c.histogram_buffer.cpu().numpy().view(np.uint32)
        adapted, exposure = (float(v) for v in c.exposure_buffer.cpu().numpy())
        texel = 8 if c.source_format else 4
        out = {"workload": "eye_adaptation", "image": image_name, "size": f"{c.width}x{c.height}", "format": "rgba16f" if c.source_format else "b10g11r11",
               "grid_cap": args.grid, "pixels": c.width * c.height, "ms_median": med, "ms_min": mn,
               "bins_hit": int((hist > 0).sum()), "fullest_bin_share": float(hist.max()) / float(c.width * c.height), "dark_pixels": int(hist[0]),
               "adapted_luminance": adapted, "exposure": exposure, "image_bytes": texel * c.width * c.height}
        assert int(hist.sum()) == c.width * c.height
        pf.streaming_floor(out, out["image_bytes"], args.hbm_tbs)
        pf.report(lines, out)
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
