"""Time oxc_apply_tonemap (tools/, not bench.py) on pass_frames.lit_frame: the configs[2] scene drawn, decoded and lit
under 8 lights at 3840 x 2160 (random ambient occlusion and shadow terms), with the exposure oxc_apply_eye_adaptation leaves behind and the
pyramid oxc_apply_bloom writes, per tone curve, with the lens flags off and all on.  One more row per curve is the same call on a 2 x 2
image: the launch floor.  Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after
--warmup), the bytes the rule reads and writes at least once and, with --hbm-tbs, the streaming floor of those bytes."""
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import BloomContext, EyeAdaptationContext, TonemapContext, exposure_buffer


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--transparent", action="store_true", help="the RGBA16F source of a transparent background instead of B10G11R11")
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the floor (0: not reported)")

    r, dev = pf.renderer()
    W, H = pf.extent(args.size)
    lit = pf.lit_frame(r, W, H, args.meshlets, (args.transparent,), dev)[0]
    small = torch.zeros((2, 2, 4), dtype=torch.int16, device=dev) if args.transparent else torch.zeros((2, 2), dtype=torch.int32, device=dev)
    base = L.SCENE_HAS_EYE_ADAPTATION | L.SCENE_HAS_BLOOM | (L.SCENE_TRANSPARENT_BACKGROUND if args.transparent else 0)
    lens = L.SCENE_HAS_FILM_GRAIN | L.SCENE_HAS_CHROMATIC_ABERRATION | L.SCENE_HAS_VIGNETTE
    names = {L.TONEMAP_NONE: "none", L.TONEMAP_ACES: "aces", L.TONEMAP_AGX: "agx", L.TONEMAP_GT7: "gt7"}
    lines = []
    for image_name, image in (("lit frame", lit), ("launch floor", small)):
        exposure = exposure_buffer(dev)
        r.apply_eye_adaptation(EyeAdaptationContext.create(image, exposure, min_exposure=-11.5, max_exposure=18.0), delta_time=1.0 / 60.0)
        bloom = BloomContext.create(image, base, exposure)
        r.apply_bloom(bloom)
        for curve, curve_name in names.items():
            for lens_name, flags in (("off", base), ("on", base | lens)):
                c = TonemapContext.create(image, flags, curve, exposure, bloom)
                c.dst_attachment.fill_(-9)
                med, mn = pf.time_call(lambda: r.apply_tonemap(c), args.steps, args.warmup)
                torch.cuda.synchronize()
                texel = 8 if c.source_format else 4
                # the source once, level 0 of the bloom once, the destination once (the aberration's taps land on texels the pass reads anyway)
                rule_bytes = c.width * c.height * (texel + 4) + (c.width // 2) * (c.height // 2) * texel + 8
                out = {"workload": "tonemap", "image": image_name, "size": f"{c.width}x{c.height}", "format": "rgba16f" if c.source_format else "b10g11r11",
                       "tonemap_type": curve_name, "lens": lens_name, "ms_median": med, "ms_min": mn, "exposure": float(exposure[1]), "rule_bytes": rule_bytes,
                       "distinct_colours": int(torch.unique(c.dst_attachment & 0xFFFFFF).numel())}
                pf.streaming_floor(out, rule_bytes, args.hbm_tbs)
                pf.report(lines, out)
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
