"""Time oxc_apply_fxaa (tools/, not bench.py) on pass_frames.lit_frame: the configs[2] scene drawn, decoded and lit under 8 lights at
3840 x 2160 (random ambient occlusion and shadow terms), in B10G11R11 or, with --transparent, RGBA16F.  Two more rows: the same call on a
2 x 2 image, the launch floor, and on a full-frame checkerboard of two plateaus, the worst case, where every pixel searches.  Prints one
JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after --warmup), the four counters of
oxc_debug_fxaa_stats, the bytes the rule reads and writes at least once and, with --hbm-tbs, the streaming floor of those bytes."""
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import FxaaContext


def checkerboard(W, H, transparent, dev):
    """Two plateaus, (1.0, 0.75, 0.5) and (0.125, 0.25, 0.0625), alternating texel by texel."""
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    bright = ((xs + ys) % 2 == 1)
    if transparent:
        halves = torch.tensor([[0x3000, 0x3400, 0x2C00, 0x3400], [0x3C00, 0x3A00, 0x3800, 0x3A00]], dtype=torch.int16, device=dev)
        return halves[bright.long()].contiguous()
    uf = lambda v, mbits: int(v.hex().split("p")[1]) + 15 << mbits | int((float.fromhex(v.hex().split("p")[0] + "p0") - 1.0) * (1 << mbits))  # noqa: E731  (a normal, exact value)
    word = lambda r, g, b: uf(r, 6) | uf(g, 6) << 11 | uf(b, 5) << 22  # noqa: E731
    words = torch.tensor([word(0.125, 0.25, 0.0625), word(1.0, 0.75, 0.5)], dtype=torch.int64, device=dev)
    return words[bright.long()].to(torch.int32).contiguous()


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--transparent", action="store_true", help="the RGBA16F image of a transparent background instead of B10G11R11")
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the floor (0: not reported)")

    r, dev = pf.renderer()
    W, H = pf.extent(args.size)
    lit = pf.lit_frame(r, W, H, args.meshlets, (args.transparent,), dev)[0]
    small = torch.zeros((2, 2, 4), dtype=torch.int16, device=dev) if args.transparent else torch.zeros((2, 2), dtype=torch.int32, device=dev)
    lines = []
    for image_name, image in (("lit frame", lit), ("launch floor", small), ("checkerboard", checkerboard(W, H, args.transparent, dev))):
        c = FxaaContext.create(image)
        c.fxaa_attachment.fill_(-9)
        med, mn = pf.time_call(lambda: r.apply_fxaa(c), args.steps, args.warmup)
        st = pf.counted_call(r, L.TUNE_FXAA_STATS, lambda: r.apply_fxaa(c), r.debug_fxaa_stats)
        texel = 8 if c.source_format else 4
        rule_bytes = c.width * c.height * texel * 2  # the source once, the destination once (a search's taps land on texels the pass reads anyway)
        out = {"workload": "fxaa", "image": image_name, "size": f"{c.width}x{c.height}", "format": "rgba16f" if c.source_format else "b10g11r11",
               "ms_median": med, "ms_min": mn, **st, "rule_bytes": rule_bytes}
        pf.streaming_floor(out, rule_bytes, args.hbm_tbs)
        pf.report(lines, out)
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
