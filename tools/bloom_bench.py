"""Time oxc_apply_bloom (tools/, not bench.py) on the lit frame of tools/eye_adaptation_bench.py: the configs[2] scene drawn, decoded and lit
under 8 lights at 3840 x 2160 (random ambient occlusion and shadow terms), in both formats oxc_apply_pbr writes, with the exposure
oxc_apply_eye_adaptation leaves behind.  One more row is the same call on a 2 x 2 image: the prefilter launch alone (L = 1), the cost of an
empty call.  --tail sets OXC_TUNE_BLOOM_TAIL_LEVEL (0: the library's choice; 13: one launch per level), and with --compare-tail the lit rows
run a second time with one launch per level and the two results are compared byte for byte.  Prints one JSON line per row: ms per call (HIP
events around the call, median and minimum of --steps after --warmup), the level count, the launches, the bytes the rule reads and writes at
least once and, with --hbm-tbs, the streaming floor of those bytes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def time_call(r, c, steps, warmup):
    times = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r.apply_bloom(c)
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--meshlets", type=int, default=10_000_000)
    ap.add_argument("--tail", type=int, default=0, help="OXC_TUNE_BLOOM_TAIL_LEVEL (0: the library's choice; 13: one launch per level)")
    ap.add_argument("--compare-tail", action="store_true", help="time the lit rows with one launch per level too and compare the bytes")
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the floor (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from eye_adaptation_bench import lit_frame
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import BloomContext, EyeAdaptationContext, RendererInstance, exposure_buffer

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    W, H = (int(v) for v in args.size.split("x"))
    lit = lit_frame(r, W, H, args.meshlets, (False, True), dev)
    rows = [("lit frame", lit[0]), ("lit frame", lit[1]), ("empty call", torch.zeros((2, 2), dtype=torch.int32, device=dev))]
    lines = []
    for image_name, image in rows:
        exposure = exposure_buffer(dev)
        r.apply_eye_adaptation(EyeAdaptationContext.create(image, exposure, min_exposure=-11.5, max_exposure=18.0), delta_time=1.0 / 60.0)
        c = BloomContext.create(image, L.SCENE_HAS_EYE_ADAPTATION | L.SCENE_HAS_BLOOM, exposure)
        levels = c.bloom_upsampled_attachment.levels
        texel = 8 if c.source_format else 4
        pyramid_texels = sum(max(1, c.bloom_upsampled_attachment.width >> k) * max(1, c.bloom_upsampled_attachment.height >> k) for k in range(levels))
        level0 = c.bloom_upsampled_attachment.width * c.bloom_upsampled_attachment.height
        # the source once; D written once and read twice (the next downsample, the upsample) but for level 0's single read; U written once and read once
        # but for level 0, which nothing reads
        rule_bytes = texel * (c.width * c.height + 3 * pyramid_texels - level0 + 2 * pyramid_texels - level0)
        variants = [("tail", args.tail)] + ([("per-level", 13)] if args.compare_tail and image_name == "lit frame" else [])
        results = {}
        for variant, tail in variants:
            r.debug_set_tuning(L.TUNE_BLOOM_TAIL_LEVEL, tail)
            c.bloom_downsampled_attachment.data.fill_(-9)
            c.bloom_upsampled_attachment.data.fill_(-9)
            med, mn = time_call(r, c, args.steps, args.warmup)
            torch.cuda.synchronize()
            results[variant] = (c.bloom_downsampled_attachment.data.clone(), c.bloom_upsampled_attachment.data.clone())
            out = {"workload": "bloom", "image": image_name, "size": f"{c.width}x{c.height}", "format": "rgba16f" if c.source_format else "b10g11r11",
                   "variant": variant, "tail_level": tail, "levels": levels, "ms_median": med, "ms_min": mn, "exposure": float(exposure[1]), "rule_bytes": rule_bytes,
                   "bloom_nonzero_texels": int((c.bloom_upsampled_attachment.level(0).reshape(level0, -1)[:, :3 if c.source_format else 1] != 0).any(dim=1).sum())}
            if args.hbm_tbs > 0:
                out["streaming_floor_ms"] = rule_bytes / (args.hbm_tbs * 1e12) * 1e3
            lines.append(json.dumps(out))
            print(lines[-1])
        if len(results) == 2:
            same = all(torch.equal(a, b) for a, b in zip(results["tail"], results["per-level"]))
            lines.append(json.dumps({"workload": "bloom", "image": image_name, "format": "rgba16f" if c.source_format else "b10g11r11", "tail_equals_per_level": same}))
            print(lines[-1])
            assert same
    r.debug_set_tuning(L.TUNE_BLOOM_TAIL_LEVEL, 0)
    r.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
