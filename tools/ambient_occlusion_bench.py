"""Time oxc_generate_ambient_occlusion (tools/, not bench.py) on pass_frames.draw_main: the configs[2] scene drawn by
oxc_draw_visbuffer at 3840 x 2160, normals from synth.normals_from_depth, then the call at the engine's four presets (1 x 2, 2 x 2, 3 x 3,
9 x 3 slices x samples per side) with GPU::VBGTAOSettings' defaults.  Prints one JSON line: per preset, ms per call (HIP events around the
three launches, median and minimum of --steps after --warmup), and from one extra call with the counting instantiation of the main kernel
(never the timed one) the fifteen counters of oxc_debug_ambient_occlusion_stats.  Also the streaming floors from --hbm-tbs: prefilter 4 B
read + 5.33 B written, main 4 + 8 + 4 + 2 B, denoise 2 + 4 + 2 B per pixel (the vector-issue floors follow from the counts and the ISA:
DESIGN.md section 14).  Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (k_ao_prefilter, k_ao_main,
k_ao_denoise)."""
import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import AmbientOcclusionContext
from oxylus_amd.synth import hilbert_noise_lut, normals_from_depth


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--effect-radius", type=float, default=0.5)
    ap.add_argument("--presets", default="low,medium,high,ultra")
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the per-kernel streaming floors (0: not reported)")

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H)
    view = np.eye(4, dtype=np.float32).reshape(-1)
    normal = normals_from_depth(s.depth.data.view(H, W), s.inv, (0.0, 0.0, 0.0))
    hilbert = hilbert_noise_lut().to(dev)
    far = float(np.float64(s.pv[14]) / np.float64(s.pv[10]))  # the far plane of the scene's reversed-Z projection
    presets = {"low": (1, 2), "medium": (2, 2), "high": (3, 3), "ultra": (9, 3)}
    bytes_pp = {"prefilter": 4 + 16 / 3, "main": 4 + 8 + 4 + 2, "denoise": 2 + 4 + 2}
    out = {"workload": "ambient_occlusion", "size": args.size, "scene_meshlets": s.M * s.K, "pixels": W * H, "effect_radius": args.effect_radius, "configs": {}}
    pf.streaming_floor(out, {k: v * W * H for k, v in bytes_pp.items()}, args.hbm_tbs)
    for kind in args.presets.split(","):
        slices, samples = presets[kind]
        c = AmbientOcclusionContext.create(s.depth, normal, hilbert, view, s.pv, far, slice_count=slices, samples_per_slice_side=samples,
                                           effect_radius=args.effect_radius)
        med, mn = pf.time_call(lambda: r.generate_ambient_occlusion(c), args.steps, args.warmup)
        st = pf.counted_call(r, L.TUNE_AMBIENT_OCCLUSION_STATS, lambda: r.generate_ambient_occlusion(c), r.debug_ambient_occlusion_stats)
        ao = c.ambient_occlusion_attachment.view(torch.float16)
        out["configs"][kind] = {"slice_count": slices, "samples_per_slice_side": samples, "ms_median": med, "ms_min": mn, **st, "mean_ao": float(ao.float().mean())}
        print(kind, out["configs"][kind], flush=True)
    r.close()
    lines = []
    pf.report(lines, out)
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
