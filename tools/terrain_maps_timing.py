"""Time oxc_generate_terrain_maps (tools/, not bench.py) at the engine's Terrain defaults: a 2048 x 2048 map with 64 x 64 patches, 3 noise
octaves and 5 erosion octaves on a 1024 x 1024 world 400 units high, zeroed edit images.  Rows: the full bake, each stage alone on the baked
maps, a regional call at the brush's default footprint (radius_world 32 on 0.5-unit texels: 64 texels, so 2 * ceil(64 + 1) + 1 = 131 texels
and ceil(131 / 32) + 1 = 6 patches, as Passes/Terrain.cpp:147-156 forms them) with the region in device memory, and the whole call on a
2 x 2 map -- what three launches cost without the texels.  Prints one JSON line per row: ms per call (HIP events around the call, median and
minimum of --steps after --warmup) and the texels and patches it writes."""
import dataclasses

import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import TerrainMapsContext


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv)

    r, dev = pf.renderer()
    lines = []
    bake = TerrainMapsContext.create(device=dev)
    region = torch.tensor([900, 1100, 28, 34], dtype=torch.int32, device=dev)
    brush = dataclasses.replace(bake, region=region, dispatch_texels=(131, 131), dispatch_patches=(6, 6))
    tiny = TerrainMapsContext.create((2, 2), (1, 1), device=dev)
    rows = [("bake", bake, 2048 * 2048, 64 * 64),
            ("generate", dataclasses.replace(bake, stages=L.TERRAIN_GENERATE), 2048 * 2048, 0),
            ("derive", dataclasses.replace(bake, stages=L.TERRAIN_DERIVE), 2048 * 2048, 0),
            ("minmax", dataclasses.replace(bake, stages=L.TERRAIN_MINMAX), 0, 64 * 64),
            ("brush region", brush, 144 * 144, 8 * 8),
            ("2 x 2", tiny, 4, 1)]
    for name, context, texels, patches in rows:
        med, mn = pf.time_call(lambda: r.generate_terrain_maps(context), args.steps, args.warmup)
        pf.report(lines, {"workload": "terrain_maps", "call": "generate_terrain_maps", "row": name, "stages": int(context.stages), "ms_median": med, "ms_min": mn,
                          "texels": texels, "patches": patches})
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
