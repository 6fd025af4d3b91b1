"""Time oxc_apply_terrain_brush (tools/, not bench.py) on the 2048 x 2048 engine-default map of terrain_maps_timing.py, baked once: the trace
alone, the apply alone in each of the five modes on the hit the trace left, and both stages, at 16 and at 256 radius texels; the same call on
a 2 x 2 map -- what two launches cost without the march or the texels; and the full edit step, brush plus the regional re-bake with the
reference's dispatch sizes (Passes/Terrain.cpp:147-156), the region being the record the trace wrote.  The ray is slanted, so the march
crosses the terrain at a step of its own and not at the first.  Prints one JSON line per row: ms per call (HIP events around the call, median
and minimum of --steps after --warmup) and the threads the apply launches.  The strokes accumulate in the edit images over the timed calls;
the work per call does not depend on their contents."""
import dataclasses
import math

import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import TerrainBrushContext, TerrainBrushParams, TerrainMapsContext

MODES = ("raise", "smooth", "flatten", "noise", "paint_layer")


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv)

    r, dev = pf.renderer()
    lines = []

    def row(name, fn, radius, stages, mode, resolution):
        med, mn = pf.time_call(fn, args.steps, args.warmup)
        side = (2 * math.ceil(radius) + 1 + 15) // 16 * 16
        pf.report(lines, {"workload": "terrain_brush", "call": "apply_terrain_brush", "row": name, "stages": stages, "mode": mode, "radius_texels": radius,
                          "resolution": resolution, "apply_threads": side * side if stages & L.TERRAIN_BRUSH_APPLY else 0, "ms_median": med, "ms_min": mn})

    maps = TerrainMapsContext.create(device=dev)
    r.generate_terrain_maps(maps)
    maps = dataclasses.replace(maps, region=torch.zeros((4,), dtype=torch.int32, device=dev))
    for radius in (16.0, 256.0):
        params = dataclasses.replace(TerrainBrushParams.engine((2048, 2048), (64, 64), (-700.0, 600.0, -40.0), (1.0, -0.6, 0.1), layer=1, flatten_height_world=200.0),
                                     radius_texels=radius)
        brush = TerrainBrushContext.over(maps, params)
        r.apply_terrain_brush(dataclasses.replace(brush, stages=L.TERRAIN_BRUSH_TRACE))
        torch.cuda.synchronize()
        assert int(brush.hit[3]) == 1, "the timing ray misses the terrain"
        row(f"trace, radius {radius:g}", lambda: r.apply_terrain_brush(dataclasses.replace(brush, stages=L.TERRAIN_BRUSH_TRACE)), radius, 1, 0, 2048)
        for mode, name in enumerate(MODES):
            c = dataclasses.replace(brush, params=dataclasses.replace(params, mode=mode))
            row(f"apply {name}, radius {radius:g}", lambda c=c: r.apply_terrain_brush(dataclasses.replace(c, stages=L.TERRAIN_BRUSH_APPLY)), radius, 2, mode, 2048)
        row(f"trace + apply raise, radius {radius:g}", lambda: r.apply_terrain_brush(brush), radius, 3, 0, 2048)

        derive_texels = 2 * math.ceil(radius + 1.0) + 1
        derive_patches = math.ceil(derive_texels / 32.0) + 1
        rebake = dataclasses.replace(maps, dispatch_texels=(derive_texels,) * 2, dispatch_patches=(derive_patches,) * 2)

        def edit_step():
            r.apply_terrain_brush(brush)
            r.generate_terrain_maps(rebake)

        row(f"edit step (brush + regional re-bake of {derive_texels} texels, {derive_patches} patches a side), radius {radius:g}", edit_step, radius, 3, 0, 2048)

    tiny_maps = TerrainMapsContext.create((2, 2), (1, 1), device=dev)
    r.generate_terrain_maps(tiny_maps)
    tiny = TerrainBrushContext.over(tiny_maps, dataclasses.replace(TerrainBrushParams.engine((2, 2), (1, 1), (10.0, 600.0, -40.0), (0.0, -1.0, 0.0)), radius_texels=1.0))
    row("2 x 2 map, trace + apply raise", lambda: r.apply_terrain_brush(tiny), 1.0, 3, 0, 2)
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
