"""Time oxc_draw_terrain (tools/, not bench.py) over the 2048 x 2048 engine-default bake of terrain_maps_timing.py with its 64 x 64 patches,
engine defaults (16 px edges, factor 64), every patch in the list (no cull in front of it: the worst case).  Rows at --size (3840x2160):
a camera straight above the map's centre, a grazing camera a few units above the highest ground, and a camera that looks up so that no
terrain is in view (every patch is still tessellated; nothing reaches a pixel); and the look-down call at 16 x 16 for the launch cost.  Each
row with `clear`.  Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after --warmup) and
what oxc_debug_terrain_draw_stats counted."""
import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd.renderer import TerrainData, TerrainDrawContext, TerrainMapsContext

NEAR, SCALE = 0.5, 2.0


def look_at(eye, target, up_hint):
    """projection_view, column-major binary32: right-handed, +y of the image down, reverse-Z with an infinite far plane."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, np.asarray(up_hint, np.float64))
    r /= np.linalg.norm(r)
    up = np.cross(r, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = r, -up, -f
    view[:3, 3] = -view[:3, :3] @ eye
    proj = np.array([[SCALE, 0, 0, 0], [0, SCALE, 0, 0], [0, 0, 0, NEAR], [0, 0, -1, 0]], np.float64)
    return (proj @ view).T.reshape(-1).astype(np.float32)


CAMERAS = {"look-down": ((0.0, 1500.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)), "grazing": ((-300.0, 420.0, -200.0), (400.0, 330.0, 300.0), (0.0, 1.0, 0.0)),
           "no terrain in view": ((0.0, 1500.0, 0.0), (0.0, 3000.0, 0.0), (0.0, 0.0, 1.0))}


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv)
    r, dev = pf.renderer()
    lines = []
    maps = TerrainMapsContext.create(device=dev)
    r.generate_terrain_maps(maps)
    T = TerrainData.of()
    patches = T.patch_count[0] * T.patch_count[1]
    visible = torch.arange(patches, dtype=torch.int32, device=dev)
    cmd = torch.tensor([4, patches, 0, 0], dtype=torch.int32, device=dev)
    h, w = maps.heightmap.shape[:2]
    W, H = pf.extent(args.size)
    rows = [(name, W, H) for name in CAMERAS] + [("look-down", 16, 16)]
    for name, ww, hh in rows:
        eye, target, up = CAMERAS[name]
        visdepth = torch.zeros((hh, ww), dtype=torch.int64, device=dev)
        c = TerrainDrawContext(visdepth, [float(x) for x in look_at(eye, target, up)], eye, NEAR, float(np.float32(hh * 0.5 * SCALE)), T, (int(w), int(h)), maps.heightmap,
                               visible, cmd, True)
        med, mn = pf.time_call(lambda c=c: r.draw_terrain_for_visbuffer(c), args.steps, args.warmup)
        stats = r.debug_terrain_draw_stats()
        pf.report(lines, {"workload": "terrain_draw", "call": "draw_terrain_for_visbuffer", "row": name, "size": f"{ww}x{hh}", "patches": patches, "map_resolution": int(w),
                          "covered_pixels": int((visdepth != 0).sum()), **{k: v for k, v in stats.items() if k != "fragments"}, "ms_median": med, "ms_min": mn})
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
