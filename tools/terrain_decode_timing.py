"""Time oxc_decode_terrain (tools/, not bench.py) over the 2048 x 2048 engine-default maps of terrain_maps_timing.py, baked once, with four
materials on the four layers.  The library has no terrain draw, so the frame is made here: a camera straight above the map's centre that
sees past its edges, every terrain pixel at the depth of a ground plane at 40 % of the height range -- the decode's work per pixel (an
unprojection, eight map loads, the layer blend, four stores) does not depend on the depth's exact value.  Rows: --size (3840x2160) with every
pixel terrain, with the upper half terrain and the lower half mesh texels, and with no terrain pixel; 16 x 16 all terrain; each with the
brush ring off and on (a hit at the map's centre, radius 200).  Prints one JSON line per row: ms per call (HIP events around the call,
median and minimum of --steps after --warmup)."""
import dataclasses

import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd.renderer import ImageAttachment, TerrainData, TerrainDecodeContext, TerrainMapsContext
from oxylus_amd.synth import pack_materials

CAMERA_HEIGHT, NEAR, SCALE = 1500.0, 0.5, 2.0
TERRAIN_TEXEL, MESH_TEXEL = 0xFFFFFE00 - (1 << 32), 0x00000100  # as int32


def inv_projection_view():
    """The inverse of a projection looking straight down from (0, CAMERA_HEIGHT, 0): reverse-Z, ndc.z = NEAR / distance; column-major."""
    view = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, -CAMERA_HEIGHT], [0, 0, 0, 1]], np.float64)
    proj = np.array([[SCALE, 0, 0, 0], [0, SCALE, 0, 0], [0, 0, 0, NEAR], [0, 0, -1, 0]], np.float64)
    return np.linalg.inv(proj @ view).T.reshape(-1).astype(np.float32)


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv)
    r, dev = pf.renderer()
    lines = []

    maps = TerrainMapsContext.create(device=dev)
    r.generate_terrain_maps(maps)
    rng = np.random.default_rng(15)
    materials = pack_materials(rng.random((4, 4)), rng.random((4, 3)), rng.random(4), rng.random(4)).to(dev)
    hit = torch.tensor(np.array([0.0, 160.0, 0.0], np.float32).view(np.int32).tolist() + [1], dtype=torch.int32, device=dev)
    ipv = inv_projection_view()

    def frame(W, H, terrain_rows):
        vis = torch.full((H, W), MESH_TEXEL, dtype=torch.int32, device=dev)
        vis[:terrain_rows] = TERRAIN_TEXEL
        depth = torch.full((H, W), NEAR / (CAMERA_HEIGHT - 160.0), dtype=torch.float32, device=dev)
        z32 = lambda: torch.zeros((H, W), dtype=torch.int32, device=dev)  # noqa: E731
        return TerrainDecodeContext(vis, ImageAttachment.depth(depth), [float(x) for x in ipv], TerrainData.of(layer_material_indices=(0, 1, 2, 3)), (2048, 2048),
                                    maps.normalmap, maps.splatmap, materials, 4, hit, z32(), torch.zeros((H, W, 4), dtype=torch.int16, device=dev), z32(), z32())

    W, H = pf.extent(args.size)
    for name, (w, h, rows) in {"all terrain": (W, H, H), "half terrain": (W, H, H // 2), "no terrain": (W, H, 0), "16 x 16, all terrain": (16, 16, 16)}.items():
        base = frame(w, h, rows)
        for ring in (False, True):
            c = dataclasses.replace(base, terrain=dataclasses.replace(base.terrain, brush_radius=200.0 if ring else 0.0))
            med, mn = pf.time_call(lambda c=c: r.decode_terrain(c), args.steps, args.warmup)
            pf.report(lines, {"workload": "terrain_decode", "call": "decode_terrain", "row": f"{name}, ring {'on' if ring else 'off'}", "size": f"{w}x{h}",
                              "terrain_pixels": w * rows, "ring": ring, "map_resolution": 2048, "ms_median": med, "ms_min": mn})
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
