"""What the terrain-brush tests share: heightmaps (flat, ramp, a ridge that gives two crossings, a pit), rays, the params built the way
Passes/Terrain.cpp:42-67 builds them, the edit images, one GPU call between guard bands and the checker's answer to it.  Numpy only until
`run` is called; the rules come from terrain_brush_model, the guard bands from gpu_passes.  `python tests/terrain_brush_frames.py` writes
the golden fixture tests/golden/terrain_brush_24x20.npz (inputs and expected hit / region / edit images only)."""
import dataclasses
import os

import numpy as np

import terrain_brush_model as TB

F = np.float32
POISON16, POISON32 = 0xFFFB, 0xFFFFFFFB
IMAGES = ("heightmap", "height_edit", "splat_edit", "hit", "region")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_brush_24x20.npz")
GOLDEN_SHAPE = ((24, 20), (3, 5))
WORLD = (1024.0, 1024.0)
FLAT_Q = 16384  # the flat map's texel: a quarter of the height range


def touched(stages, mode):
    """The buffers the requested stages touch (the header's table)."""
    names = set()
    if stages & TB.TRACE:
        names |= {"heightmap", "hit", "region"}
    if stages & TB.APPLY:
        names |= {"splat_edit", "hit"} if mode == TB.PAINT_LAYER else {"heightmap", "height_edit", "hit"}
    return tuple(n for n in IMAGES if n in names)


# ---- heightmaps ------------------------------------------------------------------------------------------------------------------------------------
def heightmap(kind, resolution, seed=5):
    W, H = int(resolution[0]), int(resolution[1])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "flat":
        h = np.full((H, W), FLAT_Q / 65535.0)
    elif kind == "zero":
        h = np.zeros((H, W))
    elif kind == "ramp":
        h = 0.1 + 0.6 * x / max(W - 1, 1) + 0.1 * y / max(H - 1, 1)
    elif kind == "ridge":  # a wall across x at 40 % of the width, ground behind it
        h = np.where(np.abs(x - 0.4 * W) < max(1.0, 0.06 * W), 0.8, 0.1)
    elif kind == "pit":
        h = 0.6 - 0.5 * np.exp(-((x - W / 2) ** 2 + (y - H / 2) ** 2) / max(2.0, (min(W, H) / 4.0) ** 2))
    else:
        h = np.random.default_rng(seed).random((H, W))
    return np.floor(np.clip(h, 0, 1) * 65535.0 + 0.5).astype(np.uint16)


def edits(resolution, seed=9):
    """(height_edit, splat_edit) with earlier strokes in them: heights in [-1, 1], some at the ends, and random painted words."""
    W, H = int(resolution[0]), int(resolution[1])
    rng = np.random.default_rng(seed)
    he = ((rng.random((H, W), dtype=np.float32) - F(0.5)) * F(1.6)).astype(np.float32)
    he.reshape(-1)[::7] = F(0.9995)
    he.reshape(-1)[3::11] = F(-0.9995)
    se = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)
    return he, se


# ---- params ----------------------------------------------------------------------------------------------------------------------------------------
def params(resolution, patch_count, ray_origin, ray_direction, radius_world=64.0, mode=TB.RAISE, layer=0, falloff=1.0, height_rate=4.0, blend_rate=3.0,
           flatten_height_world=0.0, invert=False, delta_time=1.0 / 60.0, world_size=WORLD, height_range=(0.0, 400.0), strength=None, radius_texels=None):
    """GPU::TerrainBrushParams of a Terrain at the origin the way RendererInstance::apply_terrain_brush forms them, in binary32.  `strength` /
    `radius_texels` replace the derived values."""
    ws, res = [F(v) for v in world_size], [F(float(v)) for v in resolution]
    texel = [ws[k] / res[k] for k in range(2)]
    base, scale = F(height_range[0]), F(height_range[1]) - F(height_range[0])
    height_scale = max(scale, F(1e-3))
    dt = min(max(F(delta_time), F(0.0)), F(1.0) / F(30.0))
    if strength is None:
        strength = F(height_rate) * dt / height_scale if mode in (TB.RAISE, TB.NOISE) else min(max(F(blend_rate) * dt, F(0.0)), F(1.0))
        strength = -strength if invert else strength
    if radius_texels is None:
        radius_texels = F(radius_world) / max(texel[0], texel[1])
    return TB.Params(tuple(float(F(v)) for v in ray_origin), float(F(radius_texels)), tuple(float(F(v)) for v in ray_direction), float(F(strength)),
                     tuple(int(v) for v in resolution), tuple(float(-w * F(0.5)) for w in ws), tuple(float(w) for w in ws), tuple(float(F(1.0) / w) for w in ws),
                     tuple(int(v) for v in patch_count), float(base), float(scale), float(falloff),
                     float(min(max((F(flatten_height_world) - base) / height_scale, F(0.0)), F(1.0))), int(mode), int(layer))


def flat_height():
    """The world height of the flat map, in binary64."""
    return FLAT_Q / 65535.0 * 400.0


def ray_crossing_at_step(k, z=10.0, slope=0.25):
    """A ray from outside the -x edge of the 1024-unit world that crosses the flat map's height midway between march steps k - 1 and k: the
    span is x in [-512, 512], 2 world units a step; y falls by `slope` a unit of x."""
    return (-600.0, flat_height() + slope * (88.0 + 2.0 * k - 1.0), z), (1.0, -slope, 0.0)


def ray_down_at(texel, resolution, y=500.0, world_size=WORLD):
    """A vertical ray over the centre of texel (x, y)."""
    wx = -world_size[0] / 2 + (texel[0] + 0.5) * world_size[0] / resolution[0]
    wz = -world_size[1] / 2 + (texel[1] + 0.5) * world_size[1] / resolution[1]
    return (wx, y, wz), (0.0, -1.0, 0.0)


def initial(resolution, kind="ramp", strokes=True):
    """The five buffers before a call; hit and region hold poison the trace must overwrite."""
    he, se = edits(resolution)
    if not strokes:
        he, se = np.zeros_like(he), np.zeros_like(se)
    return {"heightmap": heightmap(kind, resolution), "height_edit": he, "splat_edit": se, "hit": np.full(4, 0xDEADBEEF, np.uint32),
            "region": np.full(4, 0xDEADBEEF, np.uint32)}


def want(B, images, stages=TB.BOTH, counts=None, info=None):
    return TB.terrain_brush(B, images, stages, counts, info)


def golden_case():
    """(params, inputs) of the fixture: a slanted ray onto the 24 x 20 ramp, Smooth at 2.5 texels."""
    res, pc = GOLDEN_SHAPE
    B = params(res, pc, (-300.0, 420.0, -150.0), (0.6, -0.7, 0.35), mode=TB.SMOOTH, radius_texels=2.5, strength=0.75)
    return B, initial(res)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------------------
def guards(images, names=IMAGES):
    import torch

    from gpu_passes import Guard

    gs = {}
    for name in names:
        a = images[name]
        if a.dtype == np.uint16:
            gs[name] = Guard(name, a.shape, torch.int16, a.shape[1], POISON16, 2, data=a)
        elif a.ndim == 1:
            gs[name] = Guard(name, a.shape, torch.int32, 4, POISON32, 8, data=a)
        else:
            gs[name] = Guard(name, a.shape, torch.float32 if a.dtype == np.float32 else torch.int32, a.shape[1], POISON32, 4, data=a)
    return gs


def renderer_params(B):
    from oxylus_amd.renderer import TerrainBrushParams

    return TerrainBrushParams(**dataclasses.asdict(B))


def context(B, gs, stages=TB.BOTH):
    """The renderer's context over the guarded tensors of `gs` (a missing name is a null buffer)."""
    from oxylus_amd.renderer import TerrainBrushContext

    return TerrainBrushContext(renderer_params(B), stages=stages, **{name: (gs[name].tensor if name in gs else None) for name in IMAGES})


def got_of(gs, images) -> dict:
    return {name: g.bits()[1].view(images[name].dtype).reshape(images[name].shape).copy() for name, g in gs.items()}


def run(r, B, images, label, stages=TB.BOTH, only_touched=False, counts=None, info=None) -> dict:
    """One oxc_apply_terrain_brush between guard bands: every byte of every bound buffer equal to the checker's, the bands untouched.
    `only_touched` binds only what the stages touch and leaves every other buffer null.  Returns the buffers after the call."""
    import torch

    from gpu_passes import same

    names = touched(stages, B.mode) if only_touched else IMAGES
    gs = guards(images, names)
    r.apply_terrain_brush(context(B, gs, stages))
    torch.cuda.synchronize()
    expected = want(B, images, stages, counts, info)
    got = got_of(gs, images)
    for name, g in gs.items():
        g.check(label)
        same(got[name], expected[name], f"{label}: {name}")
    return {**expected, **got}


if __name__ == "__main__":
    B, images = golden_case()
    out = want(B, images)
    stored = {"in_" + k: v for k, v in images.items()}
    stored.update({"out_" + k: out[k] for k in ("hit", "region", "height_edit", "splat_edit")})
    paint = want(dataclasses.replace(B, mode=TB.PAINT_LAYER, layer=2), images)
    stored["out_splat_edit_paint"] = paint["splat_edit"]
    np.savez_compressed(GOLDEN, **stored)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
