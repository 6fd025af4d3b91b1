"""What the terrain-map tests share: the settings sets, the edit images, the initial contents of the five outputs, one GPU call between guard
bands and the checker's answer to it (`want`).  Numpy only until `run` is called; the rules come from terrain_maps_model, the guard bands
from gpu_passes.  `python tests/terrain_maps_frames.py` writes the golden fixture tests/golden/terrain_maps_24x20.npz."""
import dataclasses
import os

import numpy as np

import terrain_maps_model as TM

F = np.float32
POISON16, POISON32 = 0xFFFB, 0xFFFFFFFB
IMAGES = ("heightmap", "ridgemap", "normalmap", "splatmap", "height_edit", "splat_edit", "patch_minmax")
OUTPUTS = ("heightmap", "ridgemap", "normalmap", "splatmap", "patch_minmax")
TOUCHED = {TM.GENERATE: ("heightmap", "ridgemap", "height_edit"), TM.DERIVE: ("heightmap", "ridgemap", "normalmap", "splatmap", "splat_edit"),
           TM.MINMAX: ("heightmap", "patch_minmax")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_maps_24x20.npz")
GOLDEN_SHAPE = ((24, 20), (3, 2))

_kept = {}


def engine(resolution, world_size=(1024.0, 1024.0), height_range=(0.0, 400.0), **generate):
    """(Generate, Derive) at the engine's defaults for a Terrain of this resolution: texel_world_size and height_range as Terrain::bake forms
    them, in binary32."""
    tws = tuple(float(F(world_size[k]) / F(resolution[k])) for k in range(2))
    return TM.Generate(**generate), TM.Derive(texel_world_size=tws, height_range=float(F(height_range[1]) - F(height_range[0])))


def with_erosion(G, **erosion):
    return dataclasses.replace(G, erosion=dataclasses.replace(G.erosion, **erosion))


def edits(resolution, seed=3, strokes=True):
    """(height_edit, splat_edit): zero like a fresh terrain, or with a raised disc that clips the heightmap at 1, a dug one that clips it at 0,
    and a painted disc whose weight runs from 0 to 1 across the four layers."""
    W, H = int(resolution[0]), int(resolution[1])
    height_edit, splat_edit = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32)
    if not strokes:
        return height_edit, splat_edit
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    r = max(2.0, min(W, H) / 5.0)
    height_edit += np.where((x - W * 0.25) ** 2 + (y - H * 0.3) ** 2 < r * r, 0.9, 0.0).astype(np.float32)
    height_edit -= np.where((x - W * 0.75) ** 2 + (y - H * 0.7) ** 2 < r * r, 0.9, 0.0).astype(np.float32)
    height_edit += (rng.random((H, W), dtype=np.float32) - F(0.5)) * F(0.01)
    painted = (x - W * 0.6) ** 2 + (y - H * 0.25) ** 2 < r * r
    layer = rng.integers(0, 4, (H, W))
    weight = rng.integers(0, 256, (H, W)).astype(np.uint32)
    word = np.where(layer == 0, 0, np.uint32(255) << (np.uint32(8) * (layer - 1).clip(0).astype(np.uint32))).astype(np.uint32) | (weight << np.uint32(24))
    splat_edit[painted] = word[painted]
    return height_edit, splat_edit


def initial(resolution, patch_count, height_edit=None, splat_edit=None, seed=17):
    """The seven images before a call: the outputs hold random bytes no stage writes by chance everywhere (so an unwritten texel shows), the
    edit images are the given ones or zero."""
    W, H = int(resolution[0]), int(resolution[1])
    rng = np.random.default_rng(seed)
    he, se = edits(resolution, strokes=False)
    return {"heightmap": rng.integers(0, 65536, (H, W)).astype(np.uint16), "ridgemap": rng.integers(0, 0x3C00, (H, W)).astype(np.uint16),
            "normalmap": rng.integers(0, 0x3C00, (H, W, 2)).astype(np.uint16), "splatmap": rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32),
            "height_edit": he if height_edit is None else height_edit, "splat_edit": se if splat_edit is None else splat_edit,
            "patch_minmax": rng.random((int(patch_count[1]), int(patch_count[0]), 2), dtype=np.float32) + F(2.0)}


def want(G, D, resolution, patch_count, images, stages=TM.ALL, region=(0, 0, 0, 0), dispatch_texels=None, dispatch_patches=None, counts=None):
    return TM.terrain_maps(G, D, resolution, patch_count, images, stages, region, dispatch_texels, dispatch_patches, counts)


def engine_48x40():
    """The engine-default frame of the GPU tests, its edits and the checker's five outputs with the branch counts; computed once, read-only."""
    if "48x40" not in _kept:
        res, pc = (48, 40), (5, 3)
        G, D = engine(res)
        he, se = edits(res)
        images = initial(res, pc, he, se)
        counts = {}
        out = want(G, D, res, pc, images, counts=counts)
        for a in list(images.values()) + list(out.values()):
            a.setflags(write=False)
        _kept["48x40"] = (res, pc, G, D, images, out, counts)
    return _kept["48x40"]


def golden_outputs():
    """The five outputs at engine defaults on the 24 x 20 map with 3 x 2 patches and the stroked edits, from zeroed images."""
    res, pc = GOLDEN_SHAPE
    G, D = engine(res)
    he, se = edits(res)
    images = initial(res, pc, he, se)
    out = want(G, D, res, pc, images)
    return {k: out[k] for k in OUTPUTS}


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------------------
def guards(images, names=IMAGES):
    """Every named image between guard bands, holding its numpy contents."""
    import torch

    from gpu_passes import Guard

    gs = {}
    for name in names:
        a = images[name]
        if a.dtype == np.uint16:
            gs[name] = Guard(name, a.shape, torch.int16, a.shape[1] * (a.shape[2] if a.ndim == 3 else 1), POISON16, 4 if a.ndim == 3 else 2, data=a)
        else:
            dtype = torch.float32 if a.dtype == np.float32 else torch.int32
            gs[name] = Guard(name, a.shape, dtype, a.shape[1] * (2 if a.ndim == 3 else 1), POISON32, 8 if a.ndim == 3 else 4, data=a)
    return gs


def renderer_settings(G, D, resolution):
    from oxylus_amd import renderer as R

    g = dataclasses.asdict(G)
    erosion = R.TerrainErosion(**g.pop("erosion"))
    return R.TerrainGenerate(erosion=erosion, resolution=tuple(resolution), **g), R.TerrainDerive(resolution=tuple(resolution), **dataclasses.asdict(D))


def region_tensor(region):
    import torch

    return torch.from_numpy(np.asarray(region, dtype=np.uint32).view(np.int32).copy()).cuda()


def context(G, D, resolution, patch_count, gs, stages=TM.ALL, region=None, dispatch_texels=None, dispatch_patches=None):
    """The renderer's context over the guarded tensors of `gs` (a missing name is a null buffer); `region` a device tensor or None."""
    from oxylus_amd.renderer import TerrainMapsContext

    g, d = renderer_settings(G, D, resolution)
    t = {name: (gs[name].tensor if name in gs else None) for name in IMAGES}
    return TerrainMapsContext(g, d, tuple(resolution), tuple(patch_count), tuple(dispatch_texels or resolution), tuple(dispatch_patches or patch_count),
                              region=region, stages=stages, **t)


def got_of(gs, images) -> dict:
    """The guarded windows as numpy arrays of the images' dtypes and shapes."""
    return {name: g.bits()[1].view(images[name].dtype).reshape(images[name].shape).copy() for name, g in gs.items()}


def run(r, G, D, resolution, patch_count, images, label, stages=TM.ALL, region=None, dispatch_texels=None, dispatch_patches=None, only_touched=False,
        counts=None) -> dict:
    """One oxc_generate_terrain_maps between guard bands: every byte of every image equal to the checker's, the bands untouched.  `region`
    (four integers) goes through device memory, None is the null buffer; `only_touched` binds only what the stages touch and leaves every
    other buffer null.  Returns the images after the call."""
    import torch

    from gpu_passes import same

    names = IMAGES
    if only_touched:
        names = tuple(n for n in IMAGES if any(n in TOUCHED[s] for s in TOUCHED if s & stages))
    gs = guards(images, names)
    r.generate_terrain_maps(context(G, D, resolution, patch_count, gs, stages, None if region is None else region_tensor(region), dispatch_texels, dispatch_patches))
    torch.cuda.synchronize()
    expected = want(G, D, resolution, patch_count, images, stages, region or (0, 0, 0, 0), dispatch_texels, dispatch_patches, counts)
    got = got_of(gs, images)
    for name, g in gs.items():
        g.check(label)
        same(got[name], expected[name], f"{label}: {name}")
    return {**expected, **got}


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **golden_outputs())
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
