"""What the terrain-decode tests share: the maps (the 24 x 20 bake of terrain_maps_model, 1 x 1 and 2 x 2 by hand), a camera that looks down
on the map from high enough to see past all four of its edges, the terrain texels and their depth -- made here on the CPU by marching each
pixel's ray against the bilinear heightmap, which stands in for the tessellated draw the library does not have -- materials, the images
the earlier passes left, one GPU call between guard bands and the checker's answer to it.  Numpy only until `run` is called; the rules come
from terrain_decode_model, the guard bands from gpu_passes.  `python tests/terrain_decode_frames.py` writes the golden fixture
tests/golden/terrain_decode_17x9.npz (inputs and expected outputs only)."""
import dataclasses
import os

import numpy as np

import terrain_decode_model as TD
import terrain_maps_frames as TF

F = np.float32
POISON16, POISON32 = 0xFFFB, 0xFFFFFFFB
INPUTS = ("vis", "depth", "normalmap", "splatmap", "materials", "hit")
OUTPUTS = TD.IMAGES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_decode_17x9.npz")
WORLD = (1024.0, 1024.0)
HEIGHT_RANGE = (0.0, 400.0)
CAMERA_HEIGHT, NEAR, FOV_SCALE = 1500.0, 0.5, 2.0  # at ground level the view spans about +-660 world units on both axes: the map ends at +-512
EXTENTS = ((1, 1), (7, 5), (17, 9), (33, 19))

_kept = {}


# ---- the terrain and its maps ----------------------------------------------------------------------------------------------------------------------
def terrain(layers=(0, 1, 2, 3), brush_radius=0.0, world_size=WORLD, height_range=HEIGHT_RANGE, **kw) -> TD.Terrain:
    """GPU::TerrainData of a Terrain centred on the origin, in binary32."""
    ws = [F(v) for v in world_size]
    return TD.Terrain(tuple(float(-w * F(0.5)) for w in ws), tuple(float(w) for w in ws), tuple(float(F(1.0) / w) for w in ws), (3, 2), float(F(height_range[0])),
                      float(F(height_range[1]) - F(height_range[0])), layer_material_indices=tuple(int(v) for v in layers), brush_radius=float(brush_radius), **kw)


def baked_maps():
    """heightmap, normalmap and splatmap of the 24 x 20 engine-default bake with the stroked edits (terrain_maps_model); computed once, read-only."""
    if "baked" not in _kept:
        out = TF.golden_outputs()
        maps = {k: out[k] for k in ("heightmap", "normalmap", "splatmap")}
        for a in maps.values():
            a.setflags(write=False)
        _kept["baked"] = maps
    return _kept["baked"]


def half_bits(v) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)


def hand_maps(resolution, normals, splat_words, height_q=16384):
    """A flat heightmap with the given normal-map values (floats [h, w, 2], or uint16 bit patterns) and splat words."""
    w, h = resolution
    n = np.asarray(normals)
    n = n.astype(np.uint16) if np.issubdtype(n.dtype, np.integer) else half_bits(n)
    return {"heightmap": np.full((h, w), height_q, np.uint16), "normalmap": np.broadcast_to(n, (h, w, 2)).copy(),
            "splatmap": np.broadcast_to(np.asarray(splat_words, np.uint32), (h, w)).copy()}


def flat_maps(resolution=(2, 2), splat=0x000000FF):
    return hand_maps(resolution, np.zeros(2, np.float32), splat)


# ---- the camera and the stand-in for the draw ------------------------------------------------------------------------------------------------------
def camera(W, H, eye=(0.0, CAMERA_HEIGHT, 0.0), scale=FOV_SCALE):
    """(projection_view, inv_projection_view) as binary32 [16], column-major: the eye looks straight down, +x to the right and +z down the
    image, the same field of view on both axes whatever W and H are; reverse-Z with an infinite far plane, ndc.z = NEAR / distance."""
    view = np.array([[1, 0, 0, -eye[0]], [0, 0, 1, -eye[2]], [0, 1, 0, -eye[1]], [0, 0, 0, 1]], np.float64)  # view z = y - eye.y: negative below the eye
    proj = np.array([[scale, 0, 0, 0], [0, scale, 0, 0], [0, 0, 0, NEAR], [0, 0, -1, 0]], np.float64)
    pv = proj @ view
    return pv.T.reshape(-1).astype(np.float32), np.linalg.inv(pv).T.reshape(-1).astype(np.float32)


def _height64(T, heightmap, wx, wz):
    """The bilinear heightmap in binary64 with clamped texels: the surface the stand-in draw rasterises."""
    h, w = heightmap.shape
    q = heightmap.astype(np.float64) / 65535.0
    gx = (wx - T.world_min[0]) * T.inv_world_size[0] * w - 0.5
    gy = (wz - T.world_min[1]) * T.inv_world_size[1] * h - 0.5
    x0, y0 = np.floor(gx), np.floor(gy)
    fx, fy = gx - x0, gy - y0
    cx = lambda v: np.clip(v, 0, w - 1).astype(np.int64)  # noqa: E731
    cy = lambda v: np.clip(v, 0, h - 1).astype(np.int64)  # noqa: E731
    top = q[cy(y0), cx(x0)] * (1 - fx) + q[cy(y0), cx(x0 + 1)] * fx
    bot = q[cy(y0 + 1), cx(x0)] * (1 - fx) + q[cy(y0 + 1), cx(x0 + 1)] * fx
    return T.base_height + (top * (1 - fy) + bot * fy) * T.height_scale


def draw(T, heightmap, W, H, pv, ipv, steps=192, refine=20):
    """(vis uint32 [H, W], depth float32 [H, W]): every pixel's ray from the eye marched down to the heightmap, bisected; the depth is the
    hit's clip.z / clip.w, the texel 0xFFFFFE << 8."""
    m, mi = pv.astype(np.float64).reshape(4, 4).T, ipv.astype(np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * 2 - 1], axis=-1)
    at = lambda d: (lambda h: h[..., :3] / h[..., 3:])(np.concatenate([ndc, np.full((H, W, 1), d), np.ones((H, W, 1))], axis=-1) @ mi.T)  # noqa: E731
    a, b = at(1.0), at(NEAR / (CAMERA_HEIGHT * 4.0))  # from the near plane to far below the ground
    gap = lambda t: (lambda p: p[..., 1] - _height64(T, heightmap, p[..., 0], p[..., 2]))(a + (b - a) * t[..., None])  # noqa: E731
    ts = np.linspace(0.0, 1.0, steps + 1)
    gaps = np.stack([gap(np.full((H, W), t)) for t in ts], axis=0)
    first = np.argmax(gaps <= 0, axis=0)
    assert (gaps[0] > 0).all() and (gaps[-1] <= 0).all()
    lo, hi = ts[first - 1], ts[first]
    for _ in range(refine):
        mid = (lo + hi) * 0.5
        above = gap(mid) > 0
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    p = a + (b - a) * hi[..., None]
    clip = np.concatenate([p, np.ones((H, W, 1))], axis=-1) @ m.T
    return np.full((H, W), TD.TERRAIN_TEXEL, np.uint32), (clip[..., 2] / clip[..., 3]).astype(np.float32)


def mix_texels(vis, depth, pattern="mixed", seed=23):
    """The frame's other pixel classes laid over the all-terrain one: "all", "none" (mesh texels and ~0u only), "checker" (terrain and mesh
    texels alternating), "mixed" (about 1 in 7 a mesh texel, 1 in 11 ~0u, 1 in 13 a terrain texel whose depth bits are 0)."""
    H, W = vis.shape
    rng = np.random.default_rng(seed)
    vis, depth = vis.copy(), depth.copy()
    mesh = (rng.integers(0, 0xFFFFFD, (H, W)).astype(np.uint32) << np.uint32(8)) | rng.integers(0, 256, (H, W)).astype(np.uint32)
    ys, xs = np.mgrid[0:H, 0:W]
    k = ys * W + xs
    if pattern == "none":
        vis = np.where(k % 3 == 0, np.uint32(0xFFFFFFFF), mesh)
    elif pattern == "checker":
        vis = np.where((xs + ys) % 2 == 0, vis, mesh)
    elif pattern == "mixed":
        vis = np.where(k % 7 == 3, mesh, vis)
        vis = np.where(k % 11 == 5, np.uint32(0xFFFFFFFF), vis)
        depth = np.where(k % 13 == 6, F(0.0), depth)
    else:
        assert pattern == "all"
    return vis.astype(np.uint32), depth.astype(np.float32)


# ---- materials, the hit, the images before the call ----------------------------------------------------------------------------------------------------
MATERIAL_FACTORS = (  # albedo rgba, emissive rgb, roughness, metallic: grass, rock, sand, snow (snow glows a little, so the emissive sums are not all zero)
    (0.13, 0.35, 0.08, 1.0, 0.0, 0.0, 0.0, 0.9, 0.0),
    (0.30, 0.28, 0.26, 1.0, 0.0, 0.0, 0.0, 0.7, 0.1),
    (0.76, 0.70, 0.50, 0.5, 0.0, 0.0, 0.0, 0.8, 0.0),
    (0.95, 0.95, 0.97, 1.0, 0.02, 0.03, 0.25, 0.3, 0.0),
    (0.001, 0.002, 0.0005, 1.0, 3.0, 70000.0, 0.0, 0.0, 1.0),  # below the sRGB knee; an emissive beyond 2^16
)


def materials(factors=MATERIAL_FACTORS) -> np.ndarray:
    """uint8 [56 * n] GPU::Material records: a row of nine floats is rounded to binary16, a row of integers is the half bit patterns."""
    rec = np.zeros((len(factors), 28), np.uint16)
    for i, row in enumerate(factors):
        row = np.asarray(row)
        rec[i, :9] = row.astype(np.uint16) if np.issubdtype(row.dtype, np.integer) else half_bits(row)
    return rec.view(np.uint8).reshape(-1).copy()


def hit_record(position=(0.0, 0.0, 0.0), valid=1) -> np.ndarray:
    return np.concatenate([np.asarray(position, np.float32).view(np.uint32), np.array([valid], np.uint32)])


POISONED_HIT = np.full(4, 0xFFC0DEAD, np.uint32)  # a NaN position and a non-zero valid: it must not be read while brush_radius > 0 is false


def earlier_images(W, H, seed=41) -> dict:
    """The four attachments as earlier passes left them: bytes the terrain decode writes nowhere by chance everywhere."""
    rng = np.random.default_rng(seed)
    r32 = lambda: rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)  # noqa: E731
    return {"albedo": r32(), "normal": rng.integers(0, 0x3C00, (H, W, 4)).astype(np.uint16), "emissive": r32(), "mro": r32()}


@dataclasses.dataclass
class Frame:
    T: TD.Terrain
    W: int
    H: int
    ipv: np.ndarray
    inputs: dict       # INPUTS -> numpy (materials / hit may be None)
    material_count: int
    init: dict         # OUTPUTS -> numpy
    pv: np.ndarray = None


def frame(extent=(17, 9), maps=None, T=None, pattern="mixed", factors=MATERIAL_FACTORS, hit=None, eye=(0.0, CAMERA_HEIGHT, 0.0), seed=41) -> Frame:
    W, H = extent
    T = terrain() if T is None else T
    maps = baked_maps() if maps is None else maps
    pv, ipv = camera(W, H, eye)
    vis, depth = mix_texels(*draw(T, maps["heightmap"], W, H, pv, ipv), pattern)
    mats = None if factors is None else materials(factors)
    inputs = {"vis": vis, "depth": depth, "normalmap": maps["normalmap"], "splatmap": maps["splatmap"], "materials": mats, "hit": hit}
    return Frame(T, W, H, ipv, inputs, 0 if factors is None else len(factors), earlier_images(W, H, seed), pv)


def want(f: Frame, counts=None, pre=None) -> dict:
    i = f.inputs
    return TD.decode(f.T, i["vis"], i["depth"], f.ipv, i["normalmap"], i["splatmap"], i["materials"], f.material_count, i["hit"], f.init, counts, pre)


def golden_frame() -> Frame:
    """The fixture: 17 x 9 pixels over the baked 24 x 20 map, four valid layers, the ring around a hit left of the centre."""
    return frame((17, 9), T=terrain(brush_radius=260.0), hit=hit_record((-180.0, 120.0, 90.0)))


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------------------
def guards(f: Frame) -> dict:
    import torch

    from gpu_passes import Guard

    gs = {}
    for name, a in list(f.inputs.items()) + list(f.init.items()):
        if a is None:
            continue
        if a.dtype == np.uint16:  # normalmap [h, w, 2] and normal [H, W, 4]
            gs[name] = Guard(name, a.shape, torch.int16, a.shape[1] * a.shape[2], POISON16, 2 * a.shape[2], data=a)
        elif a.dtype == np.uint8:
            words = a.view(np.uint32)
            gs[name] = Guard(name, words.shape, torch.int32, 14, POISON32, 4, data=words)
        elif a.ndim == 1:
            gs[name] = Guard(name, a.shape, torch.int32, 4, POISON32, 8, data=a)
        else:
            gs[name] = Guard(name, a.shape, torch.float32 if a.dtype == np.float32 else torch.int32, a.shape[1], POISON32, 4, data=a)
    return gs


def renderer_terrain(T: TD.Terrain):
    from oxylus_amd.renderer import TerrainData

    return TerrainData(**dataclasses.asdict(T))


def context(f: Frame, gs: dict, **replace):
    """The renderer's context over the guarded tensors of `gs` (a missing name is a null buffer)."""
    from oxylus_amd.renderer import ImageAttachment, TerrainDecodeContext

    t = lambda name: gs[name].tensor if name in gs else None  # noqa: E731
    h, w = f.inputs["splatmap"].shape
    c = TerrainDecodeContext(t("vis"), ImageAttachment.depth(t("depth")), [float(x) for x in f.ipv], renderer_terrain(f.T), (w, h), t("normalmap"), t("splatmap"),
                             t("materials"), f.material_count, t("hit"), t("albedo"), t("normal"), t("emissive"), t("mro"))
    return dataclasses.replace(c, **replace)


def got_of(gs, f: Frame) -> dict:
    return {name: gs[name].bits()[1].view(f.init[name].dtype).reshape(f.init[name].shape).copy() for name in OUTPUTS}


def check_unwritten(gs, f: Frame, label):
    """Nothing written: the four outputs hold their earlier bytes, every band its poison."""
    from gpu_passes import same

    for g in gs.values():
        g.check(label)
    same(got_of(gs, f), f.init, f"{label}: written after a refusal")


def run(r, f: Frame, label, counts=None) -> dict:
    """One oxc_decode_terrain between guard bands: every word of the four outputs equal to the checker's (so every pixel that is not terrain
    keeps its earlier bytes), every input unchanged, the bands untouched.  Returns the outputs."""
    import torch

    from gpu_passes import same

    gs = guards(f)
    r.decode_terrain(context(f, gs))
    torch.cuda.synchronize()
    for g in gs.values():
        g.check(label)
    got = got_of(gs, f)
    same(got, want(f, counts), label)
    for name, a in f.inputs.items():
        if a is not None:
            same(gs[name].bits()[1], np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.uint16 else np.uint32).reshape(-1), f"{label}: input {name}")
    return got


if __name__ == "__main__":
    f = golden_frame()
    stored = {"in_" + k: v for k, v in f.inputs.items()}
    stored.update({"init_" + k: v for k, v in f.init.items()})
    stored.update({"out_" + k: v for k, v in want(f).items()})
    stored["ipv"] = f.ipv
    np.savez_compressed(GOLDEN, **stored)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
