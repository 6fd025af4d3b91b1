"""The frames of the sprite tests: hand-made sprite lists, materials, world matrices, depths and lit images, the checker's call over them and
the GPU calls between guard bands.  The rules come from sprites_model, the guard bands from gpu_passes.  `python tests/sprites_frames.py`
writes the golden fixture tests/golden/sprites_17x9.npz: the 17 x 9 frame's inputs and, for both formats and the three stage sets, the
checker's depth, visbuffer and colour words."""
import dataclasses
import os
import types

import numpy as np

import pixel_rules as PR
import sprites_model as SM

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sprites_17x9.npz")
POISON32, POISON16 = 0xFFFFFFFB, 0xFFFB
FILL_VIS = 0x0BADBAD0   # visbuffer_2d's pre-fill: `clear` must overwrite it everywhere
IDENTITY = np.eye(4, dtype=F).T.reshape(16)
# the kernel's named constants (oxylus_amd/csrc/oxcull_kernels.hpp)
BIN, TILE, CHUNK, BIN_CAPACITY = 128, 16, 256, 2048
STAGES = (SM.VIS, SM.COLOR, SM.ALL)
FORMATS = (SM.B10G11R11, SM.RGBA16F)


def column_major(rows) -> np.ndarray:
    return np.asarray(rows, F).T.reshape(16).copy()


def quad(W, H, cx, cy, w, h, z, angle=0.0, shear=0.0, mirror=False) -> np.ndarray:
    """The world matrix that, under the identity projection_view, puts the unit sprite on the pixel rectangle of w x h pixels centred at pixel
    coordinates (cx, cy), at depth z; rotated by `angle`, sheared, or mirrored (negative determinant)."""
    c, s = np.cos(angle), np.sin(angle)
    ax = np.array([c * w, s * w]) * (-1.0 if mirror else 1.0)
    ay = np.array([-s * h + shear * w, c * h])
    sx, sy = 2.0 / W, 2.0 / H
    return column_major([[ax[0] * sx, ay[0] * sx, 0, cx * sx - 1.0], [ax[1] * sy, ay[1] * sy, 0, cy * sy - 1.0], [0, 0, 1, z], [0, 0, 0, 1]])


def materials_of(colors, cutoffs=None) -> np.ndarray:
    """uint16 [M, 28] GPU::Material records: albedo_color and alpha_cutoff, the rest zero."""
    colors = np.asarray(colors, F).reshape(-1, 4)
    rec = np.zeros((len(colors), 28), np.uint16)
    rec[:, 0:4] = PR.to_half_bits(colors)
    rec[:, 9] = PR.to_half_bits(np.zeros(len(colors), F) - F(1.0) if cutoffs is None else np.asarray(cutoffs, F))
    return rec


def sprites_of(entries) -> np.ndarray:
    """[(transform_id, material_id[, flags])] -> uint32 [n, 3]."""
    return np.array([SM.pack_sprite(e[2] if len(e) > 2 else 0, 0.0, e[0], e[1], 1.0) for e in entries], np.uint32).reshape(-1, 3)


@dataclasses.dataclass
class Frame:
    sprites: np.ndarray     # uint32 [n, 3]
    materials: np.ndarray   # uint16 [M, 28]
    transforms: np.ndarray  # float32 [T, 16]
    depth: np.ndarray       # float32 [H, W]
    color: np.ndarray       # uint32 [H, W]
    pv: np.ndarray = dataclasses.field(default_factory=lambda: IDENTITY.copy())
    first_sprite: int = 0
    sprite_count: int = None
    material_count: int = None
    transform_count: int = None
    clear: bool = True
    vis: np.ndarray = None  # what visbuffer_2d holds before a call without `clear`

    @property
    def extent(self):
        return self.depth.shape[1], self.depth.shape[0]

    @property
    def counts(self):
        return (len(self.sprites) - self.first_sprite if self.sprite_count is None else self.sprite_count,
                len(self.materials) if self.material_count is None else self.material_count,
                len(self.transforms) if self.transform_count is None else self.transform_count)

    def color_in(self, fmt):
        """The lit image in `fmt`: the B10G11R11 words, or the same colours as four halves with a varying alpha."""
        if fmt == SM.B10G11R11:
            return self.color
        r, g, b = PR.unpack_b10g11r11(self.color)
        a = ((np.arange(self.color.size).reshape(self.color.shape) % 5) / 4.0).astype(F)
        return np.stack([PR.channel_half(c) for c in (r, g, b, a)], axis=-1).astype(np.uint16)


def background(W, H, seed=5, depth=0.25):
    rng = np.random.default_rng(seed + 1000 * W + H)
    d = np.full((H, W), depth, F) if depth is not None else rng.random((H, W)).astype(F)
    color = PR.pack_b10g11r11(*(rng.random((H, W)).astype(F) * F(2.0) for _ in range(3))).reshape(H, W).astype(np.uint32)
    return d, color


PALETTE = [(1.0, 0.25, 0.0, 0.5), (0.0, 0.75, 0.5, 0.25), (0.125, 0.5, 1.5, 0.75), (2.0, 1.0, 0.25, 0.625), (0.3, 0.6, 0.9, 0.4), (0.9, 0.1, 0.7, 0.3),
           (0.5, 0.5, 0.5, 1.0), (0.05, 0.95, 0.35, 0.55)]


def stack_frame(extent=(17, 9), n=8, seed=5, same_depth=True, cover=None) -> Frame:
    """n translucent sprites of different colours over one pixel region (`cover` = (cx, cy, w, h), default most of the image), at one depth
    or from back (far, small z) to front."""
    W, H = extent
    cx, cy, w, h = cover or (W / 2.0 + 0.25, H / 2.0 - 0.25, W * 0.75, H * 0.75)
    d, color = background(W, H, seed)
    transforms = np.stack([quad(W, H, cx + 0.37 * k, cy - 0.21 * k, w, h, 0.5 if same_depth else 0.3 + 0.05 * k, angle=0.1 * k) for k in range(n)])
    mats = materials_of([PALETTE[k % len(PALETTE)] for k in range(n)])
    return Frame(sprites_of([(k, k) for k in range(n)]), mats, transforms, d, color)


def golden_frame() -> Frame:
    """17 x 9: five sprites -- rotated, sheared, flipped, one behind the scene depth, one with a discarding material -- over a random depth."""
    W, H = 17, 9
    d, color = background(W, H, 7, depth=None)
    d = (d * F(0.5)).astype(F)
    transforms = np.stack([quad(W, H, 6, 4, 9, 6, 0.4, angle=0.3), quad(W, H, 10, 5, 8, 5, 0.4, shear=0.4), quad(W, H, 3, 3, 5, 7, 0.6, angle=-0.5),
                           quad(W, H, 12, 2, 9, 3, 0.1), quad(W, H, 8, 4, 17, 9, 0.9)])
    mats = materials_of(PALETTE[:4] + [(1.0, 1.0, 1.0, 0.25)], cutoffs=[-1, 0.1, -1, -1, 0.5])
    return Frame(sprites_of([(0, 0), (1, 1), (2, 2, SM.FLIP_X), (3, 3), (4, 4)]), mats, transforms, d, color)


def want(f: Frame, stages=SM.ALL, fmt=SM.B10G11R11, stats=None, **kw) -> dict:
    W, H = f.extent
    n, m, t = f.counts
    return SM.draw(f.sprites, f.materials, f.transforms, f.pv, W, H, f.depth, vis=f.vis, color=f.color_in(fmt), stages=stages, clear=f.clear, source_format=fmt,
                   first_sprite=f.first_sprite, sprite_count=n, material_count=m, transform_count=t, stats=stats, **kw)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------------
def guards(f: Frame, stages=SM.ALL, fmt=SM.B10G11R11) -> dict:
    import torch

    from gpu_passes import Guard

    W, H = f.extent
    gs = {}
    for name, a in (("sprites", f.sprites), ("materials", f.materials), ("transforms", f.transforms), ("depth", f.depth)):
        if a.size == 0:
            a = np.zeros((1, a.shape[1]), a.dtype)  # a zero-length buffer still has an address
        dtype = torch.float32 if a.dtype == np.float32 else torch.int16 if a.dtype == np.uint16 else torch.int32
        gs[name] = Guard(name, a.shape, dtype, W if name == "depth" else a.shape[1], POISON16 if a.dtype == np.uint16 else POISON32, 4, data=a)
    if stages & SM.VIS:
        gs["vis"] = Guard("vis", (H, W), torch.int32, W, POISON32, 4, **(dict(fill=FILL_VIS) if f.clear else dict(data=f.vis)))
    if stages & SM.COLOR:
        c = f.color_in(fmt)
        gs["color"] = Guard("color", c.shape, torch.int16 if fmt else torch.int32, W * (4 if fmt else 1), POISON16 if fmt else POISON32, 8 if fmt else 4, data=c)
    return gs


def prepared_frame(gs: dict, f: Frame):
    from oxylus_amd.renderer import PreparedFrame

    scene = types.SimpleNamespace(n_mesh_instances=0, meshes=None, transforms=gs["transforms"].tensor, mesh_instances=None)
    return PreparedFrame(scene, 0, None, None, None, None)


def context(f: Frame, gs: dict, stages=SM.ALL, fmt=SM.B10G11R11, **replace):
    from oxylus_amd.renderer import ImageAttachment, SpriteContext

    W, H = f.extent
    n, m, t = f.counts
    tensor = lambda name: gs[name].tensor if name in gs else None  # noqa: E731
    c = SpriteContext(stages, W, H, tuple(float(v) for v in f.pv), gs["sprites"].tensor, n, t, ImageAttachment.depth(gs["depth"].tensor), gs["materials"].tensor.view(-1), m,
                      tensor("vis"), tensor("color"), fmt, f.first_sprite, f.clear)
    return dataclasses.replace(c, **replace)


def outputs(gs, f: Frame, stages, fmt) -> dict:
    W, H = f.extent
    out = dict(depth=gs["depth"].bits()[1].reshape(H, W).view(np.float32).copy())
    if stages & SM.VIS:
        out["vis"] = gs["vis"].bits()[1].reshape(H, W).copy()
    if stages & SM.COLOR:
        out["color"] = gs["color"].bits()[1].reshape((H, W, 4) if fmt else (H, W)).copy()
    return out


def run(r, f: Frame, label, stages=SM.ALL, fmt=SM.B10G11R11, stats=None) -> dict:
    """One oxc_draw_sprites between guard bands: every word of depth, visbuffer_2d and final_attachment equal to the checker's, every input
    unchanged, the bands untouched.  Returns the outputs."""
    import torch

    from gpu_passes import same

    gs = guards(f, stages, fmt)
    r.prepared_frame = prepared_frame(gs, f)
    r.draw_sprites(context(f, gs, stages, fmt))
    torch.cuda.synchronize()
    expected = want(f, stages, fmt, stats)
    for name, g in gs.items():
        g.check(label, expected["vis"] if name == "vis" and f.clear else None)
    got = outputs(gs, f, stages, fmt)
    same(got, expected, label)
    for name in ("sprites", "materials", "transforms"):
        a = getattr(f, name)
        if a.size:
            same(gs[name].bits()[1], np.ascontiguousarray(a).view(gs[name].bits()[1].dtype).reshape(-1), f"{label}: input {name}")
    return got


def run_pick(r, vis: np.ndarray, texels, label):
    """oxc_pick_sprite on each (x, y) between guard bands: the word equals the texel."""
    import torch

    from gpu_passes import Guard
    from oxylus_amd.renderer import SpritePickContext

    H, W = vis.shape
    src = Guard("vis", (H, W), torch.int32, W, POISON32, 4, data=vis)
    out = Guard("transform_id", (1,), torch.int32, 1, POISON32, 4, fill=0x0BADBAD0)
    got = []
    for x, y in texels:
        out.refill()
        r.pick_sprite(SpritePickContext.over(src.tensor, (x, y), out.tensor))
        torch.cuda.synchronize()
        out.check(f"{label} ({x}, {y})")
        src.check(label)
        got.append(int(out.bits()[1][0]))
        assert got[-1] == SM.pick(vis, x, y), f"{label}: texel ({x}, {y}): 0x{got[-1]:X} != 0x{SM.pick(vis, x, y):X}"
    return got


if __name__ == "__main__":
    f = golden_frame()
    stored = {"in_" + name: getattr(f, name) for name in ("sprites", "materials", "transforms", "depth", "color", "pv")}
    for fmt in FORMATS:
        stored[f"in_color_format{fmt}"] = f.color_in(fmt)
        for stages in STAGES:
            for name, image in want(f, stages, fmt).items():
                stored[f"{name}_format{fmt}_stages{stages}"] = image
    np.savez_compressed(GOLDEN, **stored)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
