"""The frames of the highlight tests: hand-made visbuffers over a small record chain, selections, depths and 8-bit colour images, the
checker's calls over them and the GPU calls between guard bands.  The rules come from highlight_model, the guard bands from gpu_passes.
`python tests/highlight_frames.py` writes the golden fixture tests/golden/highlight_17x9.npz: the 17 x 9 frame's inputs, its mask words and
mask image, and the composite in the three formats and three modes."""
import dataclasses
import os
import types

import numpy as np

import highlight_model as HM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "highlight_17x9.npz")
POISON32, POISON16 = 0xFFFFFFFB, 0xFFFB
FILL_DST = 0xFFFFFFFB     # the composite's pre-fill
FILL_ONES = 0xFFFFFFFF    # mask_bits' pre-fill: the zeroed tail bits of a row's last word are seen
FILL_BYTES = 0x7B7B       # the mask image's pre-fill: neither 0 nor 255
TERRAIN_TEXEL = 0xFFFFFE00
TRANSFORMS = np.array([10, 11, 12, 13, HM.EMPTY, 15], np.uint32)   # transform_index of the six mesh instances; one record holds ~0u
TERRAIN_TRANSFORM = 40


@dataclasses.dataclass
class Frame:
    vis: np.ndarray                # uint32 [H, W]
    depth: np.ndarray              # float32 [H, W]
    color: np.ndarray              # uint32 [H, W]
    meshlet_instances: np.ndarray  # uint32 [N, 2]
    mesh_instances: np.ndarray     # uint32 [M, 5]
    meshlet_instance_count: int
    selected: np.ndarray           # uint32 [selected_count]
    terrain_transform_index: int = TERRAIN_TRANSFORM
    color_format: int = HM.RGBA8_SRGB
    outline_color: tuple = HM.OUTLINE
    dilate_radius: int = 8
    outline_width: int = 5
    occluded_mode: int = 2

    @property
    def extent(self):
        return self.vis.shape[1], self.vis.shape[0]

    @property
    def records(self) -> dict:
        return dict(meshlet_instance_count=self.meshlet_instance_count, meshlet_instances=self.meshlet_instances, mesh_instances=self.mesh_instances,
                    terrain_transform_index=self.terrain_transform_index)

    @property
    def settings(self) -> dict:
        return dict(color_format=self.color_format, outline_color=self.outline_color, dilate_radius=self.dilate_radius, outline_width=self.outline_width,
                    occluded_mode=self.occluded_mode)


def record_chain(n=12):
    """n meshlet instances over the six mesh instances of TRANSFORMS, two apiece."""
    m = len(TRANSFORMS)
    mli = np.stack([np.arange(n) % m, np.arange(n) * 3 % 7], axis=-1).astype(np.uint32)
    mi = np.zeros((m, 5), np.uint32)
    mi[:, 0], mi[:, 2], mi[:, 3] = np.arange(m) % 3, np.arange(m) + 20, TRANSFORMS
    return mli, mi


def frame(extent=(17, 9), seed=3, n=12, selected=(11, 13), cell=(5, 3), **settings) -> Frame:
    """Cells of `cell` pixels, each of one meshlet instance, so that the selected transforms form blobs with room between them; ~0u in the
    upper right corner with depth 0 (an outline over it is not occluded), terrain in the lower left corner, depths above 0.00001 elsewhere;
    random colour bytes, three alpha bytes in four 255, the rest 128 or 0."""
    W, H = extent
    rng = np.random.default_rng(seed + 1000 * W + H)
    y, x = np.mgrid[0:H, 0:W]
    cells = rng.integers(0, n, (H // cell[1] + 1, W // cell[0] + 1))
    vis = ((cells[y // cell[1], x // cell[0]].astype(np.uint32) << np.uint32(8)) | rng.integers(0, 64, (H, W)).astype(np.uint32)).astype(np.uint32)
    vis[(x >= W - max(1, W // 4)) & (y < max(1, H // 3))] = HM.EMPTY
    vis[(x < max(1, W // 5)) & (y >= H - max(1, H // 3))] = TERRAIN_TEXEL | 3
    depth = np.where(vis == HM.EMPTY, np.float32(0.0), np.float32(0.2) + np.float32(0.6) * rng.random((H, W)).astype(np.float32)).astype(np.float32)
    alpha = rng.choice(np.array([255, 255, 255, 255, 255, 255, 128, 0], np.uint32), (H, W))
    color = ((rng.integers(0, 1 << 24, (H, W)).astype(np.uint32)) | (alpha << np.uint32(24))).astype(np.uint32)
    mli, mi = record_chain(n)
    return Frame(vis, depth, color, mli, mi, n, np.asarray(selected, np.uint32), **settings)


def golden_frame() -> Frame:
    return frame((17, 9))


def want_mask(f: Frame) -> np.ndarray:
    return HM.selection_mask(f.vis, f.selected, **f.records)


def want_composite(f: Frame, mask=None, stats=None) -> np.ndarray:
    return HM.composite(want_mask(f) if mask is None else mask, f.depth, f.color, stats=stats, **f.settings)


def want_pick(f: Frame, x, y) -> int:
    return HM.pick(f.vis, x, y, **f.records)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------------
def words_per_row(W) -> int:
    return (W + 63) // 64


def guards(f: Frame, stages=HM.ALL, mask_image=True, poisoned_rest=False, mask=None) -> dict:
    """Guarded tensors of what `stages` touch -- with `poisoned_rest` also of every other buffer, holding poison only.  `mask` (bool [H, W])
    fills mask_bits for a composite that runs alone."""
    import torch

    from gpu_passes import Guard

    W, H = f.extent
    n = words_per_row(W)
    gs = {}
    poison = lambda a: np.full(a.shape, POISON32, np.uint32)  # noqa: E731
    reads_mask, reads_composite = bool(stages & HM.MASK), bool(stages & HM.COMPOSITE)
    for name, mine in (("vis", reads_mask), ("meshlet_instances", reads_mask), ("mesh_instances", reads_mask), ("selected", reads_mask and len(f.selected) > 0),
                       ("depth", reads_composite), ("color", reads_composite)):
        a = getattr(f, name)
        if not mine and (not poisoned_rest or a.size == 0):
            continue
        row = W if a.ndim == 2 and name in ("vis", "depth", "color") else (a.shape[1] if a.ndim == 2 else min(a.size, 64))
        gs[name] = Guard(name, a.shape, torch.float32 if a.dtype == np.float32 else torch.int32, row, POISON32, 4, data=a if mine else poison(a))
    if reads_mask:
        gs["mask_bits"] = Guard("mask_bits", (H, 2 * n), torch.int32, 2 * n, POISON32, 8, fill=FILL_ONES)
        if mask_image:
            gs["mask_image"] = Guard("mask_image", ((W * H + 1) // 2,), torch.int16, W, POISON16, 2, fill=FILL_BYTES)
    else:
        words = HM.mask_words(mask).view(np.uint32) if mask is not None else np.full((H, 2 * n), POISON32, np.uint32)
        if mask is not None or poisoned_rest:
            gs["mask_bits"] = Guard("mask_bits", (H, 2 * n), torch.int32, 2 * n, POISON32, 8, data=words)
    if reads_composite:
        gs["dst"] = Guard("dst", (H, W), torch.int32, W, POISON32, 4, fill=FILL_DST)
    elif poisoned_rest:
        gs["dst"] = Guard("dst", (H, W), torch.int32, W, POISON32, 4, data=np.full((H, W), POISON32, np.uint32))
    return gs


def prepared_frame(gs: dict, f: Frame):
    """A PreparedFrame over the guarded record buffers; None when they are not bound."""
    from oxylus_amd.renderer import PreparedFrame

    if "mesh_instances" not in gs:
        return None
    scene = types.SimpleNamespace(n_mesh_instances=len(f.mesh_instances), meshes=None, transforms=None, mesh_instances=gs["mesh_instances"].tensor)
    return PreparedFrame(scene, f.meshlet_instance_count, gs["meshlet_instances"].tensor, None, None, None)


def context(f: Frame, gs: dict, stages=HM.ALL, **replace):
    import torch

    from oxylus_amd.renderer import HighlightContext, ImageAttachment

    W, H = f.extent
    t = lambda name: gs[name].tensor if name in gs else None  # noqa: E731
    image = gs["mask_image"].tensor.view(torch.uint8)[:W * H] if "mask_image" in gs else None
    c = HighlightContext(stages, W, H, t("mask_bits"), visbuffer_attachment=t("vis"), transform_indices=t("selected"),
                         terrain_transform_index=f.terrain_transform_index, meshlet_instance_count=f.meshlet_instance_count, mask_attachment=image,
                         depth_attachment=ImageAttachment.depth(t("depth")) if "depth" in gs else None, color_attachment=t("color"), dst_attachment=t("dst"), **f.settings)
    return dataclasses.replace(c, **replace)


def got_mask_words(gs, f: Frame) -> np.ndarray:
    return gs["mask_bits"].bits()[1].view(np.uint64).reshape(f.extent[1], -1).copy()


def got_mask_image(gs, f: Frame):
    """(the W * H bytes, the bytes of the window behind them)."""
    W, H = f.extent
    b = gs["mask_image"].bits()[1].view(np.uint8)
    return b[:W * H].reshape(H, W).copy(), b[W * H:].copy()


def got_dst(gs, f: Frame) -> np.ndarray:
    return gs["dst"].bits()[1].reshape(f.extent[1], f.extent[0]).copy()


def check_inputs(gs, f: Frame, stages, label):
    from gpu_passes import same

    names = (("vis", "meshlet_instances", "mesh_instances") + (("selected",) if len(f.selected) else ()) if stages & HM.MASK else ()) + (("depth", "color") if stages & HM.COMPOSITE else ())
    for name in names:
        same(gs[name].bits()[1], np.ascontiguousarray(getattr(f, name)).view(np.uint32).reshape(-1), f"{label}: input {name}")


def run(r, f: Frame, label, stages=HM.ALL, mask_image=True, poisoned_rest=False, mask=None, stats=None) -> dict:
    """One oxc_apply_highlight between guard bands: every word of mask_bits, every byte of the mask image and every word of the composite
    equal to the checker's, every input unchanged, the bands untouched.  `mask`: what a composite that runs alone reads.  Returns the
    outputs."""
    import torch

    from gpu_passes import same

    gs = guards(f, stages, mask_image, poisoned_rest, mask)
    r.prepared_frame = prepared_frame(gs, f)
    r.apply_highlight(context(f, gs, stages))
    torch.cuda.synchronize()
    for g in gs.values():
        g.check(label)
    out = {}
    if stages & HM.MASK:
        mask = want_mask(f)
        out["mask_bits"] = got_mask_words(gs, f)
        same(out["mask_bits"], HM.mask_words(mask), f"{label}: mask_bits")
        if mask_image:
            got, rest = got_mask_image(gs, f)
            same(got, HM.mask_image(mask), f"{label}: mask_attachment")
            assert (rest == (FILL_BYTES & 0xFF)).all(), f"{label}: a byte behind the mask image was written"
            out["mask_attachment"] = got
    if stages & HM.COMPOSITE:
        want = want_composite(f, mask, stats)
        gs["dst"].check(label, want)
        out["dst"] = got_dst(gs, f)
        same(out["dst"], want, f"{label}: dst_attachment")
    elif stats is not None:
        want_composite(f, mask, stats)
    check_inputs(gs, f, stages, label)
    return out


def run_pick(r, f: Frame, texels, label):
    """oxc_pick_transform on each (x, y) between guard bands: the word equals the checker's."""
    import torch

    from gpu_passes import Guard
    from oxylus_amd.renderer import PickingContext

    gs = guards(f, HM.MASK, mask_image=False)
    out = Guard("transform_id", (1,), torch.int32, 1, POISON32, 4, fill=0x0BADBAD0)
    r.prepared_frame = prepared_frame(gs, f)
    got = []
    for x, y in texels:
        out.refill()
        r.pick_transform(PickingContext.over(gs["vis"].tensor, (x, y), f.terrain_transform_index, f.meshlet_instance_count, out.tensor))
        torch.cuda.synchronize()
        out.check(f"{label} ({x}, {y})")
        got.append(int(out.bits()[1][0]))
        assert got[-1] == want_pick(f, x, y), f"{label}: texel ({x}, {y}) = 0x{int(f.vis[y, x]):X}: 0x{got[-1]:X} != 0x{want_pick(f, x, y):X}"
    return got


MODES = (0, 1, 2)
FORMATS = (HM.RGBA8_SRGB, HM.BGRA8_SRGB, HM.RGBA8_UNORM)

if __name__ == "__main__":
    f = golden_frame()
    mask = want_mask(f)
    stored = {"in_" + name: getattr(f, name) for name in ("vis", "depth", "color", "meshlet_instances", "mesh_instances", "selected")}
    stored["mask_bits"], stored["mask_attachment"] = HM.mask_words(mask), HM.mask_image(mask)
    for fmt in FORMATS:
        for mode in MODES:
            stored[f"dst_format{fmt}_mode{mode}"] = want_composite(dataclasses.replace(f, color_format=fmt, occluded_mode=mode), mask)
    np.savez_compressed(GOLDEN, **stored)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
