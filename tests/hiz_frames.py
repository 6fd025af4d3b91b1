"""HiZ pyramids off the square: the shapes, layouts, scenes and CPU-side conditions that tests/test_gpu_hiz_shapes.py and
tests/test_gpu_hiz_build_edges.py share ("HiZ shapes").  Nothing here touches a GPU unless it is handed a CUDA tensor."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import oracle
from oxylus_amd import lib as L
from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame
from oxylus_amd.synth import SceneSpec, hiz_layout, make_scene

HIZ_LDS_TEXELS = 384  # kHizLdsTexels (oxcull_kernels.hpp): the floats of the pyramid's top that the meshlet test stages in LDS
POISON = -1.0         # gap value of the reordered layout: below every texel, so a stray tap makes d = -1 and the box visible (fminf drops a NaN)


def level_dims(w: int, h: int, levels: int):
    return [(max(1, w >> k), max(1, h >> k)) for k in range(levels)]


def staged_first(w: int, h: int, levels: int) -> int:
    """The host's staging rule (oxc_cull_geometry, meshlet stage): the longest suffix of levels that fits HIZ_LDS_TEXELS floats;
    returns its first level (== levels: nothing staged, 0: everything)."""
    first, used = levels, 0
    while first > 0:
        mw, mh = max(1, w >> (first - 1)), max(1, h >> (first - 1))
        if used + mw * mh > HIZ_LDS_TEXELS:
            break
        used += mw * mh
        first -= 1
    return first


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
def packed_layout(w: int, h: int, levels: int):
    """The default: ascending, 256-byte aligned (synth.hiz_layout).  -> (byte offsets, total floats)"""
    _, offs, total = hiz_layout(w, h, levels)
    return offs, total // 4


def reordered_layout(w: int, h: int, levels: int):
    """The levels in descending address order (the top level first, level 0 last), a gap of at least w + 64 floats between neighbours and at
    both ends, every offset a multiple of 4 bytes -- and no more than that, except where oxc_generate_hiz asks for more on its tile path
    (level 0 a multiple of 16 bytes, level 1 of 8).  -> (byte offsets, total floats)"""
    offs, off = [0] * levels, 0
    for i, k in enumerate(reversed(range(levels))):
        off += w + 64 + (0, 1, 3, 6, 2, 5, 7)[i % 7]
        if k == 0:
            off = (off + 3) // 4 * 4
        elif k == 1:
            off = (off + 1) // 2 * 2
        elif off % 2 == 0:
            off += 1  # the other levels: odd float offsets, so that nothing but 4-byte alignment can be relied on
        offs[k] = 4 * off
        off += max(1, w >> k) * max(1, h >> k)
    return offs, off + w + 64 + 4


LAYOUTS = {"packed": packed_layout, "reordered": reordered_layout}


def inside_mask(w, h, levels, offs, total):
    m = np.zeros(total, dtype=bool)
    for k, (mw, mh) in enumerate(level_dims(w, h, levels)):
        assert not m[offs[k] // 4: offs[k] // 4 + mw * mh].any(), "levels overlap"
        m[offs[k] // 4: offs[k] // 4 + mw * mh] = True
    return m


@dataclasses.dataclass
class Pyramid:
    """One pyramid on the CPU: `data` holds the checker's levels at `offs`, POISON everywhere else."""
    w: int
    h: int
    levels: int
    offs: list
    data: torch.Tensor

    @property
    def hizd(self):
        return {"data": self.data, "w": self.w, "h": self.h, "levels": self.levels, "offs": self.offs}

    def struct(self):
        return oracle.make_hiz(self.data, self.w, self.h, self.levels, self.offs)

    def attachment(self, device="cuda") -> ImageAttachment:
        return ImageAttachment(self.data.to(device), self.w, self.h, self.levels, list(self.offs))

    def level(self, k):
        mw, mh = level_dims(self.w, self.h, self.levels)[k]
        return self.data[self.offs[k] // 4: self.offs[k] // 4 + mw * mh].view(mh, mw)

    def relaid(self, layout: str) -> "Pyramid":
        offs, total = LAYOUTS[layout](self.w, self.h, self.levels)
        out = Pyramid(self.w, self.h, self.levels, offs, torch.full((total,), POISON, dtype=torch.float32))
        for k in range(self.levels):
            out.level(k).copy_(self.level(k))
        return out


def oracle_pyramid(depth_cpu: torch.Tensor, w: int, h: int, levels: int, layout: str = "packed") -> Pyramid:
    offs, total = LAYOUTS[layout](w, h, levels)
    data = torch.full((total,), POISON, dtype=torch.float32)
    oracle.generate_hiz(depth_cpu, data, w, h, levels, offs)
    return Pyramid(w, h, levels, offs, data)


def cell_depth(dw: int, dh: int, seed: int, cell: int, far_frac: float = 0.3, near: float = 0.1, dist=(1.0, 40.0)) -> torch.Tensor:
    """Reversed-Z depth in square cells of `cell` texels: far (0) with probability far_frac, else an occluder at a distance drawn
    log-uniformly from `dist`."""
    g = torch.Generator().manual_seed(seed)
    ch, cw = -(-dh // cell), -(-dw // cell)
    d = dist[0] * torch.exp(torch.rand((ch, cw), generator=g) * float(np.log(dist[1] / dist[0])))
    z = torch.where(torch.rand((ch, cw), generator=g) < far_frac, torch.zeros(()), near / d)
    return z.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[:dh, :dw].contiguous()


# ---- what test_occlusion does with one box, restated in numpy binary32 (cull.slang:86-135) -----------------------------------------------
_F = np.float32


def _sat_u32(x) -> int:
    return 0 if not x > 0 else min(int(x), 0xFFFFFFFF)


def _sat_i32(x) -> int:
    return 0 if x != x else max(-2**31, min(int(x), 2**31 - 1))


def occlusion_taps(sa, w: int, h: int, levels: int) -> dict:
    sw, sh = _F(w), _F(h)
    minx, miny = _sat_u32(np.fmax(_F(sa[0]) * sw, _F(0))), _sat_u32(np.fmax(_F(sa[1]) * sh, _F(0)))
    maxx, maxy = _sat_u32(np.fmin(_F(sa[3]) * sw, sw - _F(1))), _sat_u32(np.fmin(_F(sa[4]) * sh, sh - _F(1)))
    ms = max((maxx - minx) & 0xFFFFFFFF, (maxy - miny) & 0xFFFFFFFF)
    raw = 0 if ms <= 1 else (ms - 1).bit_length()
    mip = min(raw, levels - 1)
    uc, vc = (_F(minx) + _F(maxx)) * _F(0.5), (_F(miny) + _F(maxy)) * _F(0.5)
    u, v = uc / sw, vc / sh
    mw, mh = max(1, w >> mip), max(1, h >> mip)
    bx, by = _sat_i32(np.floor(u * _F(mw) - _F(0.5))), _sat_i32(np.floor(v * _F(mh) - _F(0.5)))
    clamp = lambda t, hi: min(max(t, 0), hi)  # noqa: E731
    edges = ("L" if bx < 0 else "") + ("R" if bx + 1 > mw - 1 else "") + ("T" if by < 0 else "") + ("B" if by + 1 > mh - 1 else "")
    return {"raw": raw, "mip": mip, "uc": uc, "vc": vc, "u": u, "v": v, "x": (clamp(bx, mw - 1), clamp(bx + 1, mw - 1)),
            "y": (clamp(by, mh - 1), clamp(by + 1, mh - 1)), "edges": edges}


def candidates(scene_cpu):
    """The screen boxes test_occlusion sees: (meshlet instance index, project_aabb's six floats) of every meshlet that passes the camera
    tests and projects (cull_meshlets_hiz.slang:61-65), and the number of camera-test survivors."""
    assert scene_cpu.spec.lod_count == 1 and scene_cpu.spec.share_meshes == 0  # bounds row == meshlet instance index
    cam = scene_cpu.cull_camera()
    survivors = oracle.cull_meshlets(scene_cpu, cam, scene_cpu.meshlet_instances).tolist()
    bounds = oracle.decode_bounds(scene_cpu.bounds.numpy())
    pv, tr, K = np.float32(scene_cpu.camera["projection_view"]), scene_cpu.transforms.numpy(), scene_cpu.spec.meshlets_per_mesh
    mvps, out = {}, []
    for i in survivors:
        mi = i // K
        if mi not in mvps:
            mvps[mi] = oracle.mul_mat4(pv, tr[mi])
        sa = oracle.project_aabb(mvps[mi], scene_cpu.camera["near_clip"], bounds[i, 0:3], bounds[i, 3:6])
        if sa is not None:
            out.append((i, sa))
    return out, len(survivors)


def exercise_report(scene_cpu, pyr: Pyramid) -> dict:
    """How a scene exercises a pyramid, from the checker alone: the levels chosen, whether a raw mip exceeds the top, the edges at which a
    tap clamps, and the share of the camera-test survivors that occlusion removes."""
    cand, n_survivors = candidates(scene_cpu)
    hz = pyr.struct()
    chosen, edges, exceeds, occluded = set(), set(), False, 0
    for _, sa in cand:
        t = occlusion_taps(sa, pyr.w, pyr.h, pyr.levels)
        assert t["mip"] == oracle.occlusion_mip(sa, hz)
        chosen.add(t["mip"])
        edges.update(t["edges"])
        exceeds |= t["raw"] > pyr.levels - 1
        occluded += oracle.test_occlusion(sa, hz)
    n = scene_cpu.n_meshlet_instances
    mask = torch.zeros((n + 31) // 32, dtype=torch.int32)
    kept = oracle.cull_meshlets_hiz(scene_cpu, scene_cpu.cull_camera(), scene_cpu.meshlet_instances, L.CULL_TEST_ALL | L.CULL_LATE_PASS, hz,
                                    oracle.Visibility(n, 0, 0), mask, torch.zeros(max(n, 1), dtype=torch.int32))
    assert n_survivors - kept == occluded, "the boxes derived here are not the ones the checker's meshlet test sees"
    return {"levels": chosen, "edges": edges, "exceeds": exceeds, "occluded": occluded / max(n_survivors, 1), "candidates": len(cand)}


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------
MIP0_EDGES = ("one level: every box samples mip 0, where u <= 1 - 1/w puts the left tap column at w - 2 at most, so the right (and likewise the bottom) "
              "clamp cannot act; the left and top clamps do")
NO_EXCEED = ("a box spans at most max(w, h) - 1 texels and ceil(log2) of that is the top level of a full chain whose longer side is a power of two "
             "(min > max, the u32 wrap, needs a box wholly off screen, which the frustum test removes)")


@dataclasses.dataclass(frozen=True)
class Shape:
    w: int
    h: int
    levels: int            # 0: the full count
    purpose: str
    all_modes: bool = False
    seed: int = 1
    meshlets: int = 65
    dropped: tuple = ()    # ((condition, why it cannot hold at this shape), ...)

    @property
    def n_levels(self):
        return self.levels or hiz_layout(self.w, self.h)[0]

    @property
    def id(self):
        return f"{self.w}x{self.h}" + (f"-levels{self.levels}" if self.levels else "")


SHAPES = [
    Shape(128, 64, 0, "the 720p class", all_modes=True, dropped=(("exceeds", NO_EXCEED),)),
    Shape(64, 128, 0, "its transpose", meshlets=130, dropped=(("exceeds", NO_EXCEED),)),
    Shape(256, 64, 0, "4:1, upper levels N x 1", dropped=(("exceeds", NO_EXCEED),)),
    Shape(16, 64, 0, "1:4, upper levels 1 x N", meshlets=130, dropped=(("exceeds", NO_EXCEED),)),
    Shape(96, 40, 0, "neither side a power of two", all_modes=True, seed=4),
    Shape(100, 36, 0, "neither side a power of two", meshlets=130),
    Shape(3, 5, 0, "neither side a power of two", seed=13, dropped=(("exceeds", "a box spans at most 4 texels: raw mip 2, the top of the three levels"),)),
    Shape(64, 40, 0, "width a power of two, height not", all_modes=True, meshlets=130, dropped=(("exceeds", NO_EXCEED),)),
    Shape(40, 64, 0, "height a power of two, width not", seed=2, dropped=(("exceeds", NO_EXCEED),)),
    Shape(16, 16, 0, "everything staged", all_modes=True, dropped=(("exceeds", NO_EXCEED),)),
    Shape(8, 8, 0, "everything staged", meshlets=130, dropped=(("exceeds", NO_EXCEED),)),
    Shape(2, 2, 0, "everything staged", dropped=(
        ("exceeds", NO_EXCEED), ("levels", "a box spans at most 1 texel: mip 0 always, level 1 is never chosen"),
        ("edges", "mip 0 only, u in {0, 1/4, 1/2}: the left tap column is -1, 0 or 0 and the right one never passes column 1; likewise in y"))),
    Shape(1, 1, 0, "everything staged", dropped=(
        ("exceeds", NO_EXCEED), ("edges", "u = v = 0 always: the taps are columns -1 and 0, so only the left and top clamps can act"))),
    Shape(24, 16, 1, "384 texels: the staging budget met exactly", all_modes=True, dropped=(("edges", MIP0_EDGES),)),
    Shape(25, 16, 1, "400 texels: the budget just missed", all_modes=True, dropped=(("edges", MIP0_EDGES),)),
    Shape(128, 64, 1, "short level count: every mip clamps to level 0", dropped=(("edges", MIP0_EDGES),)),
    Shape(128, 64, 3, "short level count", meshlets=130),
]
SHAPE_BY_ID = {s.id: s for s in SHAPES}
# what the right-hand column of the table says about staging: shape id -> first staged level
STAGING = {"128x64": 3, "64x128": 3, "256x64": 3, "16x64": 1, "96x40": 2, "100x36": 2, "3x5": 0, "64x40": 2, "40x64": 2, "16x16": 0, "8x8": 0, "2x2": 0,
           "1x1": 0, "24x16-levels1": 0, "25x16-levels1": 1, "128x64-levels1": 1, "128x64-levels3": 3}


@functools.lru_cache(maxsize=None)
def shape_frame(shape_id: str):
    """The scene, depth, pyramid (packed) and prior mask of one shape -- built once, shared by every test of the shape, never written."""
    s = SHAPE_BY_ID[shape_id]
    scene = make_scene(SceneSpec(n_mesh_instances=40, meshlets_per_mesh=s.meshlets, seed=7100 + s.seed), "cpu")
    # the instances at distances drawn log-uniformly from 0.8 .. 40 m and out to the frustum's sides: boxes from under a texel to most of the
    # screen (every level, the top one included) and boxes against all four edges
    g = torch.Generator().manual_seed(100 + s.seed)
    dist = 0.8 * torch.exp(torch.rand(40, generator=g) * float(np.log(40.0 / 0.8)))
    scene.transforms[:, 12] = (torch.rand(40, generator=g) * 2 - 1) * 0.6 * dist
    scene.transforms[:, 13] = (torch.rand(40, generator=g) * 2 - 1) * 0.6 * dist
    scene.transforms[:, 14] = -dist
    depth = cell_depth(2 * s.w + 1, 2 * s.h + 1, seed=s.seed, cell=max(2, min(s.w, s.h) // 4))
    pyr = oracle_pyramid(depth, s.w, s.h, s.n_levels)
    g = torch.Generator().manual_seed(s.seed)
    words = (scene.n_meshlet_instances + 31) // 32
    mask = ((torch.rand((words, 32), generator=g) < 0.3).to(torch.int64) << torch.arange(32)).sum(1).to(torch.int32)
    return scene, depth, pyr, mask


@functools.lru_cache(maxsize=None)
def shape_report(shape_id: str) -> dict:
    scene, _, pyr, _ = shape_frame(shape_id)
    return exercise_report(scene, pyr)


def assert_exercised(shape: Shape, report: dict):
    """The four conditions a scene has to meet at a shape, less those the shape states it cannot."""
    dropped = dict(shape.dropped)
    if "levels" not in dropped:
        assert report["levels"] == set(range(shape.n_levels)), f"{shape.id}: levels chosen {sorted(report['levels'])} of {shape.n_levels}"
    if "exceeds" not in dropped:
        assert report["exceeds"], f"{shape.id}: no candidate's raw mip exceeds the top level"
    if "edges" not in dropped:
        assert report["edges"] == set("LRTB"), f"{shape.id}: taps clamp only at {sorted(report['edges'])}"
    assert 0.05 <= report["occluded"] <= 0.95, f"{shape.id}: occlusion removes {report['occluded']:.1%} of the camera-test survivors"


# ---- the two-element batch form ------------------------------------------------------------------------------------------------------------
def gpu_batch_two_pass(renderer, scenes_gpu, att: ImageAttachment, masks):
    """A two-pass HiZ frame of every scene through oxc_cull_geometry_batch (one early call, one late call); per scene a dict in the layout of
    util.gpu_frame."""
    frames, ctxs = [], []
    for sc, m in zip(scenes_gpu, masks):
        fr = PreparedFrame.create(sc, with_triangles=True, expand=True)
        fr.meshlet_instance_visibility_mask_buffer.copy_(m.to(sc.device))
        cx = CullGeometryContext(use_hiz=True, init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=sc.cull_camera(), hiz_attachment=att, stages=L.STAGE_ALL)
        renderer.prepared_frame = fr
        renderer.seed_meshlet_instances(cx, sc.n_meshlet_instances)
        frames.append(fr)
        ctxs.append(cx)
    out = [{} for _ in scenes_gpu]
    for tag, flags in (("early", L.CULL_TEST_ALL), ("late", L.CULL_TEST_ALL | L.CULL_LATE_PASS)):
        for cx in ctxs:
            cx.cull_flags = flags
        renderer.cull_geometry_batch(frames, ctxs)
        for res, fr, cx in zip(out, frames, ctxs):
            c = renderer.read_counters(cx)
            first = c.early_visible_meshlet_instances if tag == "late" else 0
            res[f"{tag}_emitted"] = c.cull_triangles_cmd_x
            res[f"{tag}_visible"] = fr.visible_meshlet_instances_indices_buffer[first:first + c.cull_triangles_cmd_x].cpu().numpy().copy()
            res[f"{tag}_indices"] = fr.reordered_indices_buffer[:c.draw_index_count].cpu().numpy().copy()
            res["total"], res["early"], res["late"] = c.total_visible_meshlet_instances, c.early_visible_meshlet_instances, c.late_visible_meshlet_instances
    for res, fr in zip(out, frames):
        res["mask"] = fr.meshlet_instance_visibility_mask_buffer.cpu().numpy().copy()
    return out
