"""The terrain patch cull (oxc_cull_terrain) off its one tested shape: the helpers tests/test_terrain.py had, the kernel's box rule restated in
numpy binary32, the CPU-side conditions a terrain has to meet at each HiZ shape of hiz_frames.SHAPES, and one guarded call through the ctypes
context ("Terrain cull shapes pinned by the tests").  Nothing here touches a GPU but `run` and `guarded`."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import torch

import oracle
from hiz_frames import SHAPE_BY_ID, Pyramid, Shape, cell_depth, occlusion_taps, oracle_pyramid
from oxylus_amd import lib as L
from oxylus_amd.lib import CullCamera
from oxylus_amd.renderer import ImageAttachment
from oxylus_amd.synth import perspective_reversed_z

_F = np.float32
FRUSTUM, OCCLUSION, LATE = L.CULL_TEST_FRUSTUM, L.CULL_TEST_OCCLUSION, L.CULL_LATE_PASS
PASSES = (L.CULL_TEST_ALL, L.CULL_TEST_ALL | L.CULL_LATE_PASS)


# ---- what tests/test_terrain.py had ----------------------------------------------------------------------------------------------------------
def _camera(eye=(0.0, 40.0, 0.0), near=0.1, far=2000.0):
    """Camera at `eye` looking down -Z (view = translate(-eye)); reversed-Z projection as everywhere else."""
    proj = perspective_reversed_z(60.0, 1.0, near, far).view(4, 4)  # [col][row]
    view = torch.eye(4)
    view[3, 0:3] = -torch.tensor(eye)  # column 3 = translation
    pv = (proj.t() @ view.t()).t().contiguous()  # column-major product proj * view
    cam = CullCamera()
    for i, v in enumerate(pv.flatten().tolist()):
        cam.projection_view[i] = v
    for i in range(3):
        cam.position[i] = eye[i]
    cam.near_clip = near
    cam.resolution[0] = cam.resolution[1] = 1024.0
    cam.acceptable_lod_error = 2.0
    return cam


def _terrain(pcx, pcy, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand((pcy, pcx), generator=g) * 0.6
    hi = lo + torch.rand((pcy, pcx), generator=g) * 0.4
    flat = torch.rand((pcy, pcx), generator=g) < 0.1
    hi = torch.where(flat, lo, hi)  # flat patches: extent.y falls back to 1e-3
    return torch.stack([lo, hi], -1).contiguous()


def _mask(total, seed, p):
    g = torch.Generator().manual_seed(seed)
    words = (total + 31) // 32
    bits = (torch.rand((words, 32), generator=g) < p).to(torch.int64)
    return (bits << torch.arange(32)).sum(1).to(torch.int32)


def random_words(total, seed):
    """A mask random in all 32 bits of every word, the bits past `total` included."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2**31, 2**31, ((total + 31) // 32,), generator=g, dtype=torch.int64).to(torch.int32)


# ---- one terrain -----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class World:
    """The GPU::TerrainData fields the cull reads.  The default rectangle is the one of tests/test_terrain.py."""
    grid: tuple                      # (patch_count.x, patch_count.y)
    wmin: tuple = (-300.0, -700.0)   # (x, z)
    wsize: tuple = (600.0, 650.0)
    base_h: float = -5.0
    hscale: float = 60.0

    @property
    def total(self):
        return self.grid[0] * self.grid[1]


def checker(world: World, mm: torch.Tensor, cam, flags: int, hz, mask: torch.Tensor) -> torch.Tensor:
    """oracle.cull_terrain on `world`: the emitted list; `mask` (int32 words) is updated in place."""
    return oracle.cull_terrain(list(world.wmin), list(world.wsize), world.grid, world.base_h, world.hscale, mm, cam, flags, hz, mask)


def patch_boxes(world: World, mm):
    """(centre [n, 3], extent [n, 3]) of every patch in binary32: the operations of oxcull_terrain.hip:50-59 and of orc_cull_terrain in their
    order (patch_corner, scene.slang:648-652; centre and extent, terrain_cull.slang:29-38), one rounding per operation, no contraction."""
    pcx, pcy = world.grid
    idx = np.arange(pcx * pcy, dtype=np.uint32)
    px, py = idx % np.uint32(pcx), idx // np.uint32(pcx)
    w0, w1, s0, s1 = _F(world.wmin[0]), _F(world.wmin[1]), _F(world.wsize[0]), _F(world.wsize[1])
    with np.errstate(all="ignore"):
        g0x, g0y = px.astype(_F) / _F(pcx), py.astype(_F) / _F(pcy)
        g1x, g1y = (px + np.uint32(1)).astype(_F) / _F(pcx), (py + np.uint32(1)).astype(_F) / _F(pcy)
        cminx, cminy = w0 + g0x * s0, w1 + g0y * s1
        cmaxx, cmaxy = w0 + g1x * s0, w1 + g1y * s1
        b = np.asarray(mm, dtype=_F).reshape(-1, 2)
        bx, by = b[:, 0], b[:, 1]
        cx, cy, cz = (cminx + cmaxx) * _F(0.5), _F(world.base_h) + ((bx + by) * _F(0.5)) * _F(world.hscale), (cminy + cmaxy) * _F(0.5)
        hy = _F(world.hscale) * (by - bx)
        ex, ey, ez = cmaxx - cminx, np.where(hy > _F(1e-3), hy, _F(1e-3)).astype(_F), cmaxy - cminy  # (a NaN hy compares false: 1e-3)
    return np.stack([cx, cy, cz], 1).astype(_F), np.stack([ex, ey, ez], 1).astype(_F)


def behind_camera(cam, centre, extent):
    """Per patch: every corner of the box has clip w <= 0 (the camera looks the other way)."""
    pv = np.array(list(cam.projection_view), dtype=np.float64).reshape(4, 4)  # [col][row]
    out = np.ones(len(centre), dtype=bool)
    for sx in (-0.5, 0.5):
        for sy in (-0.5, 0.5):
            for sz in (-0.5, 0.5):
                p = centre.astype(np.float64) + extent.astype(np.float64) * np.array([sx, sy, sz])
                w = p[:, 0] * pv[0, 3] + p[:, 1] * pv[1, 3] + p[:, 2] * pv[2, 3] + pv[3, 3]
                out &= w <= 0
    return out


def screen_boxes(world: World, mm, cam, frustum=True):
    """-> ([(patch index, project_aabb's six floats or None)] of every patch that passes test_frustum (every patch with frustum = False),
    in ascending order."""
    centre, extent = patch_boxes(world, mm)
    pv = np.array(list(cam.projection_view), dtype=_F)
    out = []
    for i in range(world.total):
        if frustum and not oracle.test_frustum(pv, centre[i], extent[i]):
            continue
        out.append((i, oracle.project_aabb(pv, cam.near_clip, centre[i], extent[i])))
    return out


def exercise_report(world: World, mm, cam, pyr: Pyramid) -> dict:
    """How a terrain exercises a pyramid, from the checker alone (the form of hiz_frames.exercise_report): the levels chosen, whether a raw
    mip exceeds the top, the edges at which a tap clamps, and the share of the frustum survivors that occlusion removes."""
    boxes = screen_boxes(world, mm, cam)
    hz = pyr.struct()
    chosen, edges, exceeds, occluded, none = set(), set(), False, 0, 0
    for _, sa in boxes:
        if sa is None:
            none += 1
            continue
        t = occlusion_taps(sa, pyr.w, pyr.h, pyr.levels)
        assert t["mip"] == oracle.occlusion_mip(sa, hz)
        chosen.add(t["mip"])
        edges.update(t["edges"])
        exceeds |= t["raw"] > pyr.levels - 1
        occluded += oracle.test_occlusion(sa, hz)
    words = (world.total + 31) // 32
    count = lambda flags, fill: checker(world, mm, cam, flags, hz, torch.full((words,), fill, dtype=torch.int32)).numel()  # noqa: E731
    # LatePass alone already asks for the occlusion test (HAS_FLAG(a | b) is "any of", terrain_cull.slang:52), so FRUSTUM | LATE and
    # FRUSTUM | OCCLUSION | LATE keep the same patches; the frustum survivors themselves are what FRUSTUM alone emits of a full mask
    assert count(FRUSTUM | LATE, 0) == count(FRUSTUM | OCCLUSION | LATE, 0)
    survivors = count(FRUSTUM, -1)
    assert survivors == len(boxes), "test_frustum on the boxes derived here keeps other patches than the checker's terrain cull"
    assert survivors - count(FRUSTUM | OCCLUSION | LATE, 0) == occluded, "the boxes derived here are not the ones the checker's terrain cull sees"
    return {"levels": chosen, "edges": edges, "exceeds": exceeds, "occluded": occluded / max(survivors, 1), "survivors": survivors, "none": none,
            "removed": occluded}


# ---- one terrain per HiZ shape ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Placement:
    """Where the terrain and the camera of a shape are, and how far its occluders."""
    eye: tuple = (0.0, 25.0, 0.0)      # inside the terrain's height range (-5 .. 55): boxes against the top edge as well as the bottom one
    wmin: tuple = (-304.6875, -700.0)  # half a patch to the left: one column of patches is centred under the camera, so its nearest box
    wsize: tuple = (600.0, 698.0)      # (the rows reach up to z = -2) spans the whole screen -- the top level, and a raw mip past it
    grid: tuple = (64, 64)
    dist: tuple = (30.0, 800.0)
    seed: int = 1
    dropped: tuple = ()              # ((condition, why), ...) on top of what the shape itself drops


# the default serves every shape but these (tests/test_terrain_cull_frames.py holds each to its conditions)
PLACEMENTS: dict = {
    "256x64": Placement(seed=2),
    "3x5": Placement(eye=(0.0, 15.0, 0.0), seed=2),
    "8x8": Placement(seed=2),
    # three levels: a tap clamps at the top or bottom only for a box within three texels of that edge; half-size patches put enough of them there
    "128x64-levels3": Placement(eye=(0.0, 16.0, 0.0), wmin=(-152.34375, -352.0), wsize=(300.0, 350.0)),
}


def placement(shape_id: str) -> Placement:
    return PLACEMENTS.get(shape_id, Placement())


def dropped_conditions(shape_id: str) -> dict:
    return {**dict(SHAPE_BY_ID[shape_id].dropped), **dict(placement(shape_id).dropped)}


@functools.lru_cache(maxsize=None)
def shape_frame(shape_id: str):
    """(world, min / max image, camera, pyramid (packed), prior mask) of one shape -- built once, shared by every test of it, never written."""
    s, p = SHAPE_BY_ID[shape_id], placement(shape_id)
    world = World(p.grid, p.wmin, p.wsize)
    depth = cell_depth(2 * s.w + 1, 2 * s.h + 1, seed=p.seed, cell=max(2, min(s.w, s.h) // 4), dist=p.dist)
    return world, _terrain(p.grid[0], p.grid[1], 300 + p.seed), _camera(eye=p.eye), oracle_pyramid(depth, s.w, s.h, s.n_levels), _mask(world.total, 7 + p.seed, 0.35)


@functools.lru_cache(maxsize=None)
def shape_report(shape_id: str) -> dict:
    world, mm, cam, pyr, _ = shape_frame(shape_id)
    return exercise_report(world, mm, cam, pyr)


@functools.lru_cache(maxsize=None)
def shape_want(shape_id: str):
    """The checker's early and late pass of a shape's frame: ([list, list], [mask after early, mask after late])."""
    world, mm, cam, pyr, mask = shape_frame(shape_id)
    m, lists, masks = mask.clone(), [], []
    for flags in PASSES:
        lists.append(checker(world, mm, cam, flags, pyr.struct(), m))
        masks.append(m.clone())
    return lists, masks


def assert_exercised(shape: Shape, report: dict):
    """hiz_frames.assert_exercised with the terrain's own dropped conditions next to the shape's."""
    dropped = dropped_conditions(shape.id)
    if "levels" not in dropped:
        assert report["levels"] == set(range(shape.n_levels)), f"{shape.id}: levels chosen {sorted(report['levels'])} of {shape.n_levels}"
    if "exceeds" not in dropped:
        assert report["exceeds"], f"{shape.id}: no box's raw mip exceeds the top level"
    if "edges" not in dropped:
        assert report["edges"] == set("LRTB"), f"{shape.id}: taps clamp only at {sorted(report['edges'])}"
    assert 0.05 <= report["occluded"] <= 0.95, f"{shape.id}: occlusion removes {report['occluded']:.1%} of the frustum survivors"


# ---- the call --------------------------------------------------------------------------------------------------------------------------------
GUARD_WORDS = 2
MASK_GUARD = 0x5EA1C0DE
VISIBLE_FILL = -0x21524111  # 0xDEADBEEF: no patch index (at most 2^24) looks like it


def guarded(words: torch.Tensor, device="cuda") -> torch.Tensor:
    """`words` (int32) with two guard words in front and two behind."""
    g = torch.full((GUARD_WORDS,), MASK_GUARD, dtype=torch.int32)
    return torch.cat([g, words.to(torch.int32).cpu(), g]).to(device)


def mask_words(alloc: torch.Tensor) -> torch.Tensor:
    return alloc[GUARD_WORDS:alloc.numel() - GUARD_WORDS]


def guards_intact(alloc: torch.Tensor) -> bool:
    a = alloc.cpu()
    return bool((a[:GUARD_WORDS] == MASK_GUARD).all() and (a[-GUARD_WORDS:] == MASK_GUARD).all())


def visible_allocation(total: int, device="cuda") -> torch.Tensor:
    return torch.full((total + 2 * GUARD_WORDS,), VISIBLE_FILL, dtype=torch.int32, device=device)


def hiz_image(hiz):
    """-> (L.Image, what has to stay alive): from a Pyramid, an ImageAttachment, an L.Image or None."""
    if hiz is None or isinstance(hiz, L.Image):
        return hiz, None
    att = hiz.attachment("cuda") if isinstance(hiz, Pyramid) else hiz
    assert isinstance(att, ImageAttachment)
    return att.c(), att


def terrain_context(flags: int, cam, world: World, mm: torch.Tensor, mask_alloc: torch.Tensor, visible_alloc: torch.Tensor, hiz=None):
    """The ctypes context of one call: the mask buffer is exactly ceil(total / 32) words and the visible buffer exactly `total` words, each
    between the guard words of its allocation.  -> (context, what has to stay alive)"""
    pcx, pcy = world.grid
    c = L.TerrainContext()
    c.struct_size = C.sizeof(L.TerrainContext)
    c.cull_flags = flags
    c.cull_camera = cam
    c.world_min[0], c.world_min[1] = world.wmin
    c.world_size[0], c.world_size[1] = world.wsize
    c.patch_count[0], c.patch_count[1] = pcx, pcy
    c.base_height, c.height_scale = world.base_h, world.hscale
    im = L.Image()
    im.dptr, im.width, im.height, im.levels = mm.data_ptr(), pcx, pcy, 1
    c.patch_minmax_attachment = im
    image, keep = hiz_image(hiz)
    if image is not None:
        c.hiz_attachment = image
    c.visible_patches_buffer = L.Buffer(C.c_void_p(visible_alloc.data_ptr() + 4 * GUARD_WORDS), 4 * world.total)
    c.patch_visibility_mask_buffer = L.Buffer(C.c_void_p(mask_alloc.data_ptr() + 4 * GUARD_WORDS), 4 * ((world.total + 31) // 32))
    return c, (mm, mask_alloc, visible_alloc, keep)


def read_cmd(renderer, dptr, stream=None):
    host = (C.c_uint32 * 4)()
    renderer._check(renderer._lib.oxc_debug_read_u32(renderer._ctx, dptr, 4, C.cast(host, C.c_void_p), renderer._stream(stream)))
    return list(host)


def run(renderer, flags: int, cam, world: World, mm: torch.Tensor, mask_alloc: torch.Tensor, hiz=None, visible_alloc: torch.Tensor = None, stream=None,
        tweak=None, out: dict = None):
    """One oxc_cull_terrain through the ctypes context itself (Renderer.cull_terrain hands back the list's prefix only).  `mask_alloc` comes
    from `guarded`; `tweak(context)` may spoil the context before the call; `out`, a dict, receives the context (its draw_cmd_buffer).
    -> (emitted list, draw command, the whole mask allocation, the whole visible allocation), all on the CPU."""
    assert mask_alloc.numel() == (world.total + 31) // 32 + 2 * GUARD_WORDS and mm.is_cuda and mm.is_contiguous()
    if visible_alloc is None:
        visible_alloc = visible_allocation(world.total)
    c, keep = terrain_context(flags, cam, world, mm, mask_alloc, visible_alloc, hiz)
    if tweak is not None:
        tweak(c)
    renderer._keep = keep
    renderer._check(renderer._lib.oxc_cull_terrain(renderer._ctx, C.byref(c), renderer._stream(stream)))
    if out is not None:
        out["context"] = c
    cmd = read_cmd(renderer, c.draw_cmd_buffer.dptr, stream)
    vis = visible_alloc.cpu()
    return vis[GUARD_WORDS:GUARD_WORDS + min(cmd[1], world.total)].clone(), cmd, mask_alloc.cpu(), vis


def assert_call(got, want_list: torch.Tensor, want_mask: torch.Tensor, what=""):
    """The four comparisons of one call: the list, the command, every mask word with its guards, the visible buffer beyond the count with its
    guards."""
    lst, cmd, mask_alloc, vis_alloc = got
    n = want_list.numel()
    assert cmd == [4, n, 0, 0], f"{what}: draw_cmd {cmd}, the checker emits {n}"
    assert torch.equal(lst, want_list), f"{what}: {int((lst != want_list).sum())} of {n} emitted patches differ"
    assert guards_intact(mask_alloc), f"{what}: a guard word of the mask was written"
    assert torch.equal(mask_words(mask_alloc), want_mask), f"{what}: mask words {torch.nonzero(mask_words(mask_alloc) != want_mask).flatten().tolist()[:8]} differ"
    rest = torch.cat([vis_alloc[:GUARD_WORDS], vis_alloc[GUARD_WORDS + n:]])
    assert bool((rest == VISIBLE_FILL).all()), f"{what}: the visible buffer was written beyond the {n} emitted patches"


def enqueue(renderer, flags: int, cam, world: World, mm: torch.Tensor, mask_alloc: torch.Tensor, hiz=None, stream=None):
    """`run` without the readback (nothing here synchronises): -> (context, visible allocation), for `collect`."""
    visible_alloc = visible_allocation(world.total)
    c, keep = terrain_context(flags, cam, world, mm, mask_alloc, visible_alloc, hiz)
    renderer._kept_terrain = getattr(renderer, "_kept_terrain", [])[-7:] + [keep]  # (several calls may be in flight)
    renderer._check(renderer._lib.oxc_cull_terrain(renderer._ctx, C.byref(c), renderer._stream(stream)))
    return c, visible_alloc


def collect(renderer, c, world: World, mask_alloc: torch.Tensor, visible_alloc: torch.Tensor, stream=None):
    cmd = read_cmd(renderer, c.draw_cmd_buffer.dptr, stream)
    vis = visible_alloc.cpu()
    return vis[GUARD_WORDS:GUARD_WORDS + min(cmd[1], world.total)].clone(), cmd, mask_alloc.cpu(), vis


# ---- the fixtures of tests/test_gpu_terrain_cull.py ------------------------------------------------------------------------------------------
SEAM_GRIDS = [(1, 1), (31, 1), (1, 31), (32, 1), (1, 32), (8, 4), (33, 1), (1, 33), (11, 3), (63, 1), (1, 63), (9, 7), (64, 1), (1, 64), (8, 8), (65, 1), (1, 65),
              (13, 5), (1023, 1), (1, 1023), (33, 31), (1024, 1), (1, 1024), (32, 32), (1025, 1), (1, 1025), (41, 25), (1088, 1), (1, 1088), (17, 64), (2048, 1),
              (1, 2048), (64, 32), (2049, 1), (1, 2049), (683, 3)]
SEAM_TOTALS = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1088, 2048, 2049)


@functools.lru_cache(maxsize=None)
def small_pyramid(w=48, h=20, seed=5, dist=(30.0, 800.0)) -> Pyramid:
    """The pyramid of the tests that are not about the pyramid: small, non-square, no side a power of two, the full chain."""
    from oxylus_amd.synth import hiz_layout

    return oracle_pyramid(cell_depth(2 * w + 1, 2 * h + 1, seed=seed, cell=max(2, min(w, h) // 4), dist=dist), w, h, hiz_layout(w, h)[0])


@functools.lru_cache(maxsize=None)
def two_pass_want(world: World, seed: int, mask_seed: int, random_mask: bool, eye=(0.0, 40.0, 0.0)):
    """(min / max image, prior mask, [early list, late list], [mask after early, mask after late]) of `world` under small_pyramid()."""
    mm = _terrain(world.grid[0], world.grid[1], seed)
    mask = random_words(world.total, mask_seed) if random_mask else _mask(world.total, mask_seed, 0.35)
    m, lists, masks, hz = mask.clone(), [], [], small_pyramid().struct()
    for flags in PASSES:
        lists.append(checker(world, mm, _camera(eye=eye), flags, hz, m))
        masks.append(m.clone())
    return mm, mask, lists, masks


FLAG_SETS = [0, FRUSTUM, OCCLUSION, LATE, FRUSTUM | OCCLUSION, FRUSTUM | LATE, OCCLUSION | LATE, FRUSTUM | OCCLUSION | LATE]
FLAG_EYE = (3.0, 25.0, 0.0)
FLAG_WORLD = World((64, 48), (-300.0, -350.0), (600.0, 650.0))  # z from -350 to +300: the terrain straddles the camera


@functools.lru_cache(maxsize=None)
def flag_frame():
    """(world, min / max image, camera, pyramid, prior mask, the patch the camera is inside) of the flag-set test."""
    world = FLAG_WORLD
    mm = _terrain(64, 48, 41)
    px, py = int((FLAG_EYE[0] - world.wmin[0]) / world.wsize[0] * 64), int((FLAG_EYE[2] - world.wmin[1]) / world.wsize[1] * 48)
    mm[py, px, 0], mm[py, px, 1] = 0.0, 1.0  # y from -5 to 55 around the eye's 25
    return world, mm, _camera(eye=FLAG_EYE), small_pyramid(96, 40, 4), _mask(world.total, 11, 0.35), py * 64 + px


@functools.lru_cache(maxsize=None)
def flag_classes() -> dict:
    """The patches of flag_frame() by what happens to them, from the checker alone."""
    world, mm, cam, pyr, mask, inside = flag_frame()
    centre, extent = patch_boxes(world, mm)
    hz = pyr.struct()
    every = screen_boxes(world, mm, cam, frustum=False)
    kept = {i for i, _ in screen_boxes(world, mm, cam)}
    m = mask.clone()
    early = checker(world, mm, cam, PASSES[0], hz, m)
    late = checker(world, mm, cam, PASSES[1], hz, m)
    eye = np.array(FLAG_EYE, dtype=np.float64)
    lo, hi = centre[inside] - 0.5 * extent[inside], centre[inside] + 0.5 * extent[inside]
    behind = behind_camera(cam, centre, extent)
    return {"behind": int(behind.sum()),
            "near-crossing": sum(sa is None and not behind[i] for i, sa in every),  # (a box behind the camera projects to none as well)
            "emitted early": early.numel(), "emitted late only": late.numel(),
            "occluded": sum(sa is not None and i in kept and oracle.test_occlusion(sa, hz) for i, sa in every),
            "outside the frustum": world.total - len(kept),
            "camera inside": bool((lo < eye).all() and (eye < hi).all()) and dict(every)[inside] is None}


EDGE_WORLD = World((33, 31))
EDGE_ROWS = {2: "min == max", 5: "min > max", 8: "NaN min", 9: "NaN max", 10: "NaN both", 13: "+Inf max", 14: "-Inf min", 15: "+Inf both", 16: "-Inf / +Inf",
             19: "denormals", 22: "-0.0 both", 23: "-0.0 min", 24: "-0.0 max"}


@functools.lru_cache(maxsize=None)
def edge_minmax() -> torch.Tensor:
    """The 33 x 31 min / max image whose rows hold the values of EDGE_ROWS; the other rows are an ordinary terrain."""
    mm = _terrain(33, 31, 77)
    nan, inf = float("nan"), float("inf")
    mm[2, :, 1] = mm[2, :, 0]
    mm[5] = mm[5].flip(-1) + torch.tensor([0.05, 0.0])
    mm[8, :, 0], mm[9, :, 1], mm[10] = nan, nan, nan
    mm[13, :, 1], mm[14, :, 0], mm[15], mm[16, :, 0], mm[16, :, 1] = inf, -inf, inf, -inf, inf
    mm[19, :, 0], mm[19, :, 1] = 1e-40, 3e-39
    mm[22], mm[23, :, 0], mm[24, :, 1] = -0.0, -0.0, -0.0
    mm[24, :, 0] = -0.25
    return mm.contiguous()


def _edge_camera(kind):
    cam = _camera()
    if kind == "nan":
        cam.projection_view[5] = float("nan")
    elif kind == "huge":  # rows x and y scaled: the frustum is what it is; the point is the magnitude
        for c in range(4):
            cam.projection_view[c * 4 + 0] *= 2.0 ** 101
            cam.projection_view[c * 4 + 1] *= 2.0 ** 101
    return cam


# name -> (world, camera): the parameter sets the edge image runs under
EDGE_CASES = {
    "height_scale-0": (dataclasses.replace(EDGE_WORLD, hscale=0.0), None),
    "height_scale-minus60": (dataclasses.replace(EDGE_WORLD, hscale=-60.0), None),
    "height_scale-1e30": (dataclasses.replace(EDGE_WORLD, hscale=1e30), None),
    "world_size-negative-x": (dataclasses.replace(EDGE_WORLD, wmin=(300.0, -700.0), wsize=(-600.0, 650.0)), None),
    "world_size-negative-z": (dataclasses.replace(EDGE_WORLD, wmin=(-300.0, -50.0), wsize=(600.0, -650.0)), None),
    "world_min-1e30": (dataclasses.replace(EDGE_WORLD, wmin=(1e30, -700.0)), None),
    "projection_view-nan": (EDGE_WORLD, "nan"),
    "projection_view-2^101": (EDGE_WORLD, "huge"),
}


def edge_case(name):
    world, kind = EDGE_CASES[name]
    return world, _edge_camera(kind)
