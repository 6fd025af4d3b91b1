"""The HPB shadow cull off the 64 x 64 x 10 reference shape: the shapes, layouts, poison, guard bands, scenes and the CPU-side census that
tests/test_hpb_frames.py and tests/test_gpu_hpb_shapes.py share ("HPB shapes").  Nothing here touches a GPU unless it is handed a
CUDA tensor."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

import oracle
from oxylus_amd import lib as L
from oxylus_amd.renderer import CullGeometryContext, HpbAttachment, PreparedFrame
from oxylus_amd.synth import SceneSpec, make_scene, pack_clipmaps, virtual_shadow_matrices

_F = np.float32
CLIPMAP_BYTES = 76
GUARD_RECORDS = 3       # NaN clipmap records in front of and behind the window
GUARD_WORDS = 5         # dirty words (all 1) in front of and behind the window
LIGHT = np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2])
MAX_SHADOW_DIST = 500.0
COARSEST = 256.0        # half-width of the coarsest clipmap at ten views or more, 2^(count - 1) m below that: a meshlet box (0.03 .. 2 m) is under a
                        # texel of the coarse views and half a table or more of the fine ones


def first_width(count: int) -> float:
    return min(2.0 ** (count - 1), COARSEST) / 2.0 ** (count - 1)


NON_ONE = (0x80, 0x02, 0xFF, 0x01)  # what the set level-0 bytes of the 0x00 polarity hold: the kernel ORs bytes, the checker tests != 0

# (w, h, layers, levels, clipmap_count)
SHAPES = [
    (1, 1, 1, 1, 1),         # minimum
    (2, 2, 3, 2, 2),         # layers greater than views
    (64, 64, 10, 1, 10),     # mip always clamps to 0
    (64, 64, 10, 3, 10),     # clamps at level 2
    (128, 32, 12, 8, 9),     # wide, layers greater than views
    (32, 128, 16, 8, 16),    # tall, 16 views
    (5, 3, 4, 3, 4),         # no side a power of two
    (7, 9, 16, 4, 15),       # no side a power of two, 15 views
    (4096, 1, 2, 13, 2),     # 13 levels, 4 KiB per layer
    (64, 64, 10, 7, 10),     # reference shape, control
]
REFERENCE = (64, 64, 10, 7, 10)
# one texel in one layer: every tap of every box reads the same byte, so within one polarity every page test has one outcome
ONE_TEXEL = (1, 1, 1, 1, 1)
POLARITIES = {"ff": (0xFF, 0.03), "00": (0x00, 0.9)}  # gap byte, level-0 density
DIRTY_PATTERNS = {
    "all": lambda n: [1] * n,
    "none": lambda n: [0] * n,
    "last": lambda n: [0] * (n - 1) + [1],
    "first": lambda n: [1] + [0] * (n - 1),
    "alternating": lambda n: [v & 1 for v in range(n)],
    "odd-words": lambda n: [(2, 0, 0x100, 0, -2**31)[v % 5] for v in range(n)],  # non-zero words 2, 0x100 and 0x80000000
}
LIST_LENGTHS = {1: (1, 1), 63: (3, 21), 64: (2, 32), 65: (5, 13), 255: (5, 51), 256: (4, 64), 257: (257, 1), 1023: (11, 93), 1024: (8, 128), 1025: (25, 41)}  # N: (M, K)


def shape_id(s) -> str:
    return "x".join(map(str, s[:3])) + f"-l{s[3]}-v{s[4]}"


def full_levels(w: int, h: int) -> int:
    return int(math.floor(math.log2(max(w, h)))) + 1


def level_dims(w: int, h: int, levels: int):
    return [(max(1, w >> k), max(1, h >> k)) for k in range(levels)]


def page_offset_table(size: int):
    return [0, 1, -1, size - 1, -(size - 1), size, -size, size + 1, -(size + 1), 2**20 + 3, -(2**20 + 3), 2**31 - 1, -2**31]


def offsets_for(w: int, h: int, count: int, turn: int = 0) -> np.ndarray:
    """The page-offset table cycled over the views, the two axes at different phases (independent of each other)."""
    tx, ty = page_offset_table(w), page_offset_table(h)
    return np.array([[tx[(v + turn) % 13], ty[(5 * v + 3 + turn) % 13]] for v in range(count)], dtype=np.int64).astype(np.int32)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
def packed_hpb_layout(w, h, layers, levels):
    a = HpbAttachment.create(w, h, layers, levels, "cpu")
    return list(a.level_offset), a.data.numel()


def reordered_hpb_layout(w, h, layers, levels):
    """The levels in descending address order (the top level first, level 0 last), a gap of at least w + 64 bytes between neighbours and at
    both ends, every offset odd: the pyramid is bytes, nothing may rely on an alignment.  -> (byte offsets, total bytes)"""
    offs, off = [0] * levels, 0
    for i, k in enumerate(reversed(range(levels))):
        off += w + 64 + (0, 1, 3, 6, 2, 5, 7)[i % 7]
        off += 1 - off % 2
        offs[k] = off
        off += layers * max(1, w >> k) * max(1, h >> k)
    return offs, off + w + 64 + 5


LAYOUTS = {"packed": packed_hpb_layout, "reordered": reordered_hpb_layout}


def inside_mask(w, h, layers, levels, offs, total) -> np.ndarray:
    m = np.zeros(total, dtype=bool)
    for k, (mw, mh) in enumerate(level_dims(w, h, levels)):
        assert offs[k] >= 0 and offs[k] + layers * mw * mh <= total, "level outside the allocation"
        assert not m[offs[k]: offs[k] + layers * mw * mh].any(), "levels overlap"
        m[offs[k]: offs[k] + layers * mw * mh] = True
    return m


def relaid(hpb: HpbAttachment, layout: str, gap: int) -> HpbAttachment:
    """`hpb`'s levels in `layout`, every byte outside them `gap`."""
    offs, total = LAYOUTS[layout](hpb.width, hpb.height, hpb.layers, hpb.levels)
    out = HpbAttachment(torch.full((total,), gap, dtype=torch.uint8), hpb.width, hpb.height, hpb.layers, hpb.levels, offs)
    for k in range(hpb.levels):
        out.level(k).copy_(hpb.level(k))
    inside = inside_mask(hpb.width, hpb.height, hpb.layers, hpb.levels, offs, total)
    assert (out.data.numpy()[~inside] == gap).all()
    return out


def build_or_mips(hpb: HpbAttachment):
    """Levels 1.. from level 0 with the producer's rule (rmvsm_downsample_hpb.slang:10-33): a texel ORs its 2 x 2 children, a child outside
    the level below reads 0 -- so the last column / row of an odd level has no parent.  (HpbAttachment.build_mips reshapes and needs even
    extents; this is the same OR for any extent and keeps the bytes' values.)"""
    for k in range(1, hpb.levels):
        p = hpb.level(k - 1).numpy()
        mw, mh = max(1, hpb.width >> k), max(1, hpb.height >> k)
        q = np.zeros((hpb.layers, 2 * mh, 2 * mw), dtype=np.uint8)
        ch, cw = min(2 * mh, p.shape[1]), min(2 * mw, p.shape[2])
        q[:, :ch, :cw] = p[:, :ch, :cw]
        hpb.level(k).copy_(torch.from_numpy(np.bitwise_or.reduce(q.reshape(hpb.layers, mh, 2, mw, 2), axis=(2, 4))))


def page_table(shape, polarity: str, seed: int) -> torch.Tensor:
    """int32 [layers, h, w] page words whose (visible | dirty | backed) == 7 texels are level 0: cells of about an eighth of the longer side
    (so that the upper levels are not uniformly set) plus single texels, together the polarity's density; every layer of a view holds at least
    one set and one clear texel where it has two.  Layers past the views: all set ("ff") or all clear ("00")."""
    w, h, layers, _, count = shape
    density = POLARITIES[polarity][1]
    g = torch.Generator().manual_seed(seed)
    c = max(1, max(w, h) // 8)
    ch, cw = -(-h // c), -(-w // c)
    lo = min(density, 1.0 - density)
    cells = (torch.rand((layers, ch, cw), generator=g) < lo * 0.7).repeat_interleave(c, 1).repeat_interleave(c, 2)[:, :h, :w]
    minority = cells | (torch.rand((layers, h, w), generator=g) < lo * 0.3)
    for l in range(layers):
        if w * h >= 2:
            flat = minority[l].view(-1)
            pick = torch.randperm(w * h, generator=g)
            flat[pick[0]], flat[pick[1]] = True, False
    on = minority if density < 0.5 else ~minority
    on[count:] = polarity == "ff"
    pt = torch.randint(0, 7, (layers, h, w), generator=g, dtype=torch.int32)  # some flags, never all three
    pt[on] = 7 | (5 << 16)
    return pt


def pyramid(shape, polarity: str, seed: int) -> HpbAttachment:
    """The producer's pyramid (oracle.generate_hpb) of page_table(), packed; in the "00" polarity the set level-0 bytes then take the values of
    NON_ONE and the levels above are rebuilt by OR; layers past the views are 0xFF ("ff") or 0 on every level."""
    w, h, layers, levels, count = shape
    hpb = HpbAttachment.create(w, h, layers, levels, "cpu")
    oracle.generate_hpb(page_table(shape, polarity, seed), oracle.make_hpb(hpb.data, w, h, layers, levels, hpb.level_offset))
    if polarity == "00":
        l0 = hpb.level(0).numpy()
        vals = np.array(NON_ONE, dtype=np.uint8)[np.arange(l0.size).reshape(l0.shape) % 4]
        before = [hpb.level(k).numpy() != 0 for k in range(levels)]
        l0[...] = np.where(l0 != 0, vals, 0)
        build_or_mips(hpb)
        assert all(np.array_equal(hpb.level(k).numpy() != 0, before[k]) for k in range(levels)), "the OR rebuild is not the producer's pyramid"
    for k in range(levels):
        hpb.level(k)[count:] = 0xFF if polarity == "ff" else 0
    return hpb


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
CENTRE = np.array([3.0, 1.0, -60.0])


def placed_scene(m: int, k: int, seed: int, reach: float, centre=CENTRE, **spec):
    """make_scene with the instances moved around `centre` (the clipmaps' centre): the even ones to distances drawn log-uniformly from 0.3 m ..
    `reach`, the odd ones uniformly from 0.4 .. 1 x `reach` (inside the coarsest clipmaps only)."""
    scene = make_scene(SceneSpec(n_mesh_instances=m, meshlets_per_mesh=k, seed=seed, **spec), "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    r = 0.3 * torch.exp(torch.rand(m, generator=g) * math.log(max(reach, 0.6) / 0.3))
    r = torch.where(torch.arange(m) % 2 == 1, (0.4 + 0.6 * torch.rand(m, generator=g)) * reach, r)
    d = torch.randn((m, 3), generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    scene.transforms[:, 12:15] = torch.tensor(centre, dtype=torch.float32) + d * r[:, None]
    return scene


def reach_of(count: int) -> float:
    return 1.15 * min(2.0 ** (count - 1), COARSEST)


# ---- a case ----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    shape: tuple
    polarity: str
    scene: object            # oxylus_amd.synth.Scene on the CPU
    mats: np.ndarray         # float32 [count, 16]
    offs: np.ndarray         # int32 [count, 2]
    z_near: np.ndarray       # float32 [count]
    dirty: np.ndarray        # int32 [count]
    hpb: HpbAttachment       # on the CPU, in its layout, gaps poisoned
    camera_mat: np.ndarray   # the cull camera: the coarsest clipmap of the light
    other_views: tuple = ()  # views built from another light direction (their frustum normals are not clipmap 0's)

    @property
    def count(self):
        return self.shape[4]

    def camera(self, scene=None):
        cam = (scene or self.scene).cull_camera()
        for i in range(16):
            cam.projection_view[i] = float(self.camera_mat[i])
        for i in range(3):
            cam.position[i] = float(-LIGHT[i])
        cam.near_clip = -MAX_SHADOW_DIST
        return cam

    def clip_records(self) -> torch.Tensor:
        return pack_clipmaps(self.mats, self.offs, self.z_near)

    def clip_alloc(self, flip=False):
        """(allocation, window): the records inside a larger allocation whose other records are NaN matrices (`flip`: zeros instead)."""
        g = np.full((GUARD_RECORDS, 19), 0.0 if flip else np.nan, dtype=np.float32)
        g.view(np.int32)[:, 16:18] = 0x7FFFFFFF if not flip else 0
        guard = torch.from_numpy(g.view(np.uint8).reshape(-1).copy())
        alloc = torch.cat([guard, self.clip_records(), guard])
        return alloc, alloc[GUARD_RECORDS * CLIPMAP_BYTES: (GUARD_RECORDS + self.count) * CLIPMAP_BYTES]

    def dirty_alloc(self, flip=False):
        guard = torch.full((GUARD_WORDS,), 0 if flip else 1, dtype=torch.int32)
        alloc = torch.cat([guard, torch.from_numpy(self.dirty.astype(np.int32)), guard])
        return alloc, alloc[GUARD_WORDS: GUARD_WORDS + self.count]

    def hpb_struct(self, hpb=None):
        h = hpb or self.hpb
        return oracle.make_hpb(h.data, h.width, h.height, h.layers, h.levels, h.level_offset)

    def with_hpb(self, hpb):
        return dataclasses.replace(self, hpb=hpb)

    def want(self, hpb=None, flip_guards=False, triangles=False) -> dict:
        """The checker's lists: cull_meshes against the cull camera, cull_meshlets_hpb over the window of records and dirty words."""
        cam = self.camera()
        mli, _ = oracle.cull_meshes(self.scene, cam, L.CULL_TEST_FRUSTUM)
        clip = self.clip_alloc(flip_guards)[1].clone()
        dirty = self.dirty_alloc(flip_guards)[1].clone()
        vis = oracle.cull_meshlets_hpb(self.scene, cam, mli, clip, dirty, self.hpb_struct(hpb))
        out = {"mli": mli, "visible": vis}
        if triangles:
            out["indices"] = oracle.cull_triangles(self.scene, cam, mli, vis, 0, vis.numel())
        return out


def shape_views(shape, other=True):
    """The clipmap matrices and generated page offsets of a shape: virtual_shadow_matrices of LIGHT around CENTRE; with `other`, view
    count // 2 (and view count - 2 from 15 views on) comes from another light, as test_gpu_parity._vsm_inputs(other_lights=...) does."""
    w, _, _, _, count = shape
    mats, offs, zn = virtual_shadow_matrices(CENTRE.tolist(), LIGHT, MAX_SHADOW_DIST, first_width(count), count, page_table_size=w)
    camera_mat = mats[count - 1].copy()
    others = ()
    if other and count >= 3:
        others = (count // 2,) + ((count - 2,) if count >= 15 else ())
        for v in others:
            l2 = np.array([0.3 + 0.05 * v, -1.0, 0.2 - 0.04 * v])
            m2, o2, _ = virtual_shadow_matrices(CENTRE.tolist(), l2 / np.linalg.norm(l2), MAX_SHADOW_DIST, first_width(count), count, page_table_size=w)
            mats[v], offs[v] = m2[v], o2[v]
    return mats.astype(np.float32), offs.astype(np.int32), np.full(count, zn, dtype=np.float32), camera_mat, others


def make_case(name, shape, polarity="ff", layout="packed", seed=0, dirty="all", offsets=None, scene=None, other=True) -> Case:
    w, h, layers, levels, count = shape
    mats, offs, zn, camera_mat, others = shape_views(shape, other)
    if offsets is not None:
        offs = offsets
    if scene is None:
        scene = placed_scene(36, 33, 7300 + seed, reach_of(count))
    d = np.array(DIRTY_PATTERNS[dirty](count), dtype=np.int64).astype(np.int32) if isinstance(dirty, str) else np.asarray(dirty, dtype=np.int32)
    hpb = relaid(pyramid(shape, polarity, 100 + seed), layout, POLARITIES[polarity][0])
    return Case(name, shape, polarity, scene, mats, offs, zn, d, hpb, camera_mat, others)


@functools.lru_cache(maxsize=None)
def shape_case(sid: str, layout: str, polarity: str) -> Case:
    """The case of test_shape: built once, shared by the CPU and the GPU file, never written.  "ff": all views dirty but view 1 of shapes with
    four views or more.  "00": of four views or more only view 1, view count // 2 (another light's) and the coarsest are dirty -- at a density of 0.9
    a candidate that fails the page test of every one of ten views does not occur, and one that no view accepts is what the case has to hold."""
    shape = next(s for s in SHAPES if shape_id(s) == sid)
    count = shape[4]
    dirty = [1] * count
    if count >= 4:
        dirty[1] = 0
        if polarity == "00":
            dirty = [int(v in (1, count // 2, count - 1)) for v in range(count)]
    return make_case(f"{sid}-{layout}-{polarity}", shape, polarity, layout, seed=SHAPE_SEEDS.get(shape, SHAPES.index(shape)), dirty=dirty)


SHAPE_SEEDS = {(32, 128, 16, 8, 16): 20}  # (shape: seed) where the shape's index, the default, misses a condition of test_hpb_frames.py


OFFSET_SHAPES = [REFERENCE, (128, 32, 12, 8, 9), (5, 3, 4, 3, 4)]


@functools.lru_cache(maxsize=None)
def offset_case(sid: str, turn: int) -> Case:
    shape = next(s for s in SHAPES if shape_id(s) == sid)
    return make_case(f"offsets-{sid}-turn{turn}", shape, "ff", "reordered", seed=40 + turn, offsets=offsets_for(shape[0], shape[1], shape[4], turn))


@functools.lru_cache(maxsize=None)
def dirty_case(pattern: str, polarity: str = "00") -> Case:
    return make_case(f"dirty-{pattern}-{polarity}", (32, 128, 16, 8, 16), polarity, "packed", seed=50, dirty=pattern)


@functools.lru_cache(maxsize=None)
def list_length_case(n: int) -> Case:
    m, k = LIST_LENGTHS[n]
    return make_case(f"list-{n}", REFERENCE, "00", "packed", seed=60, scene=placed_scene(m, k, 7400 + n, 40.0, degenerate_cone_frac=1.0))


def _cone_scene(m: int, k: int, seed: int, keep):
    """Every meshlet passes the cone test (cutoff 1: cull.slang's `cutoff >= 1` arm) but those `keep(mi, j)` refuses, which no direction passes
    (cutoff -1: dot >= -1 culls)."""
    scene = placed_scene(m, k, seed, 40.0, degenerate_cone_frac=1.0)
    b = scene.bounds.view(m, k, 8)
    for mi in range(m):
        for j in range(k):
            if not keep(mi, j):
                b[mi, j, 7] = int(b[mi, j, 7]) & 0xFF | (-127 << 8)
    return scene


ROUND_KEEP = (256, 160, 224, 40)  # cone survivors of the four 256-meshlet instances: one round each of total 256, 129..191, 193..255, 1..63


@functools.lru_cache(maxsize=None)
def round_case(which: str) -> Case:
    if which == "bands":
        scene = _cone_scene(4, 256, 7500, lambda mi, j: j < ROUND_KEEP[mi])
    else:  # "instances": one-meshlet instances, 256 distinct ones per run
        scene = _cone_scene(300, 1, 7501, lambda mi, j: mi % 7 != 3)
    return make_case(f"rounds-{which}", REFERENCE, "ff", "reordered", seed=61, scene=scene)


@functools.lru_cache(maxsize=None)
def none_case(which: str) -> Case:
    """"z_near": view 1 of three orthographic views has z_near = 1.5 -- the affine path's 1.0f < near_clip.  "perspective": view 1 of four is the
    scene's main camera (perspective, its own z_near) and the instances stand around that camera, so that boxes cross its near plane -- the
    general path's depth < near_clip."""
    if which == "z_near":
        case = make_case("none-z_near", (64, 64, 10, 7, 3), "ff", "packed", seed=70, other=False)
        case.z_near[1] = 1.5
        return case
    centre = np.array([0.0, 0.0, -0.5])
    scene = placed_scene(60, 33, 7600, 30.0, centre=centre)
    case = make_case("none-perspective", (64, 64, 10, 7, 4), "ff", "packed", seed=71, scene=scene, other=False)
    mats, offs, _ = virtual_shadow_matrices(centre.tolist(), LIGHT, MAX_SHADOW_DIST, 4.0, 4)
    case.mats[:], case.offs[:], case.camera_mat = mats, offs, mats[3].copy()
    # instance 0 stands at the camera, and twelve of its boxes (0.3 m, every cone passes) straddle the near plane z = -0.1 next to the axis
    scene.transforms[0] = torch.eye(4).reshape(-1)
    f16 = lambda *v: torch.tensor(v, dtype=torch.float32).to(torch.float16).view(torch.int16)  # noqa: E731
    for j in range(12):
        scene.bounds[j, 0:3] = f16(0.02 * j - 0.1, 0.03 * (j % 3) - 0.03, -0.2 + 0.05 * (j % 4))
        scene.bounds[j, 4:7] = f16(0.3, 0.3, 0.3)
        scene.bounds[j, 7] = int(scene.bounds[j, 7]) & 0xFF | (127 << 8)
    case.mats[1] = np.asarray(scene.camera["projection_view"], dtype=np.float32)
    case.z_near[1] = scene.camera["near_clip"]
    return case


# ---- the census ------------------------------------------------------------------------------------------------------------------------------
def _raw_mip(box: np.float32) -> int:
    """ceil(log2(box)) without the upper clamp; box <= 0, NaN and denormals -> 0 (cull.slang:146-147 after its lower clamp)."""
    if not box > 0 or not np.isfinite(box):
        return 0 if not box > 0 else 10**6
    m, e = math.frexp(float(box))
    return max(e - 1 if m == 0.5 else e, 0)


def census(case: Case) -> dict:
    """A walk of the case with the checker's primitives and numpy: what the case makes the kernel do.  Reproduces cull_meshlets_hpb's list
    (asserted)."""
    scene, (w, h, layers, levels, count) = case.scene, case.shape
    want = case.want()
    mli = want["mli"].numpy()
    cam = case.camera()
    K = scene.spec.meshlets_per_mesh
    assert scene.spec.lod_count == 1 and scene.spec.share_meshes == 0  # bounds row == mesh instance * K + meshlet
    bounds = oracle.decode_bounds(scene.bounds.numpy())
    tr = scene.transforms.numpy()
    hpbs = case.hpb_struct()
    # the candidates -- cone and camera-frustum survivors -- from the checker itself: one dirty view with the camera's matrix and z_near = +Inf,
    # so that every box inside it is "none" and visible without a page test
    probe = pack_clipmaps(np.asarray(case.camera_mat, dtype=np.float32)[None], np.zeros((1, 2), np.int32), np.array([np.inf], np.float32))
    cand = oracle.cull_meshlets_hpb(scene, cam, want["mli"], probe, torch.ones(1, dtype=torch.int32), hpbs).numpy()
    views = [dict(in_frustum=0, none=0, mips={}, clamped=0, wrapped=[0, 0], seam=[0, 0], passed=0, failed=0, only=0) for _ in range(count)]
    first, nobody, kept = [0] * count, 0, []
    sw, sh = _F(w), _F(h)
    mvps = {}
    for i in cand.tolist():
        mi, row = int(mli[i, 0]), int(mli[i, 0]) * K + int(mli[i, 1])
        c, e = bounds[row, 0:3], bounds[row, 3:6]
        accepted = []
        for v in range(count):
            if case.dirty[v] == 0:
                continue
            if (mi, v) not in mvps:
                mvps[mi, v] = oracle.mul_mat4(case.mats[v], tr[mi])
            if not oracle.test_frustum(mvps[mi, v], c, e):
                continue
            s = views[v]
            s["in_frustum"] += 1
            sa = oracle.project_aabb(mvps[mi, v], float(case.z_near[v]), c, e)
            if sa is None:
                s["none"] += 1
                accepted.append(v)
                continue
            raw = _raw_mip(np.fmax((sa[3] - sa[0]) * sw, (sa[4] - sa[1]) * sh))
            mip = min(raw, levels - 1)
            s["mips"][mip] = s["mips"].get(mip, 0) + 1
            s["clamped"] += raw > levels - 1
            for axis, (lo, hi, size, ext) in enumerate(((sa[0], sa[3], sw, w), (sa[1], sa[4], sh, h))):
                po = _F(case.offs[v][axis]) / size
                t0, t1 = _F(lo + po), _F(hi + po)
                s["wrapped"][axis] += int(np.floor(t0) != 0) + int(np.floor(t1) != 0)
                mext = max(1, ext >> mip)
                x0, x1 = (min(int(_F(t - np.floor(t)) * _F(mext)), mext - 1) if np.isfinite(t) else 0 for t in (t0, t1))
                s["seam"][axis] += x1 < x0
            if oracle.test_vsm_page(sa, hpbs, v, case.offs[v]):
                s["passed"] += 1
                accepted.append(v)
            else:
                s["failed"] += 1
        if accepted:
            first[accepted[0]] += 1
            kept.append(i)
            if len(accepted) == 1:
                views[accepted[0]]["only"] += 1
        else:
            nobody += 1
    assert np.array_equal(np.array(kept, dtype=np.int32), want["visible"].numpy()), f"{case.name}: the census walk is not the checker's cull_meshlets_hpb"
    is_cand = np.zeros(len(mli), dtype=bool)
    is_cand[cand] = True
    runs = []
    for r0 in range(0, len(mli), 256):
        inst = mli[r0:r0 + 256, 0]
        runs.append({int(m): int(is_cand[r0:r0 + 256][inst == m].sum()) for m in np.unique(inst)})
    return {"n": len(mli), "candidates": len(cand), "visible": len(kept), "views": views, "first": first, "nobody": nobody, "runs": runs}


def census_line(case: Case, c: dict) -> str:
    tot = lambda key: sum(v[key] for v in c["views"])  # noqa: E731
    mips = sorted({m for v in c["views"] for m in v["mips"]})
    wrapped = [sum(v["wrapped"][a] for v in c["views"]) for a in (0, 1)]
    seam = [sum(v["seam"][a] for v in c["views"]) for a in (0, 1)]
    return (f"{case.name}: N {c['n']} candidates {c['candidates']} visible {c['visible']} nobody {c['nobody']} in-frustum {tot('in_frustum')} none {tot('none')} "
            f"passed {tot('passed')} failed {tot('failed')} mips {mips} clamped {tot('clamped')} wrapped {wrapped} seam {seam} first {c['first']}")


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------
class Upload:
    """A case's inputs on the GPU: the scene, the HPB allocation, the clipmap and dirty allocations with their windows."""

    def __init__(self, case: Case, triangles=False):
        self.case = case
        self.scene = case.scene.to("cuda")
        self.frame = PreparedFrame.create(self.scene, with_triangles=triangles, expand=False)
        self.hpb_cpu = case.hpb.data.clone()
        self.hpb = HpbAttachment(case.hpb.data.cuda(), case.hpb.width, case.hpb.height, case.hpb.layers, case.hpb.levels, list(case.hpb.level_offset))
        self.clip_cpu, _ = case.clip_alloc()
        self.dirty_cpu, _ = case.dirty_alloc()
        self.clip_all, self.dirty_all = self.clip_cpu.cuda(), self.dirty_cpu.cuda()
        self.clip = self.clip_all[GUARD_RECORDS * CLIPMAP_BYTES: (GUARD_RECORDS + case.count) * CLIPMAP_BYTES]
        self.dirty = self.dirty_all[GUARD_WORDS: GUARD_WORDS + case.count]
        self.stages = L.STAGE_ALL if triangles else L.STAGE_MESHES | L.STAGE_MESHLETS

    def context(self, **over) -> CullGeometryContext:
        kw = dict(use_hpb=True, init_cull_meshes=True, cull_flags=L.CULL_TEST_FRUSTUM, cull_camera=self.case.camera(self.scene), hpb_attachment=self.hpb,
                  vsm_clipmaps_buffer=self.clip, vsm_clipmap_dirty_flags_buffer=self.dirty, vsm_clipmap_count=self.case.count, stages=self.stages)
        kw.update(over)
        return CullGeometryContext(**kw)

    def run(self, renderer, stream=None) -> dict:
        renderer.prepared_frame = self.frame
        ctx = self.context()
        renderer.cull_geometry(ctx, stream=stream)
        return self.read(renderer, ctx)

    def read(self, renderer, ctx) -> dict:
        c = renderer.read_counters(ctx)
        out = {"total": c.total_visible_meshlet_instances, "mli": self.frame.meshlet_instances_buffer[:c.total_visible_meshlet_instances].cpu(),
               "visible": self.frame.visible_meshlet_instances_indices_buffer[:c.cull_triangles_cmd_x].cpu()}
        if self.stages & L.STAGE_TRIANGLES:
            out["indices"] = self.frame.reordered_indices_buffer[:c.draw_index_count].cpu()
        return out

    def assert_inputs_untouched(self):
        assert torch.equal(self.hpb.data.cpu(), self.hpb_cpu), "the kernel wrote into the HPB allocation"
        assert torch.equal(self.clip_all.cpu(), self.clip_cpu), "the kernel wrote into the clipmap allocation"
        assert torch.equal(self.dirty_all.cpu(), self.dirty_cpu), "the kernel wrote into the dirty-flag allocation"


def assert_equals_checker(want: dict, got: dict, what=""):
    assert got["total"] == want["mli"].shape[0], what
    assert torch.equal(got["mli"], want["mli"]), what
    assert torch.equal(got["visible"], want["visible"]), f"{what}: {got['visible'].numel()} visible, the checker has {want['visible'].numel()}"
    if "indices" in want:
        assert torch.equal(got["indices"], want["indices"]), what
