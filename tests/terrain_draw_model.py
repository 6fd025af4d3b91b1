"""The numpy checker of oxc_draw_terrain: steps T1 - T7 of its header block in include/oxcull.h, restated.  Every binary32 operation is one
numpy float32 operation in the order the header states.  It adds the tessellator's rules (T2 - T6) and joins rules that already have a
Python copy: sample_height (B3) from terrain_brush_model, the projection_view multiply from pixel_rules, the clip classes and the clipper
from vsm_draw_model, the set-up and the walk of a big pixel box from raster_model.  Vectorised per patch (a 63-factor patch has 7938
triangles); pixel boxes up to 8 x 8 are evaluated at once, larger ones one at a time.  Images are numpy: heightmap uint16 [h, w], the
depth|vis image uint64 [H, W].  `counts`, when given, receives what oxc_debug_terrain_draw_stats reports (patches_drawn, patches_discarded,
patches_skipped, triangles, set_up, clipped, big, fragments) and the checker's own branch counts: patches_all_one, inner_redone, and per ring side k
side{k}_outer_steps, side{k}_inner_steps, side{k}_ties, side{k}_inner_exhausted_first, side{k}_outer_exhausted_first.  CPU only."""
from __future__ import annotations

import dataclasses
from fractions import Fraction

import numpy as np

import raster_model as RM
import terrain_brush_model as TB
import vsm_draw_model as VD
from pixel_rules import count, mul_mp

F = np.float32
VIS = 0xFFFFFE00  # VisBufferData(TERRAIN_INSTANCE_ID, 0).encode()
MAX_FACTOR = F(63.0)
EDGES = ((0, 3), (0, 1), (1, 2), (3, 2))  # corner pairs of edges 0 .. 3
CORNERS = ((0, 0), (1, 0), (1, 1), (0, 1))
STATS = ("patches_drawn", "patches_discarded", "patches_skipped", "triangles", "set_up", "clipped", "big")


@dataclasses.dataclass
class Camera:
    projection_view: np.ndarray  # float32 [16], column-major
    position: tuple
    near_clip: float
    projection_scale: float


def projection_scale(resolution_y, fov_degrees) -> float:
    """The engine's resolution.y * 0.5 / tan(radians(fov) * 0.5) in binary64, rounded to binary32 once (T2)."""
    import math

    return float(F(float(resolution_y) * 0.5 / math.tan(math.radians(float(fov_degrees)) * 0.5)))


# ---- T1, T2 ----------------------------------------------------------------------------------------------------------------------------------------
def _brush_params(T, heightmap):
    h, w = heightmap.shape
    return TB.Params(resolution=(w, h), world_min=T.world_min, world_size=T.world_size, inv_world_size=T.inv_world_size, base_height=T.base_height,
                     height_scale=T.height_scale)


@np.errstate(all="ignore")
def corners(T, heightmap, p: int) -> np.ndarray:
    """T1: world positions float32 [4, 3] of patch index p."""
    pcx, pcy = int(T.patch_count[0]), int(T.patch_count[1])
    B = _brush_params(T, heightmap)
    out = np.zeros((4, 3), np.float32)
    for c, (cu, cv) in enumerate(CORNERS):
        gx, gz = F(p % pcx + cu) / F(pcx), F(p // pcx + cv) / F(pcy)
        x, z = F(T.world_min[0]) + gx * F(T.world_size[0]), F(T.world_min[1]) + gz * F(T.world_size[1])
        out[c] = (x, TB.sample_height(B, heightmap, np.array([x], np.float32), np.array([z], np.float32))[0], z)
    return out


@np.errstate(all="ignore")
def _distance(a, b):
    d = (a - b).astype(np.float32)
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


@np.errstate(all="ignore")
def edge_factor(T, cam: Camera, a, b):
    center = ((a + b) * F(0.5)).astype(np.float32)
    radius = _distance(a, b) * F(0.5)
    view_distance = np.fmax(_distance(center, np.asarray(cam.position, np.float32)) - radius, F(cam.near_clip))
    projected = ((F(2.0) * radius) * F(cam.projection_scale)) / view_distance
    return np.fmin(np.fmax(projected / F(T.target_edge_pixels), F(1.0)), F(T.max_tessellation))


def factors(T, cam: Camera, cs) -> list:
    return [edge_factor(T, cam, cs[a], cs[b]) for a, b in EDGES]


# ---- T3 --------------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def clamp_factor(f):
    return np.fmin(np.fmax(F(f), F(1.0)), MAX_FACTOR)


def segments(fc) -> int:
    c = int(np.ceil(fc))
    return c if c % 2 else c + 1


def parameters(fc, n: int) -> np.ndarray:
    """The n + 1 parameters float32 of a list with clamped factor fc and n segments."""
    t = np.zeros(n + 1, np.float32)
    t[n] = F(1.0)
    if n == 1:
        return t
    r = F(1.0) / F(fc)
    s = (F(1.0) - F(n - 2) * r) * F(0.5)
    h = (n - 1) // 2
    for k in range(1, h + 1):
        t[k] = s + F(k - 1) * r
    for k in range(h + 1, n):
        t[k] = F(1.0) - t[n - k]
    return t


def subdivide(f):
    """T3 for one factor: (n, parameters)."""
    fc = clamp_factor(f)
    n = segments(fc)
    return n, parameters(fc, n)


# ---- T4 --------------------------------------------------------------------------------------------------------------------------------------------
def triangle_count(n6) -> int:
    n0, n1, n2, n3, nu, nv = n6
    return 2 * (nu - 2) * (nv - 2) + (n0 + nv - 2) + (n2 + nv - 2) + (n1 + nu - 2) + (n3 + nu - 2)


def lists_of(e4):
    """The six (n, parameters) of edge factors e4: edges 0 .. 3, inner u, inner v -- with an inner n of 1 redone unless all six are 1."""
    fcs = [clamp_factor(e) for e in e4] + [clamp_factor(np.fmax(e4[1], e4[3])), clamp_factor(np.fmax(e4[0], e4[2]))]
    ns = [segments(fc) for fc in fcs]
    redone = 0
    if any(n != 1 for n in ns):
        for k in (4, 5):
            if ns[k] == 1:
                fcs[k], ns[k] = np.array(0x3F800001, np.uint32).view(np.float32), 3
                redone += 1
    return [(n, parameters(fc, n)) for n, fc in zip(ns, fcs)], redone


def topology(lists, counts=None):
    """T4: (u float32 [P], v float32 [P], triangles int64 [K, 3]) of a patch, every triangle counter-clockwise in (u, v) unless its area is zero."""
    (n0, t0), (n1, t1), (n2, t2), (n3, t3), (nu, U), (nv, V) = lists
    if all(n == 1 for n, _ in lists):
        count(counts, "patches_all_one")
        return np.array([0, 1, 1, 0], np.float32), np.array([0, 0, 1, 1], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int64)
    pw = nu - 1  # inner points a row
    u = [np.tile(U[1:nu], nv - 1)]
    v = [np.repeat(V[1:nv], pw)]
    j, i = np.mgrid[0:nv - 2, 0:nu - 2]
    p00 = (j * pw + i).reshape(-1)
    tris = [np.stack([p00, p00 + 1, p00 + pw + 1], 1), np.stack([p00, p00 + pw + 1, p00 + pw], 1)]
    base = pw * (nv - 1)
    inner_of = {0: lambda k: k * pw, 1: lambda k: k, 2: lambda k: k * pw + pw - 1, 3: lambda k: (nv - 2) * pw + k}  # inner point k of the side's axis list (0-based)
    for side, (no, to) in enumerate(((n0, t0), (n1, t1), (n2, t2), (n3, t3))):
        along_v = side % 2 == 0
        axis, ni = (V, nv - 2) if along_v else (U, nu - 2)
        fixed = F(1.0) if side >= 2 else F(0.0)
        u.append(np.full(no + 1, fixed, np.float32) if along_v else to)
        v.append(to if along_v else np.full(no + 1, fixed, np.float32))
        oa = ib = 0
        flip = side in (1, 2)
        while oa < no or ib < ni:
            outer = ib == ni or (oa < no and to[oa + 1] <= axis[ib + 2])
            if counts is not None:
                count(counts, f"side{side}_{'outer' if outer else 'inner'}_steps")
                if outer and ib < ni and to[oa + 1] == axis[ib + 2]:
                    count(counts, f"side{side}_ties")
                if ib == ni - 1 and not outer and oa < no:
                    count(counts, f"side{side}_inner_exhausted_first")
                if oa == no - 1 and outer and ib < ni:
                    count(counts, f"side{side}_outer_exhausted_first")
            c0, c1 = base + oa, inner_of[side](ib)
            c2 = base + oa + 1 if outer else inner_of[side](ib + 1)
            tris.append(np.array([[c0, c2, c1] if flip else [c0, c1, c2]], np.int64))
            oa, ib = (oa + 1, ib) if outer else (oa, ib + 1)
        base += no + 1
    return np.concatenate(u).astype(np.float32), np.concatenate(v).astype(np.float32), np.concatenate(tris).astype(np.int64)


# ---- T5 --------------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def _lerp_end(a, b, t):
    return np.where(t == 0, a, np.where(t == 1, b, a + (b - a) * t)).astype(np.float32)


@np.errstate(all="ignore")
def domain_points(T, heightmap, cs, u, v) -> np.ndarray:
    """World positions float32 [P, 3] of the domain points (u, v) of the patch with corners cs."""
    ax, az = _lerp_end(cs[0, 0], cs[1, 0], u), _lerp_end(cs[0, 2], cs[1, 2], u)
    bx, bz = _lerp_end(cs[3, 0], cs[2, 0], u), _lerp_end(cs[3, 2], cs[2, 2], u)
    x, z = _lerp_end(ax, bx, v), _lerp_end(az, bz, v)
    y = TB.sample_height(_brush_params(T, heightmap), heightmap, x, z)
    return np.stack([x, y, z], 1).astype(np.float32)


# ---- T6, T7 ----------------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def _snap(clip, W, H):
    """[K, 3, 4] -> (kept, X, Y, z): the snap and cullMode eBack (fixed-point area >= 0 dropped), corners 1 and 2 exchanged: positive area."""
    w = clip[..., 3]
    sx = ((clip[..., 0] / w) * F(0.5) + F(0.5)) * F(W)
    sy = ((clip[..., 1] / w) * F(0.5) + F(0.5)) * F(H)
    z = (clip[..., 2] / w).astype(np.float32)
    ok = (w > 0).all(1) & (np.abs(sx) <= RM.RANGE).all(1) & (np.abs(sy) <= RM.RANGE).all(1)
    X = np.where(ok[:, None], np.floor(sx * F(256.0) + F(0.5)), F(0)).astype(np.int64)
    Y = np.where(ok[:, None], np.floor(sy * F(256.0) + F(0.5)), F(0)).astype(np.int64)
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    order = [0, 2, 1]
    return ok & (area < 0), X[:, order], Y[:, order], z[:, order]


def _small_fragments(image, X, Y, z, px0, py0, px1, py1):
    """Oriented triangles [K] whose boxes are at most 8 x 8: cover (top-left), binary64 depth, the (0, 1] test, the maximum."""
    kk = np.arange(RM.SMALL_SPAN * RM.SMALL_SPAN)
    px, py = px0[:, None] + kk % RM.SMALL_SPAN, py0[:, None] + kk // RM.SMALL_SPAN
    inbox = (px <= px1[:, None]) & (py <= py1[:, None])
    cx, cy = px * 256 + 128, py * 256 + 128

    def edge(a, b):
        return (X[:, b, None] - X[:, a, None]) * (cy - Y[:, a, None]) - (Y[:, b, None] - Y[:, a, None]) * (cx - X[:, a, None])

    e = [edge(1, 2), edge(2, 0), edge(0, 1)]
    bias = [np.where(VD._incl(X[:, a], Y[:, a], X[:, b], Y[:, b]), 0, -1)[:, None] for a, b in ((1, 2), (2, 0), (0, 1))]
    inside = inbox & (e[0] + bias[0] >= 0) & (e[1] + bias[1] >= 0) & (e[2] + bias[2] >= 0)
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    inv = 1.0 / area.astype(np.float64)
    zd = ((e[0].astype(np.float64) * z[:, 0, None].astype(np.float64) + e[1].astype(np.float64) * z[:, 1, None].astype(np.float64)) +
          e[2].astype(np.float64) * z[:, 2, None].astype(np.float64)) * inv[:, None]
    zf = zd.astype(np.float32)
    with np.errstate(invalid="ignore"):
        keep = inside & (zf > 0) & ~(zf > 1)
    packed = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(VIS)
    H, W = image.shape
    np.maximum.at(image.reshape(-1), (py * W + px)[keep], packed[keep])
    return int(keep.sum())


def raster(image, clip, counts=None):
    """T7 on triangles clip float32 [K, 3, 4] in T6's corner order, into `image` (uint64 [H, W])."""
    H, W = image.shape
    if len(clip) == 0:
        return
    cls = VD.clip_class(clip)
    groups, from_clipper = [clip[cls == 0]], [np.zeros(int((cls == 0).sum()), bool)]
    for t in np.flatnonzero(cls == 1):
        with np.errstate(all="ignore"):
            pieces = VD.clip_polygon(clip[t])
        groups += [p[None] for p in pieces]
        from_clipper.append(np.ones(len(pieces), bool))
    tris, fc = np.concatenate(groups).reshape(-1, 3, 4).astype(np.float32), np.concatenate(from_clipper)
    kept, X, Y, z = _snap(tris, W, H)
    X, Y, z, fc = X[kept], Y[kept], z[kept], fc[kept]
    count(counts, "clipped", int((cls == 1).sum()))
    if len(X) == 0:
        return
    minx, maxx, miny, maxy = X.min(1), X.max(1), Y.min(1), Y.max(1)
    px0, py0 = np.maximum((minx - 128 + 255) >> 8, 0), np.maximum((miny - 128 + 255) >> 8, 0)
    px1, py1 = np.minimum((maxx - 128) >> 8, W - 1), np.minimum((maxy - 128) >> 8, H - 1)
    boxed = (px1 >= px0) & (py1 >= py0)
    fits = (px1 - px0 < RM.SMALL_SPAN) & (py1 - py0 < RM.SMALL_SPAN)
    small = boxed & fits & (fc | (np.maximum(maxx - minx, maxy - miny) < RM.SMALL_SPREAD))
    count(counts, "set_up", len(X))
    count(counts, "big", int((boxed & ~small).sum()))
    s = boxed & fits  # every walk writes the same texels: the box alone decides how the checker evaluates it
    if s.any():
        count(counts, "fragments", _small_fragments(image, X[s], Y[s], z[s], px0[s], py0[s], px1[s], py1[s]))
    for i in np.flatnonzero(boxed & ~fits):
        t = RM.setup(([int(X[i, 0]), int(X[i, 2]), int(X[i, 1])], [int(Y[i, 0]), int(Y[i, 2]), int(Y[i, 1])], [z[i, 0], z[i, 2], z[i, 1]]), W, H)
        RM.draw_triangle(t, VIS, image)
        if counts is not None:  # the fragments of this triangle alone: what it leaves in an empty window of its own box
            alone = np.zeros((H, W), np.uint64)
            RM.draw_triangle(t, VIS, alone)
            count(counts, "fragments", int((alone[t["py0"]:t["py1"] + 1, t["px0"]:t["px1"] + 1] != 0).sum()))


def patch_clip(T, heightmap, cam: Camera, p: int, counts=None):
    """T1 - T6 for patch index p: clip-space triangles float32 [K, 3, 4] in the order the set-up takes them, or None when T2 discards it."""
    cs = corners(T, heightmap, p)
    e4 = factors(T, cam, cs)
    if any(not (e > 0) for e in e4):
        count(counts, "patches_discarded")
        return None
    lists, redone = lists_of(e4)
    count(counts, "inner_redone", redone)
    u, v, tris = topology(lists, counts)
    count(counts, "patches_drawn")
    count(counts, "triangles", len(tris))
    assert all(n == 1 for n, _ in lists) or len(tris) == triangle_count([n for n, _ in lists])
    world = domain_points(T, heightmap, cs, u, v)
    with np.errstate(all="ignore"):
        clip = mul_mp(np.asarray(cam.projection_view, np.float32), world)
    return clip[tris[:, [0, 2, 1]]]


def draw(T, heightmap, cam: Camera, visible, draw_cmd, W, H, image=None, clear=True, counts=None) -> np.ndarray:
    """One oxc_draw_terrain call: the depth|vis image uint64 [H, W] after it (`image`, the image before it, is not changed)."""
    img = np.zeros((H, W), np.uint64) if clear or image is None else np.array(image, dtype=np.uint64).reshape(H, W).copy()
    cmd = np.asarray(draw_cmd).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    vis = np.asarray(visible).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    patches = int(T.patch_count[0]) * int(T.patch_count[1])
    if counts is not None:
        for k in STATS + ("fragments",):
            counts.setdefault(k, 0)
    for i in range(int(cmd[1])):
        entry = int(cmd[3]) + i
        if entry >= len(vis) or int(vis[entry]) >= patches:
            count(counts, "patches_skipped")
            continue
        clip = patch_clip(T, heightmap, cam, int(vis[entry]), counts)
        if clip is not None:
            raster(img, clip, counts)
    return img


def resolve(image):
    """(depth float32 [H, W], vis uint32 [H, W]) of a depth|vis image."""
    return (image >> np.uint64(32)).astype(np.uint32).view(np.float32), (image & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- exact coverage of the (u, v) square, for the tests ----------------------------------------------------------------------------------------
def lattice_coverage(u, v, tris, n: int = 24) -> np.ndarray:
    """How many triangles cover each point ((i + 1/2) / n, (j + 1/2) / n) of the unit square, in exact integers (every coordinate scaled
    by its common power-of-two denominator), with the rasteriser's top-left rule on counter-clockwise triangles: int [n, n]."""
    fr = [[Fraction(float(a)) for a in arr] for arr in (u, v)]
    D = max([f.denominator for arr in fr for f in arr] + [2 * n if n & (n - 1) == 0 else 1])
    assert D & (D - 1) == 0 and n & (n - 1) == 0
    U = [int(f * D) for f in fr[0]]
    V = [int(f * D) for f in fr[1]]
    pts = [(2 * i + 1) * D // (2 * n) for i in range(n)]
    cover = np.zeros((n, n), np.int64)
    for a, b, c in np.asarray(tris).tolist():
        xs, ys = (U[a], U[b], U[c]), (V[a], V[b], V[c])
        area = RM.edge(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2])
        if area == 0:
            continue
        assert area > 0, "clockwise in (u, v)"
        i0, i1 = [k for k in range(n) if min(xs) <= pts[k] <= max(xs)], [k for k in range(n) if min(ys) <= pts[k] <= max(ys)]
        for j in i1:
            for i in i0:
                ok = True
                for k in range(3):
                    p, q = (k + 1) % 3, (k + 2) % 3
                    e = RM.edge(xs[p], ys[p], xs[q], ys[q], pts[i], pts[j])
                    # counter-clockwise with v up is the rasteriser's positive orientation mirrored: an edge owns its points when it goes up, or is horizontal going right
                    owns = (ys[q] - ys[p]) > 0 or ((ys[q] - ys[p]) == 0 and (xs[q] - xs[p]) > 0)
                    if e < 0 or (e == 0 and not owns):
                        ok = False
                        break
                cover[j, i] += ok
    return cover
