"""Checker of oxc_resolve_shadowmap: the resolve_shadowmaps pass (Shadowmaps.cpp:756-822) restated in numpy binary32, vectorised over
pixels, under the rules include/oxcull.h states: the Slang's evaluation order, no contraction, IEEE division and square root, the integer
pixel hash in place of the sin hash, and the rotation pair from an exact octant reduction and two binary64 polynomials.  unproject, the
clipmap index, the texel length, floor_mod wrapping and the clipmap records are those of tests/vsm_pages_model.py."""
from __future__ import annotations

import numpy as np

from pixel_rules import COS_C, PIO2, SIN_C, _m, cos_sin_turn, cross, decode_normal, dot, length, normalize, unproject, vec3_to_oct
from vsm_pages_model import BACKED, clipmap_index, texel_length, unpack_clipmaps, wrap

F = np.float32
BLOCKER_SAMPLES, PCF_SAMPLES = 16, 24
SEARCH_RADIUS, LIGHT_WIDTH, MAX_PCF_RADIUS = F(0.1), F(0.002), F(0.1)
SQRT2, QUANTIZE = F(1.41421356), F(2.0 ** -22)
MISS = F(-1.0)
# outcome of a pixel
SKY, HARD, NO_BLOCKER, ALL_BLOCKERS, PCF = 0, 1, 2, 3, 4

# ---- rule 5: noise ------------------------------------------------------------------------------------------------------------------------
def pcg2d(x, y):
    """pcg2d (Jarzynski and Olano, JCGT 9(3), 2020) on u32 arrays, every operation modulo 2^32."""
    vx, vy = np.atleast_1d(x).astype(np.uint32), np.atleast_1d(y).astype(np.uint32)
    m, a = np.uint32(1664525), np.uint32(1013904223)
    vx, vy = vx * m + a, vy * m + a
    vx = vx + vy * m
    vy = vy + vx * m
    vx, vy = vx ^ (vx >> np.uint32(16)), vy ^ (vy >> np.uint32(16))
    vx = vx + vy * m
    vy = vy + vx * m
    return vx ^ (vx >> np.uint32(16)), vy ^ (vy >> np.uint32(16))


def noise(x, y):
    """(float(h.x >> 8) * 2^-24, float(h.y >> 8) * 2^-24) of h = pcg2d(x, y): two binary32 values in [0, 1)."""
    hx, hy = pcg2d(x, y)
    return (hx >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24), (hy >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24)


def pcg2d_scalar(x: int, y: int):
    """The same in plain Python integers."""
    M = 0xFFFFFFFF
    vx, vy = (x * 1664525 + 1013904223) & M, (y * 1664525 + 1013904223) & M
    vx = (vx + vy * 1664525) & M
    vy = (vy + vx * 1664525) & M
    vx, vy = vx ^ (vx >> 16), vy ^ (vy >> 16)
    vx = (vx + vy * 1664525) & M
    vy = (vy + vx * 1664525) & M
    return vx ^ (vx >> 16), vy ^ (vy >> 16)


def hammersley2d(i: int, N: int):
    """(f32(i) / f32(N), f32(reversebits(i)) * 2^-32)."""
    rev = int(f"{i:032b}"[::-1], 2)
    return F(i) / F(N), F(rev) * F(2.0 ** -32)


def fract(x):
    return x - np.floor(x)


# ---- rule 6: rotation ---------------------------------------------------------------------------------------------------------------------
def cos_sin_turn_scalar(t):
    """The same, one value, in Python floats (binary64) with explicit binary32 roundings."""
    q4 = float(F(t)) * 4.0
    k = int(q4 // 1.0)
    f = q4 - k
    swap = f > 0.5
    g = 1.0 - f if swap else f
    a = g * PIO2
    z = a * a
    ps = ((SIN_C[3] * z + SIN_C[2]) * z + SIN_C[1]) * z + SIN_C[0]
    s = F(a + (a * z) * ps)
    pc = (((COS_C[4] * z + COS_C[3]) * z + COS_C[2]) * z + COS_C[1]) * z + COS_C[0]
    c = F(1.0 + z * pc)
    sq, cq = (c, s) if swap else (s, c)
    return [(cq, sq), (-sq, cq), (-cq, -sq), (sq, -cq)][k]


def perpendicular_basis(L):
    L = tuple(F(v) for v in L)
    axis = (F(0), F(1), F(0)) if abs(L[1]) < F(0.999) else (F(1), F(0), F(0))
    with np.errstate(all="ignore"):
        t = normalize(cross(axis, L))
        return t, cross(L, t)


def _row(c, r, p):
    return ((_m(c, r, 0) * p[0] + _m(c, r, 1) * p[1]) + _m(c, r, 2) * p[2]) + _m(c, r, 3)


# ---- rule 4: a tap ------------------------------------------------------------------------------------------------------------------------
class Shape:
    """The per-call state of the taps: shape, clipmap records, page table (uint32 [count, n, n]) and physical image (float32 [phys, phys])."""

    def __init__(self, table, clipmaps, physical, *, page_size: int, page_table_size: int, physical_page_table_size: int, clipmap_count: int):
        self.ps, self.n, self.phys, self.count = page_size, page_table_size, physical_page_table_size, clipmap_count
        self.P, self.V = physical_page_table_size // page_size, page_table_size * page_size
        mats, offs, _ = unpack_clipmaps(clipmaps)
        self.mats, self.offs = mats[:clipmap_count], offs[:clipmap_count].astype(np.int64)
        self.table = np.ascontiguousarray(np.asarray(table)).view(np.uint32).reshape(clipmap_count, self.n, self.n)
        self.physical = np.asarray(physical, dtype=np.float32).reshape(self.phys, self.phys)


def tap_address(S: Shape, ci, p):
    """sample_vsm_shadow_depth up to the load: (ok, X, Y) -- the physical texel clipmap `ci` reads for world position p, ok False on a miss."""
    ci = np.asarray(ci, dtype=np.int64)
    valid = (ci >= 0) & (ci < S.count)
    cc = np.clip(ci, 0, S.count - 1)
    c = S.mats[cc]
    with np.errstate(all="ignore"):
        hx, hy, hw = _row(c, 0, p), _row(c, 1, p), _row(c, 3, p)
        su, sv = (hx / hw + F(1.0)) * F(0.5), (hy / hw + F(1.0)) * F(0.5)
        ok = valid & (su >= 0) & (su <= 1) & (sv >= 0) & (sv <= 1)  # NaN: a miss
        su, sv = np.where(ok, su, F(0)), np.where(ok, sv, F(0))
        vx, vy = np.floor(su * F(S.n)).astype(np.int64), np.floor(sv * F(S.n)).astype(np.int64)
        tx, ty = np.floor(su * F(S.V)).astype(np.int64) % S.ps, np.floor(sv * F(S.V)).astype(np.int64) % S.ps
    ok &= (vx <= S.n - 1) & (vy <= S.n - 1)
    vx, vy = np.minimum(vx, S.n - 1), np.minimum(vy, S.n - 1)
    wx, wy = wrap(vx, S.offs[cc, 0], S.n), wrap(vy, S.offs[cc, 1], S.n)
    e = S.table[cc, wy, wx].astype(np.int64)
    ok &= (e & BACKED) != 0
    addr = e >> 16
    ok &= addr < S.P * S.P
    addr = np.where(ok, addr, 0)
    return ok, (addr % S.P) * S.ps + tx, (addr // S.P) * S.ps + ty


def tap(S: Shape, ci, p):
    """sample_vsm_shadow_depth: (hit, depth)."""
    ok, X, Y = tap_address(S, ci, p)
    d = S.physical[Y, X]
    ok &= d != MISS
    return ok, np.where(ok, d, MISS)


def tap_with_fallback(S: Shape, base, p, stats=None):
    """base, base - 1, base + 1 in that order: (hit, depth)."""
    hit = np.zeros(base.shape, dtype=bool)
    depth = np.full(base.shape, MISS, dtype=np.float32)
    for t, delta in enumerate((0, -1, 1)):
        todo = np.flatnonzero(~hit)
        if todo.size == 0:
            break
        ok, d = tap(S, base[todo] + delta, tuple(v[todo] for v in p))
        hit[todo] = ok
        depth[todo] = d
        if stats is not None and t:
            stats["fallback_minus" if t == 1 else "fallback_plus"] += int(ok.sum())
    if stats is not None:
        stats["taps"] += int(base.size)
        stats["misses"] += int((~hit).sum())
    return hit, depth


# ---- rules 1-3 and 7 ------------------------------------------------------------------------------------------------------------------------
def resolve(depth, normal, table, clipmaps, physical, inv_pv, resolution, light_dir, z_length, *, page_size=128, page_table_size=64,
            physical_page_table_size=8192, clipmap_count=10, first_clipmap_width=10.0, bias=-1.5, virtual_extent=8192.0, stats: dict = None):
    """One oxc_resolve_shadowmap call: float32 [H, W].  `normal` is the uint16 / int16 [H, W, 4] image.  `stats` receives the tap counts
    (taps, misses = taps no clipmap served, fallback_minus / fallback_plus = taps served by base - 1 / base + 1) and `outcome`, the
    int8 [H, W] class of every pixel (SKY, HARD, NO_BLOCKER, ALL_BLOCKERS, PCF)."""
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    S = Shape(table, clipmaps, physical, page_size=page_size, page_table_size=page_table_size, physical_page_table_size=physical_page_table_size,
              clipmap_count=clipmap_count)
    st = {"taps": 0, "misses": 0, "fallback_minus": 0, "fallback_plus": 0}
    out = np.ones((H, W), dtype=np.float32)
    outcome = np.zeros((H, W), dtype=np.int8)
    ys, xs = np.nonzero(depth != F(0.0))  # (a NaN depth is not sky)
    if xs.size:
        with np.errstate(all="ignore"):
            res, oc = _pixels(S, st, depth[ys, xs], np.asarray(normal).reshape(H, W, 4)[ys, xs], xs, ys, W, H, np.asarray(inv_pv, dtype=np.float32),
                              np.asarray(resolution, dtype=np.float32), light_dir, F(z_length), first_clipmap_width, bias, virtual_extent)
        out[ys, xs] = res
        outcome[ys, xs] = oc
    if stats is not None:
        stats.update(st, outcome=outcome)
    return out


def _pixels(S, st, d, normal, xs, ys, W, H, inv_pv, resolution, light_dir, z_length, fcw, bias, vext):
    u = (xs.astype(np.float32) + F(0.5)) / F(W)
    v = (ys.astype(np.float32) + F(0.5)) / F(H)
    world = unproject(inv_pv, u, v, d)
    o = (F(1.0) / resolution) * F(0.5)
    lft = unproject(inv_pv, u + -o[0], v + o[1], d)
    rgt = unproject(inv_pv, u + o[0], v + o[1], d)
    dl = (lft[0] - rgt[0], lft[1] - rgt[1], lft[2] - rgt[2])
    tl = texel_length(S.n, fcw, vext)
    base = clipmap_index(length(dl) / tl, bias, S.count)
    N = decode_normal(normal)
    nx, ny = noise(xs, ys)
    # pcss_shadow
    L = tuple(F(c) for c in light_dir)
    T, B = perpendicular_basis(L)
    NoL = np.fmax(dot(N, L), F(0.0))
    cts = np.exp2(base + 1).astype(np.float32) * tl
    b = (SQRT2 * cts) * F(0.5)
    slope = (b * length(cross(N, L))) / np.fmax(NoL, F(0.1))
    base_bias = (QUANTIZE + b) + np.where(NoL < F(0.99), slope, b)
    inv_z = F(1.0) / z_length
    now = cts * (F(1.0) + F(2.0) * (F(1.0) - NoL))
    owp = tuple(world[k] + N[k] * now for k in range(3))
    c = S.mats[base]
    d_recv = _row(c, 2, owp) / _row(c, 3, owp)
    d_recv_world = d_recv * z_length
    c_hit, c_depth = tap_with_fallback(S, base, owp, st)

    def disc(i, count, n0, n1, radius):
        h = hammersley2d(i, count)
        xi0, xi1 = fract(h[0] + n0), fract(h[1] + n1)
        r = np.sqrt(xi0) * radius
        cs, sn = cos_sin_turn(xi1)
        p = tuple(owp[k] + r * (T[k] * cs + B[k] * sn) for k in range(3))
        pcf_bias = F(2.0) * r
        return p, inv_z * (base_bias + (pcf_bias + (F(0.0) - pcf_bias) * NoL))

    accum = np.zeros(d.shape, dtype=np.float32)
    blockers = np.zeros(d.shape, dtype=np.int64)
    valid = np.zeros(d.shape, dtype=np.int64)
    for i in range(BLOCKER_SAMPLES):
        p, bias_norm = disc(i, BLOCKER_SAMPLES, nx, ny, SEARCH_RADIUS)
        hit, dep = tap_with_fallback(S, base, p, st)
        valid += hit
        blk = hit & (dep + bias_norm < d_recv)
        accum = np.where(blk, accum + dep * z_length, accum)
        blockers += blk
    hard = np.where(c_hit & (c_depth + inv_z * base_bias < d_recv), F(0.0), F(1.0))
    res = hard.copy()
    oc = np.full(d.shape, HARD, dtype=np.int8)
    some = valid > 0
    res[some & (blockers == 0)] = 1.0
    oc[some & (blockers == 0)] = NO_BLOCKER
    res[some & (blockers == valid)] = 0.0
    oc[some & (blockers == valid)] = ALL_BLOCKERS
    pen = np.flatnonzero(some & (blockers > 0) & (blockers < valid))
    if pen.size:
        sub = lambda a: a[pen]  # noqa: E731
        d_blocker_world = accum[pen] / blockers[pen].astype(np.float32)
        pcf_radius = np.fmin(MAX_PCF_RADIUS, (d_recv_world[pen] - d_blocker_world) * LIGHT_WIDTH)
        owp, NoL, base_bias, base_p, d_recv_p = tuple(sub(a) for a in owp), NoL[pen], base_bias[pen], base[pen], d_recv[pen]
        nyx = (ny[pen], nx[pen])
        vis = np.zeros(pen.shape, dtype=np.float32)
        vpcf = np.zeros(pen.shape, dtype=np.int64)
        for i in range(PCF_SAMPLES):
            p, bias_norm = disc(i, PCF_SAMPLES, nyx[0], nyx[1], pcf_radius)
            hit, dep = tap_with_fallback(S, base_p, p, st)
            vpcf += hit
            vis = np.where(hit & (dep + bias_norm >= d_recv_p), vis + F(1.0), vis)
        ratio = vis / vpcf.astype(np.float32)
        res[pen] = np.where(vpcf > 0, ratio, hard[pen])
        oc[pen] = np.where(vpcf > 0, PCF, HARD)
    return res, oc


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def ortho_clipmaps(count: int, widths, offsets=None, z_range: float = 1.0) -> np.ndarray:
    """uint8 [count * 76] clipmap records of an axis-aligned orthographic light that shines along +z: clipmap c maps world
    x, y in [-widths[c] / 2, widths[c] / 2] to clip [-1, 1] and world z in [0, z_range] to depth [0, 1], w = 1."""
    rec = np.zeros((count, 19), dtype=np.float32)
    for c in range(count):
        m = np.zeros(16, np.float32)
        m[0] = m[5] = 2.0 / float(widths[c])
        m[10] = 1.0 / z_range
        m[15] = 1.0
        rec[c, :16] = m
        if offsets is not None:
            rec.view(np.int32)[c, 16:18] = offsets[c]
    return rec.view(np.uint8).reshape(-1).copy()


def encode_normal(n) -> np.ndarray:
    """uint16 [..., 4] texels whose .ba is vec3_to_oct(n) in binary16 (and .rg the same): n float32 [..., 3]."""
    n = np.asarray(n, dtype=np.float32)
    ex, ey = vec3_to_oct((n[..., 0], n[..., 1], n[..., 2]))
    h = np.stack([ex, ey, ex, ey], axis=-1).astype(np.float16)
    return h.view(np.uint16)
