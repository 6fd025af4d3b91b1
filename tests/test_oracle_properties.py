"""Property tests of the CPU oracle (hypothesis): invariants the reference's algorithms must satisfy whatever the
input, complementing the hand-derived known answers in test_oracle_kat.py / test_oracle_bounds.py / test_raster.py."""
import math

import numpy as np
import torch
from hypothesis import assume, given, settings, strategies as st

import oracle
from scenes import _coverage


def f32(x):
    return float(np.float32(x))


def floats32(lo, hi):
    return st.floats(min_value=f32(lo), max_value=f32(hi), width=32, allow_nan=False)


SMALL = floats32(-60000.0, 60000.0)


@settings(max_examples=300, deadline=None)
@given(SMALL, SMALL)
def test_quantize_half_is_monotone_and_close(a, b):
    lo, hi = (a, b) if a <= b else (b, a)
    dq = lambda h: float(oracle.lib().orc_dequantize_half(h))  # noqa: E731
    qa, qb = dq(oracle.quantize_half(lo)), dq(oracle.quantize_half(hi))
    assert qa <= qb
    for x, q in ((lo, qa), (hi, qb)):
        if abs(x) >= 2.0 ** -14:
            assert abs(q - x) <= abs(x) * 2.0 ** -11 + 1e-30   # half an ulp of an 11-bit significand
        else:
            assert q == 0.0                                    # flushed


@settings(max_examples=200, deadline=None)
@given(floats32(-1.0, 1.0))
def test_quantize_snorm_error_bound(v):
    q = oracle.quantize_snorm(v, 8)
    assert -127 <= q <= 127 and abs(q / 127.0 - v) <= 0.5 / 127.0 + 1e-6


IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
UNIT = floats32(-0.9, 0.9)
EXT = floats32(0.0, 0.19)


@settings(max_examples=300, deadline=None)
@given(UNIT, UNIT, floats32(0.1, 0.9), EXT, EXT, floats32(0.0, 0.19))
def test_frustum_keeps_boxes_inside_the_clip_volume(cx, cy, cz, ex, ey, ez):
    # identity mvp: the clip volume is |x| <= 1, |y| <= 1, 0 <= z <= 1 (planes r3+-r0, r3+-r1, r2, r3-r2)
    assert oracle.lib().orc_test_frustum(oracle._p(oracle.f32a(IDENTITY)), oracle._p(oracle.f32a([cx, cy, cz])), oracle._p(oracle.f32a([ex, ey, ez])))


@settings(max_examples=300, deadline=None)
@given(st.sampled_from([0, 1, 2]), st.booleans(), floats32(1.3, 50.0), UNIT, UNIT,
       floats32(0.0, 0.5))
def test_frustum_culls_boxes_wholly_beyond_a_plane(axis, negative, dist, u, v, extent):
    c = [u, v, 0.5]
    c[axis] = -dist if negative else dist
    if axis == 2 and negative:
        c[axis] = -dist + 1.0  # beyond z = 0 by more than the half extent
    m, cc, ee = oracle.f32a(IDENTITY), oracle.f32a(c), oracle.f32a([extent, extent, extent])
    assert not oracle.lib().orc_test_frustum(oracle._p(m), oracle._p(cc), oracle._p(ee))


@settings(max_examples=200, deadline=None)
@given(floats32(-30, 30), floats32(-30, 30), floats32(-900, -1.0),
       floats32(0.01, 1.5))
def test_project_aabb_contains_the_projected_centre(x, y, z, e):
    from oxylus_amd.synth import perspective_reversed_z

    pv = perspective_reversed_z(60.0, 1.0, 0.1, 1000.0).tolist()
    r = oracle.project_aabb(pv, 0.1, [x, y, z], [e, e, e])
    assert r is not None  # wholly in front of the near plane
    m = np.asarray(pv, dtype=np.float64).reshape(4, 4).T  # column-major -> [row][col]
    clip = m @ np.array([x, y, z, 1.0])
    u, v, d = clip[0] / clip[3] * 0.5 + 0.5, clip[1] / clip[3] * 0.5 + 0.5, clip[2] / clip[3]
    tol = 1e-4
    assert r[0] - tol <= u <= r[3] + tol and r[1] - tol <= v <= r[4] + tol and r[2] - tol <= d <= r[5] + tol
    assert r[0] <= r[3] and r[1] <= r[4] and 0.0 <= r[2] <= r[5] <= 1.0 + tol


@settings(max_examples=60, deadline=None)
@given(st.lists(st.tuples(st.integers(4, 59), st.integers(4, 59)), min_size=3, max_size=3, unique=True), st.integers(0, 2 ** 31 - 1))
def test_raster_fan_is_watertight(tri, seed):
    """A point inside a front-facing triangle splits it into three: together they cover exactly what the whole covers,
    no pixel twice (top-left rule on the shared edges)."""
    (ax, ay), (bx, by), (cx, cy) = tri
    area2 = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)
    if area2 == 0:
        return
    if area2 > 0:  # make it front facing (negative fixed-point area)
        (bx, by), (cx, cy) = (cx, cy), (bx, by)
    rng = np.random.default_rng(seed)
    w = rng.dirichlet([2.0, 2.0, 2.0])
    px = round(float(w[0] * ax + w[1] * bx + w[2] * cx) * 2) / 2  # half-pixel grid: exactly representable
    py = round(float(w[0] * ay + w[1] * by + w[2] * cy) * 2) / 2
    parts = [[(ax, ay), (bx, by), (px, py)], [(bx, by), (cx, cy), (px, py)], [(cx, cy), (ax, ay), (px, py)]]
    # the snapped point must still be strictly inside: all three parts keep the orientation of the whole
    orient = lambda t: (t[1][0] - t[0][0]) * (t[2][1] - t[0][1]) - (t[2][0] - t[0][0]) * (t[1][1] - t[0][1])  # noqa: E731
    assume(all(orient(t) < 0 for t in parts))
    whole, _ = _coverage([[(ax, ay), (bx, by), (cx, cy)]], 64, 64)
    cover = np.zeros((64, 64), dtype=np.int32)
    for t in parts:
        d, _ = _coverage([t], 64, 64)
        cover += (d > 0)
    assert cover.max() <= 1
    assert np.array_equal(cover > 0, whole > 0)
