"""The checker of oxc_contact_shadows (tests/contact_shadows_model.py) against answers worked out on paper from the rules in
include/oxcull.h, and the proof that the main GPU fixture is not degenerate, made with the checker alone (no GPU needed).

Most hand cases use identity matrices for inv_projection_view, view and projection: clip space is world space, a texel's value d is the
clip-space z of its surface and 1 / d its linear depth.  On a W x H image pixel x has cs.x = (x + 0.5) * 2 / W - 1 and cs_to_uv(cs.x) * W =
x + 0.5, all exact for W a power of two."""
import numpy as np
import pytest

import contact_shadows_model as CM
from scenes import CS_MAIN as MAIN
from scenes import CS_MAIN_SIZE as MAIN_SIZE
from scenes import CS_SUN as SUN
from scenes import I16
from scenes import cs_assert_not_degenerate as assert_not_degenerate
from scenes import identity_camera, main_frame_depth_from_the_oracle

F = np.float32


def plane(W, H, d):
    return np.full((H, W), d, dtype=np.float32)


def run(depth, sun=(1.0, 0.0, 0.0), steps=8, thickness=4.0, shadow_length=0.5, near=1.0, stats=None):
    return CM.contact_shadows(depth, I16, I16, I16, near, sun, steps, thickness, shadow_length, stats=stats)


def step_edge():
    """16 x 4: columns 0..7 hold 0.25 (linear depth 4, far), columns 8..15 hold 0.5 (linear depth 2, near)."""
    d = plane(16, 4, 0.25)
    d[:, 8:] = 0.5
    return d


# ---- constants ---------------------------------------------------------------------------------------------------------------------------
def test_the_two_binary32_constants():
    """2e-6 is 16.78 ulp(1.0) = 16.78 * 2^-23, so 1.0f + 0.000002f rounds to 1 + 17 * 2^-23.  0.3f = 0x99999A * 2^-25 has an even significand, so
    1 - 0.3f is a multiple of 2^-24 in [0.5, 1): exact, the binary32 number 0x3F333333."""
    assert CM.BIAS_SCALE.view(np.uint32) == 0x3F800011
    assert CM.EDGE_SPAN.view(np.uint32) == 0xBF333333


# ---- rule 7 ------------------------------------------------------------------------------------------------------------------------------
def test_smoothstep_at_its_edges_in_the_middle_and_beyond():
    """frac = 0.3f: (0.3f - 1) / (0.3f - 1) = 1 exactly, shadow = 1 * (3 - 2) = 1.  frac = 1: 0 / .. = 0, shadow 0.  Beyond: frac = 2 gives
    1 / -0.7 < 0, clamped to 0, shadow 0; frac = -1 gives -2 / -0.7 > 1, clamped to 1, shadow 1; frac = -Inf likewise.
    frac = 0.65f = 0x3F266666 = 0.649999976...: frac - 1 = -0.350000024 (exact); divided by -0.699999988 = 0.5000000426, which rounds to
    s = 0.5 + 2^-24 (ulp 2^-24 = 5.96e-8: 4.26e-8 is nearer to one ulp than to zero).  s * s = 0.25 + 2^-24 + 2^-48 -> 0.25 + 2^-24;
    3 - 2 s = 2 - 2^-23 (exact);  product = 0.5 + 3 * 2^-25 - 2^-47, just below the tie between 0.5 + 2^-24 and 0.5 + 2^-23: 0.5 + 2^-24."""
    assert CM.shadow_of(F(0.3)) == F(1.0)
    assert CM.shadow_of(F(1.0)) == F(0.0)
    assert CM.shadow_of(F(2.0)) == F(0.0)
    assert CM.shadow_of(F(-1.0)) == F(1.0)
    assert CM.shadow_of(F(-np.inf)) == F(1.0)
    assert CM.shadow_of(F(0.65)) == F(0.5) + F(2.0 ** -24)


# ---- rule 4 ------------------------------------------------------------------------------------------------------------------------------
def test_step_count_below_two_pixels_between_and_above_steps():
    n, cls = CM.step_count(np.array([0, 1, 2, 5, 8, 9, 4294967295]), 8)
    assert n.tolist() == [2, 2, 2, 5, 8, 8, 8]
    assert cls.tolist() == [CM.N_LOWER, CM.N_LOWER, CM.N_BETWEEN, CM.N_BETWEEN, CM.N_UPPER, CM.N_UPPER, CM.N_UPPER]
    n, cls = CM.step_count(np.array([0, 1, 2, 100]), 1)  # min(1, len) < 2: always the lower clamp
    assert n.tolist() == [2, 2, 2, 2] and cls.tolist() == [CM.N_LOWER] * 4
    n, cls = CM.step_count(np.array([1, 2, 3]), 2)
    assert n.tolist() == [2, 2, 2] and cls.tolist() == [CM.N_LOWER, CM.N_UPPER, CM.N_UPPER]


def test_ray_length_in_pixels():
    """16 x 8: start (0, 0), end (0.375, 0.5) in clip space: uv delta (0.1875, 0.25), pixels (3, 2), length sqrt(13) = 3.6 -> 3.  A NaN
    length converts to 0, a huge one saturates."""
    z = F(0.5)
    assert int(CM.ray_length_u32((F(0), F(0), z), (F(0.375), F(0.5), z), 16, 8)) == 3
    assert int(CM.ray_length_u32((F(np.nan), F(0), z), (F(0.375), F(0.5), z), 16, 8)) == 0
    assert int(CM.ray_length_u32((F(-3e38), F(0), z), (F(3e38), F(0), z), 16, 8)) == 4294967295


# ---- rule 3 ------------------------------------------------------------------------------------------------------------------------------
def test_clip_with_a_zero_delta_of_either_sign():
    """cs = (0, 0, 0.5), end = (0.5, 0, 0.5): delta.y = delta.z = +0.  Start clip: x: (-1 - 0) / 0.5 = -2; y: (-1 - 0) / +0 = -Inf; m = -2, max(0, m) =
    0: start = cs.  End clip: (1 - 0) / 0.5 = 2, (1 - 0) / +0 = +Inf, (1 - 0.5) / +0 = +Inf: clip = min(1, 2) = 1, ray_end = end.
    end.x = -0.0 against cs.x = +0.0: delta.x = -0.0; -0 < 0 is false, near_edge.x = -1, (-1 - 0) / -0 = +Inf = m; start.x = 0 + -0 * Inf = NaN,
    start.y = 0 + 0.25 * Inf = Inf, start.z = 0.5 + 0 * Inf = NaN."""
    z = F(0.0)
    start, end, clip, moved = CM.clip_ray((z, z, F(0.5)), (F(0.5), z, F(0.5)))
    assert [float(v) for v in start] == [0.0, 0.0, 0.5] and [float(v) for v in end] == [0.5, 0.0, 0.5] and clip == 1.0 and moved == 0.0
    with np.errstate(all="ignore"):
        start, end, clip, moved = CM.clip_ray((z, z, F(0.5)), (F(-0.0), F(0.25), F(0.5)))
    assert moved == np.inf and np.isnan(start[0]) and start[1] == np.inf and np.isnan(start[2])


def test_a_ray_that_leaves_the_image_is_cut_at_the_border():
    """cs = (0.5625, 0, 0.25) (pixel 12 of 16), end.x = 1.0625: q.x = (1 - 0.5625) / 0.5 = 0.875 < 1, ray_end.x = 0.5625 + 0.5 * 0.875 = 1.0.  Towards
    the far plane: cs.z = 0.25, end.z = -0.25: far_edge.z = 0, q.z = (0 - 0.25) / -0.5 = 0.5, ray_end.z = 0."""
    z = F(0.0)
    start, end, clip, _ = CM.clip_ray((F(0.5625), z, F(0.25)), (F(1.0625), z, F(0.25)))
    assert clip == F(0.875) and end[0] == F(1.0) and start[0] == F(0.5625)
    start, end, clip, _ = CM.clip_ray((z, z, F(0.25)), (z, z, F(-0.25)))
    assert clip == F(0.5) and end[2] == F(0.0)


# ---- rule 6 ------------------------------------------------------------------------------------------------------------------------------
def test_the_four_texel_clamp_at_every_edge_and_corner():
    """4 x 3 image.  interp_uv * size = 0.25: g = -0.25, i = -1, f = 0.75: columns clamp(-1), clamp(0) = 0, 0.  = 3.75 (W = 4): g = 3.25, i = 3:
    columns 3, clamp(4) = 3.  Inside, 1.5: g = 1.0, i = 1, f = 0: columns 1, 2.  Rows likewise with H = 3."""
    d = np.arange(12, dtype=np.float32).reshape(3, 4) + F(1.0)
    lo, mid, hix, hiy = F(0.25), F(1.5), F(3.75), F(2.75)
    cases = {(lo, lo): (0, 0, 0, 0, 0, 0), (hix, lo): (3, 3, 0, 0, 3, 0), (lo, hiy): (0, 0, 2, 2, 0, 2), (hix, hiy): (3, 3, 2, 2, 3, 2),
             (mid, lo): (1, 2, 0, 0, 1, 0), (mid, hiy): (1, 2, 2, 2, 1, 2), (lo, mid): (0, 0, 1, 2, 0, 1), (hix, mid): (3, 3, 1, 2, 3, 1),
             (mid, mid): (1, 2, 1, 2, 1, 1)}
    for (ux, uy), want in cases.items():
        lin, unf, coords = CM.tap(d, np.array([ux]), np.array([uy]))
        assert tuple(int(c[0]) for c in coords) == want, (ux, uy)
        assert unf[0] == F(1.0) / d[want[5], want[4]]
    # a corner reads one texel four times: the bilinear is that texel
    lin, _, _ = CM.tap(d, np.array([hix]), np.array([hiy]))
    assert lin[0] == F(1.0) / F(12.0)
    # at (1.75, 1.5): f = (0.25, 0): lerp(d[1][1], d[1][2], 0.25) = 6 + 0.25 = 6.25
    lin, _, _ = CM.tap(d, np.array([F(1.75)]), np.array([mid]))
    assert lin[0] == F(1.0) / F(6.25)
    # NaN -> i = 0 (texels 0 and 1, nearest 0); beyond the i32 range -> saturated, then clamped; i = INT_MAX does not wrap
    with np.errstate(all="ignore"):
        _, _, c = CM.tap(d, np.array([F(np.nan), F(1e20), F(-1e20), F(np.inf)]), np.array([mid] * 4))
    assert [int(v) for v in c[0]] == [0, 3, 0, 3] and [int(v) for v in c[1]] == [1, 3, 0, 3] and [int(v) for v in c[4]] == [0, 3, 0, 3]


# ---- whole images --------------------------------------------------------------------------------------------------------------------------
def test_a_flat_plane_facing_the_camera_has_no_shadow():
    """Every texel 0.5.  A ray along the plane stays at linear depth 2 and meets max_depth * (1 + 17 * 2^-23) = 2.000004 > 2: distance > 0 at every
    tap.  A ray towards the camera (z rising) has ray_depth < 2.  Through a perspective camera: the same."""
    for sun in ((1, 0, 0), (0, 1, 0), (-1, -1, 0), (0.6, 0, 0.8)):
        st = {}
        img = run(plane(16, 8, 0.5), sun=sun, stats=st)
        assert (img == 1.0).all() and (st["outcome"] == CM.MISS).all()
    from oxylus_amd.synth import perspective_reversed_z

    proj = perspective_reversed_z(60.0, 1.0, 0.1, 1000.0).numpy()
    inv = np.linalg.inv(proj.astype(np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    img = CM.contact_shadows(plane(32, 32, 0.01), inv, I16, proj, 0.1, (0.3, 0.8, 0.5), 8, 0.1, 1.0)
    assert (img == 1.0).all()


def test_a_step_edge_with_the_sun_across_it():
    """step_edge(), sun (1, 0, 0), shadow_length 0.5 = 4 pixels, steps 8: n = min(8, 4) = 4, t = 1/4 .. 1, taps at x + 1 .. x + 4, each exactly on a
    texel centre (f = 0: bilinear == nearest == that texel).  A pixel of the far half (ray_depth 1 / 0.25 = 4) intersects at its first tap in
    the near half (max_depth 2: distance = 2.000004 - 4 < 0): columns 4..7, after 4, 3, 2, 1 taps.  penetration = 4 - 2 = 2.
    thickness 4 (near 1): frac = 0.5, s = (0.5 - 1) / -0.7 = 5 / 7, shadow = (25 / 49) (3 - 10 / 7) = 275 / 343, pixel = 68 / 343 = 0.19825.
    Four roundings of at most 2^-24 each on values <= 1, and the edge constant off by 1.2e-8: within 5e-7.
    thickness 2: penetration < 2 fails: intersected, rejected, 1.0.  thickness 1000: frac = 0.002, s clamps to 1, shadow 1, pixel exactly 0.0.
    Columns 12..15: the ray leaves the image, end clip active, n = floor(3.5, 2.5, 1.5, 0.5 px) -> 3, 2, 2 (lower clamp), 2 (lower clamp).
    The near half marches at ray_depth 2 over texels of linear depth 2: no intersection."""
    st = {}
    img = run(step_edge(), thickness=4.0, stats=st)
    want = np.ones((4, 16), dtype=np.float32)
    shadowed = img[:, 4:8]
    assert np.array_equal(np.delete(img, np.s_[4:8], axis=1), np.delete(want, np.s_[4:8], axis=1))
    assert (np.abs(shadowed.astype(np.float64) - 68.0 / 343.0) < 5e-7).all() and ((shadowed > 0) & (shadowed < 1)).all()
    assert st["taps"][0].tolist() == [4, 4, 4, 4, 4, 3, 2, 1, 4, 4, 4, 4, 3, 2, 2, 2]
    assert st["n"][0].tolist() == [4] * 12 + [3, 2, 2, 2]
    assert st["n_class"][0].tolist() == [CM.N_BETWEEN] * 14 + [CM.N_LOWER] * 2
    assert st["end_clip"][0].tolist() == [False] * 12 + [True] * 4
    assert (st["outcome"][:, 4:8] == CM.HIT_PARTIAL).all() and (st["outcome"][:, :4] == CM.MISS).all() and not st["start_moved"].any()
    st = {}
    assert (run(step_edge(), thickness=2.0, stats=st) == 1.0).all() and (st["outcome"][:, 4:8] == CM.REJECTED).all()
    st = {}
    img = run(step_edge(), thickness=1000.0, stats=st)
    assert (img[:, 4:8] == 0.0).all() and (st["outcome"][:, 4:8] == CM.HIT_ZERO).all() and (np.delete(img, np.s_[4:8], axis=1) == 1.0).all()
    c = CM.counters(st)
    assert c["non_sky_pixels"] == 64 and c["taps"] == 4 * 51 and c["hit_zero"] == 16 and c["miss"] == 48 and c["end_clip"] == 16
    # steps above and below the ray's length: 3 steps -> taps at x + 4/3, 8/3, 4; columns 4..7 still find the near half
    st = {}
    img = run(step_edge(), steps=3, thickness=1000.0, stats=st)
    assert st["n"][0, :12].tolist() == [3] * 12 and (st["n_class"][0, :12] == CM.N_UPPER).all() and (img[:, 6:8] == 0.0).all()


def test_sky_pixels_and_a_nan_depth():
    """depth +0.0 and -0.0 are sky: 1.0, no tap.  A NaN depth is not sky: e.z = NaN, sign(NaN) = 0, so the ray collapses onto its start
    (end = cs + (e - cs) * 0; the z components are NaN): length 0, n = 2 by the lower clamp, two taps whose ray_depth and distance are NaN: no
    intersection, 1.0."""
    d = step_edge()
    d[0, 5], d[1, 5], d[2, 5] = 0.0, -0.0, np.nan
    st = {}
    img = run(d, thickness=1000.0, stats=st)
    assert img[0, 5] == 1.0 and img[1, 5] == 1.0 and img[2, 5] == 1.0 and img[3, 5] == 0.0
    assert st["outcome"][:3, 5].tolist() == [CM.SKY, CM.SKY, CM.MISS] and st["taps"][:3, 5].tolist() == [0, 0, 2] and st["n_class"][2, 5] == CM.N_LOWER


@pytest.mark.parametrize("value,want", [(np.inf, 68.0 / 343.0), (-0.5, 243.0 / 343.0), (np.nan, 1.0), (-np.inf, None), (1e-42, 1.0)])
def test_non_finite_negative_and_denormal_texels(value, want):
    """16 x 3 plane of 0.25 (ray_depth 4), one texel at (row 1, column 9) replaced, sun (1, 0, 0), 4 pixels, thickness 8 (dt = 8).  A tap on
    that texel has f = 0, so the bilinear is t00 + (t10 - t00) * 0 + ...:
    +Inf: (0.25 - Inf) * 0 = NaN, linear_depth NaN; unfiltered = 1 / Inf = 0; max and min drop the NaN: max_depth = min_depth = 0: distance = -4,
          penetration 4, frac 0.5: the pixels 5..8 of row 1 are 68 / 343 (as the step edge).  An infinitely near occluder shadows.
    -0.5: linear = unfiltered = -2: distance = -2.000004 - 4 < 0, penetration 6, frac 0.75: s = 0.25 / 0.7 = 5 / 14, shadow = (25 / 196)(16 / 7) =
          100 / 343, pixel 243 / 343.
    NaN:  both depths NaN, distance NaN: never an intersection.  A neighbouring tap that weighs the NaN with 0 has a NaN bilinear and
          falls back on its nearest texel through max / min: the plane, no intersection.  All 1.0.
    -Inf: 1 / -Inf = -0: max_depth = -0, distance = -4 < 0, penetration = 4 - -0 = 4: as +Inf.
    1e-42 (denormal): linear depth 1 / 1e-42 is far beyond the ray: distance > 0.  All 1.0.
    The pixel at (1, 9) itself marches from cs.z = the value: Inf / NaN give NaN taps (1.0); -0.5 is behind the far plane: end.z = -0.5,
    ray_depth = -2 against the plane's 4: distance > 0 (1.0); 1e-42: ray_depth 1e42 -> Inf, penetration Inf: rejected (1.0).
    Every result is finite."""
    d = plane(16, 3, 0.25)
    d[1, 9] = value
    with np.errstate(all="ignore"):
        img = run(d, thickness=8.0)
    assert np.isfinite(img).all() and (img >= 0).all() and (img <= 1).all()
    expect = np.ones((3, 16))
    if want is None:
        want = 68.0 / 343.0
    expect[1, 5:9] = want
    assert (np.abs(img.astype(np.float64) - expect) < 5e-7).all(), img
    if want == 1.0:
        assert (img == 1.0).all()


def test_a_rotated_view_is_the_same_frame_with_the_sun_rotated():
    """view = R, a quarter turn about y (entries 0 and +-1, no translation): view space (x, y, z) = (world.z, world.y, -world.x).  Every product
    with such a matrix is exact and every row sum has the same non-zero terms, so the frame with (view R, sun s) is byte for byte the frame
    with (view I, sun R s).  s = (0.6, 0.8, 0) -> R s = (0, 0.8, -0.6): the normalisation adds the same two squares."""
    from oxylus_amd.synth import make_depth, perspective_reversed_z

    proj = perspective_reversed_z(60.0, 1.0, 0.1, 1000.0).numpy()
    invp = np.linalg.inv(proj.astype(np.float64).reshape(4, 4).T).astype(np.float32)  # row-major M
    R = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
    inv_rot = (R.T @ invp).astype(np.float32)  # exact: a signed permutation of rows
    depth = make_depth(96, 64, 12, seed=3).numpy()
    st = {}
    a = CM.contact_shadows(depth, inv_rot.T.reshape(-1), R.T.reshape(-1), proj, 0.1, (0.6, 0.8, 0.0), 8, 0.5, 1.0, stats=st)
    b = CM.contact_shadows(depth, invp.T.reshape(-1), I16, proj, 0.1, (0.0, 0.8, -0.6), 8, 0.5, 1.0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (a < 1.0).sum() > 20 and (st["outcome"] == CM.MISS).sum() > 20
    c = CM.contact_shadows(depth, invp.T.reshape(-1), I16, proj, 0.1, (0.6, 0.8, 0.0), 8, 0.5, 1.0)
    assert not np.array_equal(a, c)  # and the rotation matters


# ---- the GPU fixture is not degenerate -------------------------------------------------------------------------------------------------------


def test_the_main_gpu_frame_is_not_degenerate():
    """The frame tests/test_gpu_contact_shadows.py compares byte for byte -- occluder_scene(61) at 768 x 768, the sun of the resolve tests,
    steps 12, thickness 0.3, shadow_length 0.15 -- judged by the checker alone on the oracle's depth image: every outcome class holds at
    least 1000 pixels and the end clip at least 100 (no floor had to be lowered).  Reached: sky 267 518, miss 243 076, hit == 0.0 51 106, hit inside
    (0, 1) 22 239, intersected but rejected 5 885, n == 2 by the lower clamp 7 522, 2 <= n < steps 228 162, n == steps 86 622, end clip active
    5 893; 2 132 799 taps.  (A hit that writes 1.0 and a moved start do not occur on it.)"""
    s, depth = main_frame_depth_from_the_oracle()
    inv, view, proj, near = identity_camera(s)
    st = {}
    img = CM.contact_shadows(depth, inv, view, proj, near, SUN, stats=st, **MAIN)
    c = assert_not_degenerate(st)
    print(c)
    assert c["non_sky_pixels"] + c["sky"] == MAIN_SIZE * MAIN_SIZE
    assert c["miss"] + c["hit_zero"] + c["hit_partial"] + c["hit_one"] + c["rejected"] == c["non_sky_pixels"] == c["n_lower"] + c["n_between"] + c["n_upper"]
    assert int(((img > 0) & (img < 1)).sum()) == c["hit_partial"] and int((img == 0).sum()) == c["hit_zero"]
