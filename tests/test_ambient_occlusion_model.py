"""The checker of oxc_generate_ambient_occlusion (tests/ambient_occlusion_model.py) against answers worked out on paper from the rules in
include/oxcull.h, the error bounds of its log2 and pow rules, the Hilbert table, and the proof that the main GPU fixture is not degenerate,
made with the checker alone (no GPU needed)."""
import math

import numpy as np
import pytest

import ambient_occlusion_model as AM
import vsm_resolve_model as RM
from scenes import AO_MAIN as MAIN
from scenes import AO_MAIN_SIZE as MAIN_SIZE
from scenes import I16, PROJ
from scenes import ao_assert_not_degenerate as assert_not_degenerate
from scenes import ao_main_frame_inputs as main_frame_inputs
from scenes import flat_normals, hilbert, pit_image

F = np.float32


# ---- prefilter -----------------------------------------------------------------------------------------------------------------------------
def test_weighted_average_of_equal_depths_and_of_a_saturated_outlier():
    """Four equal depths d: every d_i - min is 0, every weight is saturate(falloff_add) = 1 (falloff_add = 0.385 / 0.615 + 1 > 1), the sum is
    ((d + d) + d) + d = 4 d exactly and the quotient d.  One outlier at 3 + 100: its weight is saturate(100 * falloff_mul + falloff_add) with
    falloff_mul = -1 / (0.615 * 0.546375) = -2.976..., far below 0, so 0: the result is (3 + 3 + 3 + 0 * 103) / 3 = 3."""
    assert AM.weighted_average(F(7.25), F(7.25), F(7.25), F(7.25)) == F(7.25)
    assert AM.weighted_average(F(3), F(3), F(103), F(3)) == F(3)
    mul, add = AM.falloff_constants(AM.PREFILTER_RADIUS)
    assert AM.PREFILTER_RADIUS == F(F(0.375) * F(1.457)) and mul < -2.9 and add > 1.0


def test_prefilter_gather_mapping_on_a_4_by_2_image():
    """mul = 1, add = 0: linear = 1 / depth.  Depths 1 / (1 .. 8) row by row: level 0 is 1..8 at their own places; thread (0, 0) averages texels
    (0,0) (1,0) (0,1) (1,1) = 1, 2, 5, 6 in the order .w .z .x .y; min 1, weights saturate((d - 1) * mul + add): with mul = -2.976, add = 1.626
    d = 1 -> 1, d = 2 -> saturate(-1.35) = 0, so the result is 1 / 1; thread (1, 0) likewise gives 3."""
    depth = (F(1.0) / np.arange(1, 9, dtype=np.float32)).reshape(2, 4)
    lv = AM.prefilter(depth, PROJ)
    assert [l.shape for l in lv] == [(2, 4), (1, 2), (1, 1), (1, 1), (1, 1)]
    assert np.allclose(lv[0], np.arange(1, 9).reshape(2, 4), rtol=1e-6)
    assert lv[1][0, 0] == lv[0][0, 0] and lv[1][0, 1] == lv[0][0, 2]


def test_prefilter_edge_clamp_and_all_five_extents_on_5_by_3():
    """5 x 3, constant depth 0.5 (linear 2): levels are 5x3, 2x1, 1x1, 1x1, 1x1.  Thread (2, *) gathers columns 4 and 5 -> 4 (clamped), thread
    (*, 1) rows 2 and 3 -> 2; their mip-0 stores at x = 5 or y = 3 are dropped, their mip-1 destinations (2, *), (*, 1) lie outside 2 x 1.  All
    values are 2, so every level is 2.  With column 4 set to linear 4 only level 0 changes inside levels 0..1 (mip 1's texels come from columns
    0..3); level 2's texel averages THREADS (0..1, 0..1), which read rows 0..2 (row 3 clamps to 2) of columns 0..3: still 2."""
    depth = np.full((3, 5), 0.5, dtype=np.float32)
    lv = AM.prefilter(depth, PROJ)
    assert [l.shape for l in lv] == [(3, 5), (1, 2), (1, 1), (1, 1), (1, 1)]
    assert all((l == 2).all() for l in lv)
    depth[:, 4] = 0.25
    lv = AM.prefilter(depth, PROJ)
    assert (lv[0][:, 4] == 4).all() and (lv[0][:, :4] == 2).all() and (lv[1] == 2).all() and lv[2][0, 0] == 2
    # levels 3 and 4 fold thread (2, *), which holds the column-4 value 4: min 2, the weight of 4 is saturate((4 - 2) * -2.976 + 1.626) = 0
    assert lv[3][0, 0] == 2 and lv[4][0, 0] == 2


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_calculate_edges_constant_depth_and_planar_slope():
    """Constant depth: every difference is 0, 1.25 - 0 saturates to 1, byte 255 four times: 0xFFFFFFFF.  A plane d = 10 + x: left = -1, right
    = +1, slope_left_right = 1, adjusted left = -1 + 1 = 0, adjusted right = 1 - 1 = 0: min(|e|, |adj|) = 0 -- the slope adjustment cancels it;
    also at the clamped border column 0, where left = 0, right = 1, slope 0.5: adjusted (0.5, 0.5), min(|0|, 0.5) = 0 for left and 0.5 for
    right: 1.25 - 0.5 / (10 * 0.011) < 0 -> byte 0 in component y."""
    lvl = np.full((4, 6), 10.0, dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(4), np.arange(6), indexing="ij")
    e, c = AM.calculate_edges(lvl, xs, ys)
    assert (e == 0xFFFFFFFF).all() and (c == 10).all()
    lvl = (F(10.0) + np.arange(6, dtype=np.float32))[None, :].repeat(4, 0)
    e, _ = AM.calculate_edges(lvl, xs, ys)
    assert (e[:, 1:5] == 0xFFFFFFFF).all()
    assert (e[:, 0] == 0xFFFF00FF).all()


def test_pack_and_unpack_rounding_at_the_half_way_points():
    """x * 255 + 0.5 then floor: 0.5 / 255 (binary32) times 255 is 0.5 exactly or a hair off; the values k + 0.5 themselves: x = 1.5 / 255 rounds
    in binary32 so that x * 255 = 1.5 -> floor(2.0) = 2 (a half-way value rounds up).  Exact cases: 0 -> 0, 1 -> 255, 2 -> 255, -1 -> 0, NaN ->
    0, 0.5 -> floor(127.5 + 0.5) = 128.  Component x sits in the low byte.  unpack: byte / 255."""
    p = AM.pack_unorm4x8(F(0.5), F(1.0), F(0.0), F(np.nan))
    assert int(p) == 0x0000FF80
    assert int(AM.pack_unorm4x8(F(2.0), F(-1.0), F(1.0) / F(255.0), F(0.25))) == (64 << 24) | (1 << 16) | 0xFF  # 0.25 * 255 + 0.5 = 64.25
    u = AM.unpack_unorm4x8(np.uint32(0xFF800100))
    assert u[0] == 0 and u[1] == F(1.0) / F(255.0) and u[2] == F(128.0) / F(255.0) and u[3] == 1


# ---- sectors -------------------------------------------------------------------------------------------------------------------------------
def test_update_sectors_zero_width_full_width_and_start_31():
    m, z = AM.update_sectors(F(0.3), F(0.3))
    assert int(m) == 0 and bool(z)
    m, z = AM.update_sectors(F(0.7), F(0.2))  # negative width saturates to 0
    assert int(m) == 0 and bool(z)
    m, z = AM.update_sectors(F(0.0), F(1.0))  # ceil(32) = 32 bits from 0
    assert int(m) == 0xFFFFFFFF and not bool(z)
    m, z = AM.update_sectors(F(1.0), F(2.0))  # start = min(32, 31) = 31, width saturate(1) -> 32 bits shifted out but one
    assert int(m) == 0x80000000
    m, _ = AM.update_sectors(F(0.25), F(0.25) + F(1.0 / 64.0))  # half a sector still touches one: ceil(0.5) = 1 bit at 8
    assert int(m) == 1 << 8


def test_fast_acos_at_minus_one_zero_and_one():
    """x = 1: sqrt(saturate(0)) = 0, res = 0.  x = 0: res = HALF_PI * 1.  x = -1: PI - 0 = PI."""
    assert AM.fast_acos(F(1.0)) == 0 and AM.fast_acos(F(0.0)) == AM.HALF_PI and AM.fast_acos(F(-1.0)) == AM.PI
    assert np.isnan(AM.fast_acos(F(np.nan)))


def test_noise_pair_of_a_table_entry():
    """Entry 0, noise_index 0: frac(0.5 + 0) = 0.5 both.  Entry 3, noise_index 65 (= 1 mod 64): index 3 + 288 = 291; 291 * 0.75487767 =
    219.669..., + 0.5 -> frac 0.169...; the binary32 steps are spelled out below."""
    a, b = AM.noise_pair(np.uint16(0), 0)
    assert a == F(0.5) and b == F(0.5)
    a, b = AM.noise_pair(np.uint16(3), 65)
    ta = F(0.5) + F(291.0) * F(0.75487766624669276005)
    tb = F(0.5) + F(291.0) * F(0.5698402909980532659114)
    assert a == ta - np.floor(ta) and b == tb - np.floor(tb) and abs(float(a) - 0.1694) < 1e-3


# ---- halves --------------------------------------------------------------------------------------------------------------------------------
def test_half_rounding_and_half_denormals_on_the_stores():
    """1 + 2^-11 is half-way between the halves 1 and 1 + 2^-10: ties to even give 1 (0x3C00); 1 + 3 * 2^-11 ties to 1 + 2^-9 (0x3C02).
    2^-24 is the smallest half denormal (0x0001); 2^-25 is half-way to 0 and ties to even 0; 1.5 * 2^-24 ties to 2 * 2^-24."""
    assert AM.to_half_bits(F(1.0) + F(2.0 ** -11)) == 0x3C00
    assert AM.to_half_bits(F(1.0) + F(3 * 2.0 ** -11)) == 0x3C02
    assert AM.to_half_bits(F(2.0 ** -24)) == 0x0001 and AM.to_half_bits(F(2.0 ** -25)) == 0 and AM.to_half_bits(F(1.5 * 2.0 ** -24)) == 0x0002
    assert AM.from_half_bits(np.uint16(0x0001)) == F(2.0 ** -24)


# ---- log2, pow, rotation -------------------------------------------------------------------------------------------------------------------
def test_log2_rule_error_bound_and_special_values():
    """Against math.log2 over the arguments the pass can produce (pixel lengths from 2^-20 to 2^20 and the whole normal range at the ends):
    the binary64 evaluation is good to 1e-15, so the binary32 result is the correctly rounded one or its neighbour: |err| <= 2^-23 * max(|exact|,
    2^-1)."""
    rng = np.random.default_rng(5)
    x = np.concatenate([np.exp2(rng.uniform(-20, 20, 100000)), np.exp2(rng.uniform(-126, 127.9, 20000)), [1.0, 1.4142135, 1.4142137, 2.0, 0.5]]).astype(np.float32)
    got = AM.log2_rule(x).astype(np.float64)
    want = np.array([math.log2(float(v)) for v in x])
    assert (np.abs(got - want) <= 2.0 ** -23 * np.maximum(np.abs(want), 0.5)).all()
    assert AM.log2_rule(F(1.0)) == 0 and AM.log2_rule(F(8.0)) == 3 and AM.log2_rule(F(0.25)) == -2
    for bad in (0.0, -0.0, -1.0, np.nan, 1e-40, -np.inf):
        assert AM.log2_rule(F(bad)) == -np.inf
    assert AM.log2_rule(F(np.inf)) == np.inf


def test_pow_rule_error_bound_zero_one_and_identity():
    """Against math.pow for v in [0, 1] and the powers the engine can set: within 2^-23 relative plus half a binary32 denormal.  pow(0) = 0,
    pow(1) = 1 exactly, and final_power = 1.0 returns v itself."""
    rng = np.random.default_rng(6)
    v = np.concatenate([rng.uniform(0, 1, 50000), np.exp2(rng.uniform(-24, 0, 50000))]).astype(np.float32)
    for p in (0.5, 1.0, 2.2, 3.0, 8.0):
        got = AM.pow_rule(v, p).astype(np.float64)
        want = np.array([math.pow(float(x), float(F(p))) for x in v])
        assert (np.abs(got - want) <= 2.0 ** -23 * want + 2.0 ** -150).all(), p
    assert (AM.pow_rule(v, 1.0) == v).all()
    for p in (0.5, 2.2, 100.0):
        assert AM.pow_rule(F(0.0), p) == 0 and AM.pow_rule(F(1.0), p) == 1
    assert AM.pow_rule(F(0.5), 1000.0) == 0 and AM.pow_rule(F(2.0), 1000.0) == np.inf


def test_the_slice_rotation_is_the_resolves_function():
    assert AM.cos_sin_turn is RM.cos_sin_turn
    c, s = AM.cos_sin_turn(F(0.25) * F(0.5))  # slice 0.25: phi = pi / 4
    assert abs(float(c) - math.sqrt(0.5)) < 2 ** -23 and abs(float(s) - math.sqrt(0.5)) < 2 ** -23


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def test_hilbert_noise_lut_is_a_hilbert_walk():
    t = hilbert().astype(np.int64)
    assert t.shape == (64, 64) and sorted(t.reshape(-1).tolist()) == list(range(4096))
    pos = np.zeros((4096, 2), dtype=np.int64)
    ys, xs = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    pos[t.reshape(-1)] = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
    assert (np.abs(np.diff(pos, axis=0)).sum(axis=1) == 1).all()  # consecutive indices are 4-neighbours
    assert t[0, 0] == 0


# ---- whole pixels --------------------------------------------------------------------------------------------------------------------------
def run(depth, normal=None, proj=PROJ, far=100.0, **kw):
    H, W = depth.shape
    normal = flat_normals(H, W) if normal is None else normal
    st = {}
    out = AM.generate(depth, normal, hilbert(), I16, proj, (W, H), far, stats=st, **kw)
    return out, st


def test_a_sky_pixel_is_one_and_still_writes_depth_differences():
    """linear = 1 / depth: depth 0.005 is linear 200 >= 100 * 0.999: sky.  Everything sky: noisy and final are 1.0 (0x3C00; pow(1) = 1), the edges
    of a constant image 0xFFFFFFFF.  One sky pixel inside a near plane still gets its edge word (all four differences huge: 0)."""
    out, st = run(np.full((8, 8), 0.005, dtype=np.float32))
    assert (out["noisy_occlusion"] == 0x3C00).all() and (out["ambient_occlusion"] == 0x3C00).all() and (out["depth_differences"] == 0xFFFFFFFF).all()
    assert AM.counters(st)["non_sky_pixels"] == 0
    d = np.full((8, 8), 0.5, dtype=np.float32)
    d[3, 4] = 0.005
    out, st = run(d)
    assert out["noisy_occlusion"][3, 4] == 0x3C00 and out["depth_differences"][3, 4] == 0 and AM.counters(st)["non_sky_pixels"] == 63


def test_denoise_of_a_constant_image_with_all_edges_open():
    """All edges 1: the side weights are 1, the diagonal ones 0.425 * 2 = 0.85; sum_weight = 1.2 + 4 + 3.4 = 8.6 (in binary32, step by step) and
    sum = v * each: with v = 1 the quotient is exactly 1 and pow(1) = 1.  With v = 0.5 the sum is half of sum_weight exactly (scaling by a power
    of two commutes with every rounding), the quotient 0.5, and final_power = 1 keeps it: the half 0x3800."""
    edges = np.full((5, 7), 0xFFFFFFFF, dtype=np.uint32)
    assert (AM.denoise(np.full((5, 7), 0x3C00, dtype=np.uint16), edges, 2.2) == 0x3C00).all()
    assert (AM.denoise(np.full((5, 7), 0x3800, dtype=np.uint16), edges, 1.0) == 0x3800).all()
    assert (AM.denoise(np.full((5, 7), 0x3800, dtype=np.uint16), edges, 2.0) == 0x3400).all()  # 0.25


def test_a_fully_occluded_pixel_is_exactly_zero():
    """The class the drawn scene cannot produce.  From the bottom of the pit every sample (at least 1.3 pixels away, and the pit's weight in
    the upper mips is 0) lands hundreds of units nearer to the camera and at most a few units to the side: the front horizon is within 0.01 of
    0, the back face 10^6 units behind it puts the back horizon at PI, n = 0.  Side +1: lo = saturate(-0.5) = 0, hi = 0.5 - eps: ceil(16 - eps')
    = 16 sectors from 0.  Side -1: lo = 0.5 + eps: start 16, hi = saturate(1.5) = 1: 16 sectors from 16.  |delta| < 1000 < 0.385 * 2914: falloff 1.
    occlusion = 16 / 32 + 16 / 32 = 1 after the first pair of every slice, visibility 0, the half 0x0000, pow(0) = 0."""
    d, kw = pit_image()
    out, st = run(d, **kw)
    assert out["noisy_occlusion"][16, 16] == 0 and out["ambient_occlusion"][16, 16] < 0x3C00
    assert AM.counters(st)["result_zero"] >= 1


def test_non_finite_texels_and_normals_stay_finite_in_the_output():
    rng = np.random.default_rng(9)
    d = rng.uniform(0.05, 0.5, (24, 40)).astype(np.float32)
    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42, -0.5, 0.0, 3e38], dtype=np.float32)
    d.reshape(-1)[::7] = vals[np.arange(len(d.reshape(-1)[::7])) % len(vals)]
    n = flat_normals(24, 40).copy()
    n.reshape(-1, 4)[::5, 2] = np.array([0x7E00, 0x7C00, 0x0001, 0xFC00], dtype=np.uint16)[np.arange(len(n.reshape(-1, 4)[::5])) % 4]
    out, st = run(d, normal=n)
    assert np.isfinite(AM.from_half_bits(out["ambient_occlusion"])).all() and np.isfinite(AM.from_half_bits(out["noisy_occlusion"])).all()
    assert AM.counters(st)["sign_zero"] > 0  # sign(NaN) = 0: the class the drawn scene cannot produce


# ---- the GPU fixture is not degenerate -----------------------------------------------------------------------------------------------------


def test_the_main_gpu_frame_is_not_degenerate():
    """The frame tests/test_gpu_ambient_occlusion.py compares byte for byte -- occluder_scene(61) at 512 x 512, effect_radius 3.0, the ultra
    preset -- judged by the checker alone on the oracle's depth image: each of the five mip levels, fractional levels, results of exactly 1.0
    and inside (0, 1), zero-width arcs and both signs of sign_norm reach their floors.  The scene has no fully enclosed pixel and no NaN: an
    exactly-0.0 result and a zero sign_norm are reached by the two hand-made tests above instead."""
    depth, normal, view, proj, far = main_frame_inputs()
    st = {}
    out = AM.generate(depth, normal, hilbert(), view, proj, (MAIN_SIZE, MAIN_SIZE), far, slice_count=9, samples_per_slice_side=3, stats=st, **MAIN)
    c = assert_not_degenerate(st)
    print(c)
    assert c["samples"] == c["non_sky_pixels"] * 54 == sum(c[f"mip{k}"] for k in range(5))
    assert c["sign_minus"] + c["sign_zero"] + c["sign_plus"] == c["non_sky_pixels"] * 9
    assert c["result_one"] + c["result_partial"] + c["result_zero"] == c["non_sky_pixels"]
    ao = AM.from_half_bits(out["ambient_occlusion"])
    assert ((ao > 0) & (ao < 1)).sum() > 1000
