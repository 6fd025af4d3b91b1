"""tests/tonemap_model.py, the checker of oxc_apply_tonemap, on the CPU: hand-derived known answers, an independent binary64 transcription of
every tone curve written here with math.pow / exp / log2, and a guard that the images the other tests lean on take both sides of every
branch.

Measured here: over the 400 colours (1200 codes) of test_curve_against_the_binary64_transcription the final 8-bit codes of the checker and of
the transcription are equal for ACES and AgX_DS and differ in 3 codes, by 1, for GT7; DESIGN.md section 19 records the figures."""
import math

import numpy as np
import pytest

import tonemap_model as TM
from pixel_rules import pack_b10g11r11

F = np.float32


def planes(colours):
    a = np.asarray(colours, dtype=np.float32)
    return tuple(np.ascontiguousarray(a[:, c]) for c in range(3))


def b10g11r11_image(r, g, b):
    return pack_b10g11r11(np.asarray(r, np.float32).reshape(-1), np.asarray(g, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)).astype(np.uint32).reshape(np.shape(r))


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------------------
def test_none_with_exposure_one_is_the_identity_up_to_the_store():
    """Values exact in UF11 / UF10 and in 8 bits: k / 255 is not, so take 0, 0.25, 0.5, 1 and store Unorm: floor(v * 255 + 0.5)."""
    v = np.array([[0.0, 0.25, 0.5, 1.0, 2.0]], dtype=np.float32)
    out = TM.apply_tonemap(b10g11r11_image(v, v[:, ::-1], v), 0, TM.OUT_RGBA8_UNORM, 0, TM.NONE)
    codes = np.array([0, 64, 128, 255, 255])  # 63.75 + 0.5 and 127.5 + 0.5 floor to 64 and 128; 2.0 saturates
    assert (out & 0xFF).tolist() == [codes.tolist()] and ((out >> 8) & 0xFF).tolist() == [codes[::-1].tolist()] and ((out >> 16) & 0xFF).tolist() == [codes.tolist()]
    assert ((out >> 24) == 255).all()


def test_aces_of_black_is_zero():
    """RRTAndODTFit(0) = -0.000090537 / 0.238081 < 0, times the output matrix's row sums (about 1.0, 1.0, 1.0) stays negative: saturate gives 0."""
    st = {}
    out = TM.aces_fitted(planes([[0.0, 0.0, 0.0]]), st)
    assert [float(c[0]) for c in out] == [0.0, 0.0, 0.0] and st["aces below 0"] == 3


def test_gt7_curve_is_the_identity_on_its_linear_section():
    """Between midPoint_ (0.538) and linearSection_ * peak (0.444 * 2.5 = 1.11) weightLinear is 1 and weightToe 0: 0 * toe + 1 * x = x."""
    k = TM.constants()
    x = np.array([0.5380001, 0.6, 0.75, 1.0, 1.1099999], dtype=np.float32)
    assert np.array_equal(TM.gt_curve(x, k), x)
    assert float(k["gt_lin_peak"]) == float(F(F(0.444) * F(2.5))) and float(k["gt_target"]) == 2.5 and float(k["gt_sdr"]) == float(F(0.4))
    assert TM.gt_curve(np.array([-1.0, -0.0, 0.0], dtype=np.float32), k).tolist() == [0.0, 0.0, 0.0]
    # far up the shoulder the curve converges to kA_ = peak * (linearSection_ + k): exp(x * kC_) underflows
    assert float(TM.gt_curve(np.array([1.0e4], dtype=np.float32), k)[0]) == float(k["gt_ka"])


def test_vignette_amount_zero_leaves_the_colour_alone():
    ys, xs = np.mgrid[0:5, 0:7].astype(np.int64)
    assert (TM.vignette_factor(7, 5, xs, ys, 0.0) == F(1.0)).all()  # cos(0) = 1
    one = TM.vignette_factor(7, 1, xs[:1], ys[:1], 0.5)             # a centre of 0: 0 / 0 = NaN, clamp gives 0
    assert (one == 0).all()
    # amount 2 puts the corner of an even image at cos(pi / 2) on each axis: the rule's cosine of a quarter turn is 0 exactly only when the
    # argument rounds to the quarter turn; the factor is tiny either way
    assert TM.vignette_factor(8, 8, np.array([[0]]), np.array([[0]]), 2.0)[0, 0] < 1.0e-20


def test_cos_rule():
    assert TM.cos_turn_rule(np.array([0.0, -0.0], dtype=np.float32)).tolist() == [1.0, 1.0]
    assert np.isnan(TM.cos_turn_rule(np.array([np.inf, -np.inf, np.nan], dtype=np.float32))).all()
    a = np.linspace(-40.0, 40.0, 2001, dtype=np.float32)  # more than six turns to either side
    # the rule rounds the turn t in [0, 1) to binary32: up to 2^-25 of a turn, 2 pi 2^-25 = 1.9e-7 of angle, and |d cos| <= |d angle|; the result
    # is rounded to binary32 once more, half an ulp of a value up to 1: 2^-25
    bound = 2.0 * math.pi * 2.0 ** -25 + 2.0 ** -25
    assert np.max(np.abs(TM.cos_turn_rule(a).astype(np.float64) - np.cos(a.astype(np.float64)))) <= bound


def test_pcg3d16_known_answers():
    """v = v * 12829 + 47989; x += y z; y += z x; z += x y; twice; >> 16 -- all modulo 2^32, worked with unbounded integers:
      (0, 0, 0): 47989 each -> round 1 (2302992110, 189954107, 2375789647) -> round 2 (3141049635, 1183808008, 3134210919) -> (47928, 18063, 47824)
      (1, 2, 3): (60818, 73647, 86476) -> (2073791494, 1128831607, 4214949014) -> (1358752192, 3395326199, 2327612630) -> (20732, 51808, 35516)
      (191, 77, 0xFFFFFFFF): the seed wraps, -12829 + 47989 = 35160: (2498328, 1035822, 35160) -> (2062261480, 1476781550, 3673157896)
                 -> (499243608, 2362020014, 2929449176) -> (7617, 36041, 44699)"""
    for triple, want in (((0, 0, 0), (47928, 18063, 47824)), ((1, 2, 3), (20732, 51808, 35516)), ((191, 77, 0xFFFFFFFF), (7617, 36041, 44699))):
        got = TM.pcg3d16(*(np.array([v], dtype=np.uint64) for v in triple))
        assert tuple(int(g[0]) for g in got) == want


def test_grain_divisor():
    """i32(scale / 8): 0 for every scale below 8 and taken as 1; 8 -> 1; 17 -> 2."""
    assert [TM.grain_divisor(s) for s in (0.5, 1.0, 7.999, 8.0, 17.0, 3.0e10)] == [1, 1, 1, 1, 2, 2147483647]


def test_srgb_store_known_answers():
    """0 -> 0;  0.0031308 (the linear side, <=): 0.0031308 * 12.92 * 255 = 10.31 -> 10;  0.5 -> 1.055 * 0.5^(1 / 2.4) - 0.055 = 0.73536,
    * 255 = 187.52 -> 188;  1 -> 1.055 - 0.055 = 1 -> 255.  Alpha takes no curve: 0.5 -> 128."""
    c = np.array([0.0, 0.0031308, 0.5, 1.0], dtype=np.float32)
    st = {}
    out = TM.store((c, c, c), np.full(4, 0.5, dtype=np.float32), TM.OUT_RGBA8_SRGB, st)
    assert (out & 0xFF).tolist() == [0, 10, 188, 255] and (out >> 24).tolist() == [128] * 4 and st["srgb linear"] == 6
    rgb = (np.array([1.0], np.float32), np.array([0.5], np.float32), np.array([0.0], np.float32))
    one = np.ones(1, np.float32)
    assert int(TM.store(rgb, one, TM.OUT_RGBA8_SRGB)[0]) == 0xFF00BCFF and int(TM.store(rgb, one, TM.OUT_BGRA8_SRGB)[0]) == 0xFFFFBC00
    assert int(TM.store(rgb, one, TM.OUT_RGBA8_UNORM)[0]) == 0xFF0080FF
    nan = np.array([np.nan], np.float32)
    assert int(TM.store((nan, nan, nan), nan, TM.OUT_RGBA8_SRGB)[0]) == 0


def test_repeat_bilinear_wraps():
    """A 4 x 1 level sampled at u = 0: g = -0.5, the texels are -1 -> 3 and 0, the weight 0.5."""
    plane = np.array([[1.0, 2.0, 4.0, 8.0]], dtype=np.float32)
    got = TM.bilinear_repeat(plane, np.array([[0.0, 1.0, 0.125, np.inf, np.nan]], dtype=np.float32), np.zeros((1, 5), dtype=np.float32))
    assert got[0, :3].tolist() == [4.5, 4.5, 1.0] and np.isnan(got[0, 3:]).all()


def test_chromatic_aberration_replaces_the_colour():
    """Step 7 as the reference writes it: with the flag the exposure and the curve have no effect on the result."""
    rng = np.random.default_rng(4)
    img = b10g11r11_image(*(rng.uniform(0.0, 1.0, (9, 11)).astype(np.float32) for _ in range(3)))
    a = TM.apply_tonemap(img, 0, 0, TM.HAS_CHROMATIC_ABERRATION, TM.ACES, exposure=1.0)
    b = TM.apply_tonemap(img, 0, 0, TM.HAS_CHROMATIC_ABERRATION, TM.GT7, exposure=7.0)
    assert np.array_equal(a, b) and not np.array_equal(a, TM.apply_tonemap(img, 0, 0, 0, TM.ACES))


# ---- 2. the binary64 transcription --------------------------------------------------------------------------------------------------------------
class Margin:
    """The smallest distance of a compared value from its branch point, relative to the branch point (absolute 1e-6 at 0)."""

    def __init__(self):
        self.ok = True

    def lt(self, x, t):
        if abs(x - t) < (1.0e-3 * abs(t) if t else 1.0e-6):
            self.ok = False
        return x < t


def mv(M, v):
    return [sum(M[r][c] * v[c] for c in range(3)) for r in range(3)]


def inv3(m):
    (a, b, c), (d, e, f), (g, h, i) = m
    A, B, C, D, E, Fc, G, H, I = e * i - f * h, -(d * i - f * g), d * h - e * g, -(b * i - c * h), a * i - c * g, -(a * h - b * g), b * f - c * e, -(a * f - c * d), a * e - b * d  # noqa: E741
    det = a * A + b * B + c * C
    return [[A / det, D / det, G / det], [B / det, E / det, H / det], [C / det, Fc / det, I / det]]


def primaries64(r, g, b, w):
    un = lambda p: (p[0] / p[1], 1.0, (1.0 - p[0] - p[1]) / p[1])  # noqa: E731
    R, G, B, W = un(r), un(g), un(b), un(w)
    scale = mv(inv3([[R[0], G[0], B[0]], [1.0, 1.0, 1.0], [R[2], G[2], B[2]]]), W)
    return [[R[k] * scale[0], G[k] * scale[1], B[k] * scale[2]] for k in range(3)]


def aces64(c, mg):
    v = mv(TM.ACES_IN, c)
    v = [(x * (x + 0.0245786) - 0.000090537) / (x * (0.983729 * x + 0.4329510) + 0.238081) for x in v]
    return [min(max(x, 0.0), 1.0) for x in mv(TM.ACES_OUT, v)]


def agx64(c, mg):
    xr, xg, xb, xw = (0.64, 0.33), (0.3, 0.6), (0.15, 0.06), (0.3127, 0.3290)
    s = 1.0 / (1.0 - 0.15)
    lerp = lambda a, b: (a[0] + (b[0] - a[0]) * s, a[1] + (b[1] - a[1]) * s)  # noqa: E731
    to_xyz, adj = primaries64(xr, xg, xb, xw), primaries64(lerp(xw, xr), lerp(xw, xg), lerp(xw, xb), xw)
    inv_adj = inv3(adj)
    M = [[sum(to_xyz[r][j] * inv_adj[j][col] for j in range(3)) for col in range(3)] for r in range(3)]
    w = mv(M, [max(x, 0.0) for x in c])

    def dual(x, linear=0.10, peak=1.0):
        S = peak * linear
        if mg.lt(x, S):
            return x
        return peak - (peak - S) * math.exp((-(peak / (peak - S)) * (x - S)) / peak)

    w = [min(max(dual(x), 0.0), 1.0) for x in w]
    d = w[0] * 0.2126729 + w[1] * 0.7151522 + w[2] * 0.0721750
    w = [min(max(d + (x - d) * 1.3, 0.0), 1.0) for x in w]
    return mv(inv3(M), w)


M1, M2, C1, C2, C3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875


def inv_eotf64(v):
    y = v * 100.0 / 10000.0
    ym = math.pow(y, M1) if y > 0.0 else 0.0
    return 2.0 ** (M2 * (math.log2(C1 + C2 * ym) - math.log2(1.0 + C3 * ym)))


def eotf64(n, mg):
    n = 0.0 if mg.lt(n, 0.0) else n
    n = 1.0 if mg.lt(1.0, n) else n
    np_ = math.pow(n, 1.0 / M2) if n > 0.0 else 0.0
    l = np_ - C1  # noqa: E741
    l = 0.0 if mg.lt(l, 0.0) else l  # noqa: E741
    l = l / (C2 - C3 * np_)  # noqa: E741
    return (math.pow(l, 1.0 / M1) if l > 0.0 else 0.0) * 10000.0 / 100.0


def ictcp64(rgb):
    r, g, b = rgb
    lp, mp, sp = (inv_eotf64(v) for v in ((r * 1688.0 + g * 2146.0 + b * 262.0) / 4096.0, (r * 683.0 + g * 2951.0 + b * 462.0) / 4096.0, (r * 99.0 + g * 309.0 + b * 3688.0) / 4096.0))
    return [(2048.0 * lp + 2048.0 * mp) / 4096.0, (6610.0 * lp - 13613.0 * mp + 7003.0 * sp) / 4096.0, (17933.0 * lp - 17390.0 * mp - 543.0 * sp) / 4096.0]


def smooth64(x, e0, e1, mg):
    t = (x - e0) / (e1 - e0)
    if mg.lt(x, e0):
        return 0.0
    if mg.lt(e1, x):
        return 1.0
    return t * t * (3.0 - 2.0 * t)


def gt764(c, mg):
    target = 250.0 / 100.0
    sdr = 1.0 / target
    alpha, mid, lin, toe = 0.25, 0.538, 0.444, 1.280
    k = (lin - 1.0) / (alpha - 1.0)
    kA, kB, kC = target * lin + target * k, -target * k * math.exp(lin / k), -1.0 / (k * target)
    target_ucs = ictcp64([target] * 3)[0]

    def curve(x):
        if mg.lt(x, 0.0):
            return 0.0
        wl = smooth64(x, 0.0, mid, mg)
        if mg.lt(x, lin * target):
            return (1.0 - wl) * (mid * (math.pow(x / mid, toe) if x > 0.0 else 0.0)) + wl * x
        return kA + kB * math.exp(x * kC)

    rgb = mv(TM.XYZ_TO_REC2020, mv(TM.REC709_TO_XYZ, c))
    ucs = ictcp64(rgb)
    skewed = [curve(x) for x in rgb]
    chroma = 1.0 - smooth64(ucs[0] / target_ucs, 0.98, 1.16, mg)
    i, ct, cp = ictcp64(skewed)[0], ucs[1] * chroma, ucs[2] * chroma
    ll, ml, sl = (eotf64(v, mg) for v in (i + 0.00860904 * ct + 0.11103 * cp, i - 0.00860904 * ct - 0.11103 * cp, i + 0.560031 * ct - 0.320627 * cp))
    scaled = [max(3.43661 * ll - 2.50645 * ml + 0.0698454 * sl, 0.0), max(-0.79133 * ll + 1.9836 * ml - 0.192271 * sl, 0.0), max(-0.0259499 * ll - 0.0989137 * ml + 1.12486 * sl, 0.0)]
    out = [sdr * min((1.0 - 0.6) * skewed[ch] + 0.6 * scaled[ch], target) for ch in range(3)]
    return mv(TM.XYZ_TO_REC709, mv(TM.REC2020_TO_XYZ, out))


def code64(c, mg):
    c = min(max(c, 0.0), 1.0)
    e = c * 12.92 if not mg.lt(0.0031308, c) else 1.055 * math.pow(c, 1.0 / 2.4) - 0.055
    return math.floor(min(max(e, 0.0), 1.0) * 255.0 + 0.5)


def candidate_colours(n, seed):
    """Binary32 colours, log-uniform over 2^-9 .. 2^4 per channel with one channel in eight black."""
    rng = np.random.default_rng(seed)
    c = np.exp2(rng.uniform(-9.0, 4.0, (n, 3)))
    return np.where(rng.random((n, 3)) < 0.125, 0.0, c).astype(np.float32)


@pytest.mark.parametrize("curve,transcription", [(TM.ACES, aces64), (TM.AGX, agx64), (TM.GT7, gt764)], ids=["aces", "agx", "gt7"])
def test_curve_against_the_binary64_transcription(curve, transcription):
    """400 colours, each at least 1e-3 relative away from every branch point the transcription meets (colours nearer are passed over): the
    8-bit sRGB codes of the checker and of the transcription differ by at most 1 in every channel."""
    kept, want = [], []
    for colour in candidate_colours(1200, 17 + curve):
        mg = Margin()
        codes = [code64(x, mg) for x in transcription([float(v) for v in colour], mg)]
        if mg.ok:
            kept.append(colour)
            want.append(codes)
        if len(kept) == 400:
            break
    assert len(kept) == 400
    out = TM.store(TM.tone_curve(planes(kept), curve, TM.constants()), np.ones(400, dtype=np.float32), TM.OUT_RGBA8_SRGB)
    got = np.stack([(out >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.int64)
    diff = np.abs(got - np.asarray(want, dtype=np.int64))
    print(f"curve {curve}: {int((diff != 0).sum())} of {diff.size} codes differ, the largest difference {int(diff.max())}")
    assert diff.max() <= 1
    assert len({tuple(r) for r in got.tolist()}) > 200  # the colours are spread over the curve, not all saturated


# ---- 3. the degeneracy guard --------------------------------------------------------------------------------------------------------------------
def guard_planes(seed=23, n=4096):
    """The colours of test_gpu_tonemap's random images: log-uniform over 2^-10 .. 2^6, a tenth black, and (RGBA16F holds them) a tenth
    negative."""
    rng = np.random.default_rng(seed)
    c = np.exp2(rng.uniform(-10.0, 6.0, (n, 3)))
    c = np.where(rng.random((n, 3)) < 0.1, 0.0, c)
    c = np.where(rng.random((n, 3)) < 0.1, -c, c)
    return planes(c.astype(np.float16).astype(np.float32))


BRANCHES = {TM.ACES: ["aces below 0", "aces above 1"], TM.AGX: ["agx linear"],
            TM.GT7: ["gt negative", "gt toe or linear", "gt weight below", "gt weight above", "gt chroma below", "gt chroma above", "eotf below 0", "eotf above 1",
                     "eotf l below 0", "gt above target"]}


@pytest.mark.parametrize("curve", [TM.ACES, TM.AGX, TM.GT7], ids=["aces", "agx", "gt7"])
def test_the_guard_colours_take_both_sides_of_every_branch(curve):
    st = {}
    out = TM.tone_curve(guard_planes(), curve, TM.constants(), st)
    TM.store(out, np.ones(4096, dtype=np.float32), TM.OUT_RGBA8_SRGB, st)
    for name in BRANCHES[curve] + ["srgb linear"]:
        assert st[name] >= 16 and st["not " + name] >= 16, (name, st[name], st["not " + name])


def test_the_lens_branches():
    """Film grain: the divisor's two cases (0 taken as 1, and 2); round-half-to-even is met (a tie exists among the rounded values is not
    required, but both roundings up and down are); the vignette's clamp meets NaN (a side of 1) and ordinary values."""
    ys, xs = np.mgrid[0:33, 0:65].astype(np.int64)
    assert TM.grain_divisor(1.0) == 1 and TM.grain_divisor(17.0) == 2
    g1, g17 = TM.film_grain(xs, ys, 1.0, 0), TM.film_grain(xs, ys, 17.0, 0xFFFFFFFF)
    assert np.isfinite(g1).all() and np.isfinite(g17).all() and g1.min() >= -1.0 and g1.max() <= 1.0
    assert len(np.unique(g1)) > 1000 and len(np.unique(g17)) > 1000
    assert (g1 < 0).any() and (g1 > 0).any()
    v = TM.vignette_factor(65, 33, xs, ys, 9.0)  # 9 * pi / 4 at the corner: more than a turn
    assert v.min() == 0.0 or v.min() < 1.0e-3
    assert v.max() == 1.0 and len(np.unique(v)) > 100
