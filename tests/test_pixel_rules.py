"""The rules pixel_rules shares with oxylus_amd/csrc/oxcull_pixel_device.hpp, at the inputs where a copy could drift: known answers written from
the header's statement of each rule -- by hand where the rule gives an exact value, else by a scalar transcription of the header's line in
binary32, one operation at a time -- and the structure that keeps the checkers from growing copies again.  CPU only."""
import ast
import glob
import math
import os

import numpy as np
import pytest

import pixel_rules as PR

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
TESTS = os.path.dirname(os.path.abspath(__file__))
KNEE = F(0.0031308)
ABOVE_ONE = np.nextafter(F(1.0), F(2.0))
# tonemap_model.srgb_encode(c, stats) counts the side of the comparison and returns the shared rule: the one wrapper under a shared name
WRAPPERS = {("tonemap_model", "srgb_encode")}


def words(v):
    return np.atleast_1d(np.asarray(v, dtype=np.float32)).view(np.uint32).tolist()


def word(v):
    return words(F(v))[0]


def power(base, exponent):
    """pow_rule of two binary32 scalars, as a binary32 scalar."""
    return PR.pow_rule(F(base), F(exponent))[0]


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------
def test_srgb_decode_all_bytes():
    """c = f32(byte) / 255; c <= 0.04045 ? c / 12.92 : pow_rule((c + 0.055) / 1.055, 2.4).  0.04045 * 255 = 10.3: bytes 0 .. 10 are linear."""
    want = []
    for byte in range(256):
        c = F(byte) / F(255.0)
        want.append(c / F(12.92) if c <= F(0.04045) else power((c + F(0.055)) / F(1.055), 2.4))
        assert (c <= F(0.04045)) == (byte <= 10)
    got = PR.srgb_decode(np.arange(256, dtype=np.uint32))
    assert words(got) == words(want)
    assert got[0] == 0.0 and got[255] == 1.0  # pow(1, p) = exp2(p * 0) = 1


def test_srgb_encodes_differ_where_saturation_applies():
    """srgb_encode: c = saturate(c); c <= 0.0031308 ? c * 12.92 : 1.055 * pow_rule(c, 0.4166666666666667f) - 0.055.  The encode inside srgb_unorm
    does not saturate: x <= 0.0031308 ? 12.92 * x : 1.055 * pow_rule(x, 1.0f / 2.4f) - 0.055.  A NaN fails the comparison and pow_rule(NaN, p)
    is exp2(p * -Inf) = 0, so the unsaturated encode of a NaN is 1.055 * 0 - 0.055.  Just above 1 the curve's own rounding hides the missing
    saturate (pow(1 + 2^-23, 1 / 2.4) = 1 + 5e-8 rounds to 1); 2.0 shows it."""
    below, above = np.nextafter(KNEE, F(0.0)), np.nextafter(KNEE, F(1.0))
    p_sat, p_unorm = F(0.4166666666666667), F(1.0) / F(2.4)
    assert word(p_sat) == word(p_unorm)  # the two spellings of the exponent are one binary32
    curve = lambda x, p: F(1.055) * power(x, p) - F(0.055)  # noqa: E731
    x = np.array([0.0, -0.0, below, KNEE, above, 1.0, ABOVE_ONE, NAN, -1.0, 2.0], dtype=np.float32)
    sat, unorm = PR.srgb_encode(x), PR.srgb_unorm_encode(x)
    one = F(1.055) * F(1.0) - F(0.055)
    want_sat = [F(0.0), None, below * F(12.92), KNEE * F(12.92), curve(above, p_sat), one, one, F(0.0), F(0.0), one]
    want_unorm = [F(0.0), F(-0.0), F(12.92) * below, F(12.92) * KNEE, curve(above, p_unorm), one, curve(ABOVE_ONE, p_unorm), F(-0.055), F(-12.92), curve(2.0, p_unorm)]
    for k, (ws, wu) in enumerate(zip(want_sat, want_unorm)):
        assert ws is None or word(sat[k]) == word(ws), (k, sat[k], ws)
        assert word(unorm[k]) == word(wu), (k, unorm[k], wu)
    assert sat[1] == 0.0  # saturate(-0) is a zero of either sign
    differ = [word(a) != word(b) for a, b in zip(sat, unorm)]
    assert differ[2:] == [False, False, False, False, False, True, True, True] and not differ[0]
    assert curve(ABOVE_ONE, p_unorm) == one and curve(2.0, p_unorm) > one


def test_exp_rule():
    """exp2_f64_round((double)x * log2(e)): 1 at 0; exp(88) is finite and exp(-88) a binary32 denormal; at +-104 the argument of exp2 is
    +-150.04, inside the +-160 of the closed form, and the one rounding gives +Inf and (0.97 x 2^-150 lies under half the least denormal) 0."""
    x = np.array([0.0, -0.0, 88.0, -88.0, 104.0, -104.0, INF, -INF, NAN], dtype=np.float32)
    got = PR.exp_rule(x)
    # the binary64 chain is within 1e-15 of the real value, which math.exp gives to an ulp of binary64
    want = [F(1.0), F(1.0), F(math.exp(88.0)), F(math.exp(-88.0)), INF, F(0.0), INF, F(0.0)]
    assert words(got[:8]) == words(want) and np.isnan(got[8])
    assert np.isfinite(got[2]) and 0.0 < got[3] < F(2.0 ** -126)


def turn_pair(a):
    """The header's cos_sin_angle_rule on one finite binary32 a, a line at a time."""
    aa = abs(float(F(a)))
    u = aa * float.fromhex("0x1.45f306dc9c883p-3")
    t = F(u - math.floor(u))
    t = F(0.0) if t == F(1.0) else t
    cs, sn = PR.cos_sin_turn(t)
    return F(cs), (-F(sn) if F(a) < 0 else F(sn))


def test_cos_turn_and_cos_sin_angle_rules():
    """The binary32 nearest pi / 2 is 0.25 + 7e-9 of a turn, which rounds to the turn 0.25: octant 1 with nothing left, so cos = -sq = -0.0 and
    sin = cq = 1 exactly.  The largest finite value times 1 / (2 pi) is a binary64 integer: the turn 0, cos 1, sin +-0."""
    half_pi, big = F(math.pi / 2), F(np.finfo(np.float32).max)
    exact = [(0.0, 1.0, 0.0), (-0.0, 1.0, 0.0), (half_pi, -0.0, 1.0), (-half_pi, -0.0, -1.0), (big, 1.0, 0.0), (-big, 1.0, -0.0)]
    a = np.array([e[0] for e in exact], dtype=np.float32)
    cs, sn = PR.cos_sin_angle_rule(a)
    assert words(cs) == words([e[1] for e in exact]) and words(sn) == words([e[2] for e in exact])
    turns = np.array([s * F(2.0 * math.pi * k) for k in (1, 2, 3, 7, 1000) for s in (1, -1)], dtype=np.float32)
    cs, sn = PR.cos_sin_angle_rule(turns)
    want = [turn_pair(v) for v in turns]
    assert words(cs) == words([w[0] for w in want]) and words(sn) == words([w[1] for w in want])
    assert (cs[:8] == 1.0).all() and (np.abs(sn[:8]) < 4e-6).all() and words(sn[0::2]) == words(-sn[1::2])  # the negated sine for a < 0
    bad = np.array([INF, -INF, NAN], dtype=np.float32)
    assert np.isnan(PR.cos_sin_angle_rule(bad)[0]).all() and np.isnan(PR.cos_sin_angle_rule(bad)[1]).all() and np.isnan(PR.cos_turn_rule(bad)).all()
    everything = np.concatenate([a, turns, bad])
    assert words(PR.cos_turn_rule(everything)) == words(PR.cos_sin_angle_rule(everything)[0])  # "cs is cos_turn_rule(a) bit for bit"


@pytest.mark.parametrize("n", [1, 2, 3])
def test_axis_clamp(n):
    """axis_at<false>: g = p * n - 0.5, fl = floor(g), i = the saturating conversion of fl (a NaN gives 0), i0 = clamp(i, 0, n - 1), i1 =
    clamp(i + 1, 0, n - 1), f = g - fl."""
    last = n - 1
    under, over = np.nextafter(F(0.0), F(-1.0)), ABOVE_ONE
    p = np.array([0.0, 1.0, under, over, NAN, INF, -INF], dtype=np.float32)
    i0, i1, f = PR.axis_clamp(p, n)
    g_over = over * F(n) - F(0.5)
    # p = 0 and the denormal under it: g = -0.5, texel -1 clamps to 0 and so does texel 0.  p = 1 and just over: floor(g) = n - 1, the last texel
    # twice.  NaN: texel 0 and its neighbour.  +Inf: INT_MAX, both clamp to the last; -Inf: both clamp to 0; Inf - Inf = NaN.
    assert i0.tolist() == [0, last, 0, last, 0, last, 0]
    assert i1.tolist() == [0, last, 0, last, min(1, last), last, 0]
    assert words(f[:4]) == words([F(0.5), F(0.5), F(0.5), g_over - np.floor(g_over)]) and np.isnan(f[4:]).all()
    assert f[3] > F(0.5)
    for idx in (i0, i1):
        assert idx.min() >= 0 and idx.max() <= last


def test_unorm8():
    """pack_unorm: u32(floor(saturate(e) * 255.0 + 0.5)); a NaN gives 0."""
    half = F(0.5 / 255.0)
    below = np.nextafter(half, F(0.0))
    e = np.array([np.nextafter(below, F(0.0)), below, half, np.nextafter(half, F(1.0)), NAN, -1.0, 2.0], dtype=np.float32)
    want = [int(math.floor(v * F(255.0) + F(0.5))) for v in e[:4]] + [0, 0, 255]
    got = PR.unorm8(e)
    assert got.dtype == np.uint32 and got.tolist() == want
    # the neighbour below gives 0.5 - 2^-25 exactly, and the sum 1 - 2^-25 is a tie that rounds to 1.0: the step to byte 1 lies one value lower
    assert want[:4] == [0, 1, 1, 1]


def test_small_rules():
    x = np.array([1.75, -1.75, -0.0, 3.0], dtype=np.float32)
    assert words(PR.frac(x)) == words([0.75, 0.25, -0.0 - np.floor(F(-0.0)), 0.0])
    assert words(PR.lerp(F(2.0), F(4.0), x)) == words([F(2.0) + F(2.0) * v for v in x])  # a + (b - a) * t
    assert words(PR.clamp(np.array([NAN, -2.0, 0.5, 2.0], dtype=np.float32), -1, 1)) == words([-1.0, -1.0, 0.5, 1.0])  # max(NaN, lo) = lo
    counts = {}
    PR.count(counts, "a"), PR.count(counts, "a", 4), PR.count(counts, "a", np.array([[True, False], [True, True]])), PR.count(None, "a", 9)
    assert counts == {"a": 8} and type(counts["a"]) is int


def test_the_shared_rules_return_the_shape_of_their_input():
    one = {"exp_rule": PR.exp_rule, "cos_turn_rule": PR.cos_turn_rule, "srgb_encode": PR.srgb_encode, "srgb_unorm_encode": PR.srgb_unorm_encode,
           "unorm8": PR.unorm8, "srgb_decode": lambda v: PR.srgb_decode(np.asarray(v).astype(np.uint32)), "frac": lambda v: PR.frac(f32(v)),
           "clamp": lambda v: PR.clamp(v, 0.0, 1.0), "lerp": lambda v: PR.lerp(f32(v), F(1.0), F(0.5))}
    many = {"cos_sin_angle_rule": PR.cos_sin_angle_rule, "axis_clamp": lambda v: PR.axis_clamp(f32(v), 3)}
    for v in (0.25, F(0.25), np.full(5, 0.25, np.float32), np.full((2, 3), 0.25, np.float32)):
        for name, rule in one.items():
            assert np.shape(rule(v)) == np.shape(v), name
        for name, rule in many.items():
            assert all(np.shape(part) == np.shape(v) for part in rule(v)), name


def f32(v):
    return np.asarray(v, dtype=np.float32)


# ---- structure ----------------------------------------------------------------------------------------------------------------------------------
def checker_modules():
    return sorted(glob.glob(os.path.join(TESTS, "*_model.py")) + glob.glob(os.path.join(TESTS, "*_frames.py")))


def shared_names():
    with open(os.path.join(TESTS, "pixel_rules.py")) as f:
        return {node.name for node in ast.parse(f.read()).body if isinstance(node, ast.FunctionDef)}


def test_no_checker_defines_or_borrows_a_shared_rule():
    """No checker defines a top-level function under a name pixel_rules has, and none imports such a name from another checker."""
    shared = shared_names()
    assert {"exp_rule", "cos_turn_rule", "cos_sin_angle_rule", "srgb_decode", "srgb_encode", "srgb_unorm_encode", "unorm8", "lerp", "frac", "clamp", "axis_clamp",
            "count"} <= shared
    modules = checker_modules()
    assert len(modules) >= 30
    defined, borrowed = [], []
    for path in modules:
        module = os.path.basename(path)[:-3]
        with open(path) as f:
            tree = ast.parse(f.read())
        defined += [(module, node.name) for node in tree.body if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name in shared]
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.endswith("_model"):
                borrowed += [(module, node.module, alias.name) for alias in node.names if alias.name in shared]
    assert set(defined) == WRAPPERS, defined
    assert borrowed == []
