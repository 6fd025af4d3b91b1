"""The checker of oxc_resolve_shadowmap (tests/vsm_resolve_model.py) against plain-Python scalar versions of its noise hash and rotation,
the 2^-23 bound of the rotation, hand-derived known answers, the fallback order, and the texel addressing of the draw's checker
(tests/vsm_draw_model.py).  No GPU, no reference tree."""
import math

import numpy as np
import pytest

import vsm_draw_model as DM
import vsm_pages_model as VM
import vsm_resolve_model as RM

F = np.float32
BD = DM.BACKED | DM.DIRTY | DM.VISIBLE


# ---- rule 5 and 6 ------------------------------------------------------------------------------------------------------------------------
def test_noise_hash_matches_the_scalar_version():
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.arange(64), rng.integers(0, 65536, 500)]).astype(np.int64)
    ys = np.concatenate([np.arange(64)[::-1], rng.integers(0, 65536, 500)]).astype(np.int64)
    hx, hy = RM.pcg2d(xs, ys)
    nx, ny = RM.noise(xs, ys)
    for i in range(len(xs)):
        sx, sy = RM.pcg2d_scalar(int(xs[i]), int(ys[i]))
        assert (int(hx[i]), int(hy[i])) == (sx, sy)
        assert float(nx[i]) == (sx >> 8) / 16777216.0 and float(ny[i]) == (sy >> 8) / 16777216.0
    assert nx.min() >= 0 and nx.max() < 1 and ny.min() >= 0 and ny.max() < 1
    assert len({(int(a), int(b)) for a, b in zip(hx[:64], hy[:64])}) == 64  # neighbours decorrelate


def test_hammersley_points():
    assert RM.hammersley2d(0, 16) == (0.0, 0.0)
    assert RM.hammersley2d(1, 16) == (F(1) / F(16), 0.5)
    assert RM.hammersley2d(3, 24) == (F(3) / F(24), 0.75)
    assert RM.hammersley2d(23, 24)[1] == 0.90625  # 10111b reversed: 0.11101b


def test_rotation_matches_the_scalar_version():
    rng = np.random.default_rng(2)
    t = np.concatenate([rng.random(2000, dtype=np.float32), np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875], np.float32)])
    c, s = RM.cos_sin_turn(t)
    for i in range(len(t)):
        cs, ss = RM.cos_sin_turn_scalar(t[i])
        assert c[i].tobytes() == F(cs).tobytes() and s[i].tobytes() == F(ss).tobytes()


def test_rotation_is_within_2_pow_minus_23_of_the_exact_value():
    """Rule 6: every multiple of 2^-16 in [0, 1) and 10^5 random binary32 values, against numpy's binary64 sin / cos.  The binary64
    reference is itself within 2^-52 of the exact value at the octant-reduced argument, which does not move a 2^-23 bound."""
    rng = np.random.default_rng(3)
    t = np.concatenate([(np.arange(65536) / 65536.0).astype(np.float32), rng.random(100000, dtype=np.float32),
                        np.nextafter(np.float32([0.125, 0.25, 0.5, 1.0]), np.float32(0))])
    assert (t < 1).all()
    c, s = RM.cos_sin_turn(t)
    # exact reduction of the reference's argument too: 2 pi t through the quadrant, so the comparison is not limited by 2 pi t's rounding
    q = t.astype(np.float64) * 4.0
    k = np.floor(q)
    a = (q - k) * (math.pi / 2)
    cq, sq = np.cos(a), np.sin(a)
    ki = k.astype(int)
    cref = np.choose(ki, [cq, -sq, -cq, sq])
    sref = np.choose(ki, [sq, cq, -sq, -cq])
    err = max(np.abs(c.astype(np.float64) - cref).max(), np.abs(s.astype(np.float64) - sref).max())
    print("largest rotation error:", err, "bound", 2.0 ** -23)
    assert err <= 2.0 ** -23
    assert RM.cos_sin_turn(np.float32([0.0, 0.25, 0.5, 0.75]))[0].tolist() == [1.0, 0.0, -1.0, 0.0]


def test_oct_decode_inverts_the_encode():
    rng = np.random.default_rng(4)
    n = rng.normal(size=(500, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = RM.decode_normal(RM.encode_normal(n))
    assert np.abs(np.stack(d, axis=-1) - n).max() < 2e-3  # binary16 storage


# ---- hand-derived known answers ----------------------------------------------------------------------------------------------------------
# Identity inv_projection_view: world = (uv * 2 - 1, depth).  One orthographic clipmap 4 world units wide, light along +z (L = (0, 0, -1)
# points at the light), receiver normal (0, 0, -1): NoL = 1, so lerp(pcf_bias, 0, NoL) = 0 and base_bias = 2^-22 + 2 b.
# n = 8, page 16 (V = 128), physical 64 (P = 4): a page is 0.5 world units, a texel 1 / 32.  texel_len = ((4 * 7 / 8) * 2) / 128 = 7 / 128,
# cts = 2 * 7 / 128 = 0.109375, b = 0.0773..., base_bias = 0.1547...; the receiver sits at depth 0.5 - cts = 0.390625 after the normal offset.
# T = (-1, 0, 0), B = (0, 1, 0): the discs lie in the xy plane.  Pixel (4, 4) of the 8 x 8 image is world (0.125, 0.125): with radius <= 0.1
# every tap stays inside virtual page (4, 4), world [0, 0.5)^2.
SHAPE = dict(page_size=16, page_table_size=8, physical_page_table_size=64, clipmap_count=1, first_clipmap_width=4.0, bias=0.0, virtual_extent=128.0)
LIGHT = (0.0, 0.0, -1.0)
EYE = np.eye(4, dtype=np.float32).reshape(-1)


def _flat(count=1, widths=(4.0,), offsets=None, **over):
    depth = np.full((8, 8), 0.5, np.float32)
    normal = RM.encode_normal(np.broadcast_to(np.float32([0, 0, -1]), (8, 8, 3)))
    shape = dict(SHAPE, clipmap_count=count, **over)
    return depth, normal, RM.ortho_clipmaps(count, widths, offsets), shape


def _run(depth, normal, table, clip, phys, shape, z_length=1.0, stats=None):
    return RM.resolve(depth, normal, table, clip, phys, EYE, (8.0, 8.0), LIGHT, z_length, stats=stats, **shape)


def _one_page(value, addr=5, layer=0, count=1, page=(4, 4), flags=DM.BACKED):
    table = np.zeros((count, 8, 8), np.uint32)
    table[layer, page[1], page[0]] = DM.entry(addr, flags)
    phys = np.full((64, 64), 7.0, np.float32)  # texels no tap may read hold 7.0
    phys[(addr // 4) * 16:(addr // 4) * 16 + 16, (addr % 4) * 16:(addr % 4) * 16 + 16] = value
    return table, phys


def test_known_answers_of_a_flat_receiver():
    depth, normal, clip, shape = _flat()
    st = {}
    table, phys = _one_page(0.05)  # an occluder well in front: 0.05 + 0.155 < 0.39, all 16 search taps are blockers
    out = _run(depth, normal, table, clip, phys, shape, stats=st)
    assert out[4, 4] == 0.0 and st["outcome"][4, 4] == RM.ALL_BLOCKERS
    assert out[0, 0] == 1.0 and st["outcome"][0, 0] == RM.HARD  # far from the page: every tap misses, the centre too
    table, phys = _one_page(1.0)   # a cleared page: no blocker
    out = _run(depth, normal, table, clip, phys, shape, stats=st)
    assert out[4, 4] == 1.0 and st["outcome"][4, 4] == RM.NO_BLOCKER
    out = _run(depth, normal, np.zeros((1, 8, 8), np.uint32), clip, np.full((64, 64), 0.05, np.float32), shape, stats=st)
    assert (out == 1.0).all() and (st["outcome"] == RM.HARD).all() and st["misses"] == st["taps"] == 64 * 17  # nothing backed
    depth[:] = 0.0
    out = _run(depth, normal, table, clip, phys, shape, stats=st)
    assert (out == 1.0).all() and (st["outcome"] == RM.SKY).all() and st["taps"] == 0


def test_a_stored_minus_one_is_a_miss():
    """The Slang tells a miss by the value VSM_DEPTH_MISS = -1.0, so a backed page that holds -1.0 misses as well: all 17 taps of pixel
    (4, 4) miss and the hard-shadow path returns 1.0."""
    depth, normal, clip, shape = _flat()
    st = {}
    table, phys = _one_page(-1.0)
    out = _run(depth, normal, table, clip, phys, shape, stats=st)
    assert out[4, 4] == 1.0 and st["outcome"][4, 4] == RM.HARD


def test_half_occluded_value_is_a_ratio_of_counted_taps():
    """The page's texel columns left of world x = 0.125 (in-page column < 4: (0.125 / 4 + 0.5) * 128 = 68 = 4 * 16 + 4) hold an occluder at
    0.05, the others 1.0.  z_length = 500 makes pcf_radius = min(0.1, (0.390625 - 0.05) * 500 * 0.002) = 0.1.  The expected value is counted
    from the tap positions in plain Python: tap i of N sits at x = 0.125 - r cos(2 pi xi.y), r = sqrt(xi.x) * 0.1, and is lit when its
    texel column floor((x / 4 + 0.5) * 128) is >= 68."""
    depth, normal, clip, shape = _flat()
    table, phys = _one_page(1.0)
    phys[16:32, 16:20] = 0.05  # addr 5 = page (1, 1) of the physical image: columns 0..3
    st = {}
    out = _run(depth, normal, table, clip, phys, shape, z_length=500.0, stats=st)
    sx, sy = RM.pcg2d_scalar(4, 4)
    n0, n1 = (sx >> 8) / 2.0 ** 24, (sy >> 8) / 2.0 ** 24

    def lit_taps(N, a, b, radius):
        lit = []
        for i in range(N):
            h0, h1 = i / N, int(f"{i:032b}"[::-1], 2) / 2.0 ** 32
            x0, x1 = (h0 + a) % 1.0, (h1 + b) % 1.0
            x = 0.125 - math.sqrt(x0) * radius * math.cos(2 * math.pi * x1)
            col = (x / 4 + 0.5) * 128
            assert abs(col - round(col)) > 1e-3, "a tap on a texel edge: the hand count would depend on rounding"
            lit.append(math.floor(col) >= 68)
        return lit

    search = lit_taps(16, n0, n1, 0.1)
    assert 0 < sum(search) < 16  # some blockers, not all: the PCF loop runs
    pcf = lit_taps(24, n1, n0, 0.1)
    assert st["outcome"][4, 4] == RM.PCF
    assert out[4, 4] == F(sum(pcf)) / F(24)
    assert 0 < sum(pcf) < 24


# ---- fallback ----------------------------------------------------------------------------------------------------------------------------
def _three(bias):
    depth, normal, clip, shape = _flat(3, (4.0, 4.0, 4.0), bias=bias)
    return depth, normal, clip, shape


@pytest.mark.parametrize("bias,base", [(-100.0, 0), (0.5, 1), (5.0, 2)])
def test_fallback_reads_the_neighbouring_clipmaps_in_order(bias, base):
    """Three identical clipmaps; the bias alone picks the base.  bias 5: k - bias < 0 for k = 0 and 1, index 2 = count - 1.  bias -100:
    r > 2^(k + 100) never holds, index 0.  bias 0.5: k = 0 counts (-0.5 < 0), k = 1 counts when r > 2^0.5; the footprint is 2 / 8 world
    units and first_clipmap_width 400 makes texel_len = 700 / 128, so r = 0.046 and the index is 1.  With one page backed in one layer
    at a time, every hit is served by that layer's place in the order base, base - 1, base + 1."""
    depth, normal, clip, shape = _three(bias)
    if base == 1:
        shape["first_clipmap_width"] = 400.0
    for layer, expect in ((base, "base"), (base - 1, "minus"), (base + 1, "plus")):
        if not 0 <= layer < 3:
            continue
        table, phys = _one_page(0.05 if expect != "base" else 1.0, layer=layer, count=3)
        st = {}
        _run(depth, normal, table, clip, phys, shape, stats=st)
        served = {"base": st["taps"] - st["misses"] - st["fallback_minus"] - st["fallback_plus"], "minus": st["fallback_minus"], "plus": st["fallback_plus"]}
        assert served[expect] >= 17 and sum(served.values()) == served[expect], (layer, expect, served)
    # base - 1 wins over base + 1 when both are backed
    if base == 1:
        t0, _ = _one_page(1.0, addr=5, layer=0, count=3)
        t2, _ = _one_page(1.0, addr=6, layer=2, count=3)
        st = {}
        _run(depth, normal, t0 | t2, clip, np.ones((64, 64), np.float32), shape, stats=st)
        assert st["fallback_minus"] >= 17 and st["fallback_plus"] == 0
    # base = 0 and base = count - 1 never index outside the array: every entry backed, the sentinel layers do not exist
    full = np.full((3, 8, 8), DM.entry(0, DM.BACKED), np.uint32)
    out = _run(depth, normal, full, clip, np.ones((64, 64), np.float32), shape, stats=st)
    assert (out == 1.0).all() and st["misses"] == 0


def test_unbacked_invalidated_and_out_of_range_entries_miss():
    depth, normal, clip, shape = _flat()
    for flags, addr in ((VM.INVALIDATED, 5), (DM.VISIBLE | DM.DIRTY, 5), (DM.BACKED, 16), (DM.BACKED, 65535)):
        table = np.zeros((1, 8, 8), np.uint32)
        table[0, 4, 4] = DM.entry(addr, flags)
        st = {}
        out = _run(depth, normal, table, clip, np.full((64, 64), 0.05, np.float32), shape, stats=st)
        assert out[4, 4] == 1.0 and st["outcome"][4, 4] == RM.HARD and st["misses"] == st["taps"], (flags, addr)


def test_non_finite_inputs_do_not_raise_and_stay_in_bounds():
    depth, normal, clip, shape = _flat()
    table, phys = _one_page(0.05)
    depth[4, 4] = np.nan
    depth[2, 2] = np.inf
    normal = normal.copy()
    normal[5, 5] = 0x7E00  # NaN halves
    out = _run(depth, normal, table, clip, phys, shape)
    assert out.shape == (8, 8) and out[0, 0] == 1.0


# ---- addressing: a tap reads the texel the draw wrote ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 128, 8192, 10), (8, 48, 144, 3), (16, 32, 256, 4)], ids=["reference", "phys144-V384", "phys256-V512"])
def test_a_tap_reads_the_texel_the_draw_writes(shape):
    n, ps, phys, count = shape
    V, P = n * ps, phys // ps
    rng = np.random.default_rng(sum(shape))
    offsets = [(int(rng.integers(-3 * n, 3 * n)), int(rng.integers(-3 * n, 3 * n))) for _ in range(count)]
    offsets[0] = (-5, 7)
    scales = [float(2 ** c) for c in range(count)]
    clip = DM.pixel_clipmaps(count, V, offsets=offsets, scales=scales)
    table = ((rng.integers(0, P * P, (count, n, n)).astype(np.uint32) << 16) | np.uint32(BD))
    pm = DM.page_map(table, clip, count, n, ps, phys)
    S = RM.Shape(table, clip, np.zeros((phys, phys), np.float32), page_size=ps, page_table_size=n, physical_page_table_size=phys, clipmap_count=count)
    K = 4000
    c = rng.integers(0, count, K)
    x, y = rng.integers(0, V, K), rng.integers(0, V, K)
    x[:4], y[:4] = [0, V - 1, 0, V - 1], [0, 0, V - 1, V - 1]
    s = np.float32(scales)[c]
    p = ((x.astype(np.float32) + F(0.5)) * s, (y.astype(np.float32) + F(0.5)) * s, np.full(K, 0.5, np.float32))
    ok, X, Y = RM.tap_address(S, c, p)
    assert ok.all()
    m = pm[c, y // ps, x // ps]  # the draw's: physical page of the pixel's virtual page, then the pixel's place in the page
    assert (m[:, 0] >= 0).all()
    assert np.array_equal(X, m[:, 0] * ps + x % ps) and np.array_equal(Y, m[:, 1] * ps + y % ps)
    assert X.max() < phys and Y.max() < phys
