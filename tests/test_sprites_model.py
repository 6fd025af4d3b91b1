"""CPU tests of the 2D pass: the checker (tests/sprites_model.py) against a slow per-pixel, per-sprite transcription of 2d_forward_vis.slang,
2d_forward.slang and the pipeline state, written on its own in plain Python loops (Python integers after the snap, binary64 for the depth);
oxc_pack_sprite and oxc_sort_sprites through the built library against a transcription of RenderQueue2D::add and SpriteGPUData::operator>;
the golden fixture; and the properties the GPU frames rest on (order, the two-stage rule, the quantisation between sprites)."""
import ctypes
import dataclasses
import functools
import math
import struct

import numpy as np
import pytest

import pixel_rules as PR
import sprites_frames as SF
import sprites_model as SM

F = np.float32


# ---- the slow transcription ------------------------------------------------------------------------------------------------------------------
def _half(bits: int) -> float:
    """com::dequantize_half on Python numbers: exponent field 0 gives the sign alone."""
    v = struct.unpack("<e", struct.pack("<H", bits))[0]
    return math.copysign(0.0, v) if not bits & 0x7C00 else v


def _vertex(world, pv, x, y):
    m = lambda M, r, c: F(M[c * 4 + r])  # noqa: E731
    w = [F(F(F(m(world, r, 0) * F(x)) + F(m(world, r, 1) * F(y))) + F(m(world, r, 2) * F(0.0))) + m(world, r, 3) for r in range(3)]
    return [F(F(F(m(pv, r, 0) * w[0]) + F(m(pv, r, 1) * w[1])) + F(m(pv, r, 2) * w[2])) + m(pv, r, 3) for r in range(4)]


def _slow_sprite(f, k, W, H):
    """None, or (rgba, transform_id, [oriented (X, Y, z) triangles]) of sprite k: vs_main, the viewport, the snap, cullMode eNone."""
    n, material_count, transform_count = f.counts
    w0, w1, tid = (int(v) for v in f.sprites[f.first_sprite + k])
    if tid >= transform_count:
        return None
    rec = f.materials[w0 & 0xFFFF] if (w0 & 0xFFFF) < material_count else [0] * 28
    rgba = [F(_half(int(rec[c]))) for c in range(4)]
    if rgba[3] <= F(_half(int(rec[9]))):  # discard
        return None
    tris = []
    sign = -1.0 if (w1 & 0xFFFF) & 2 else 1.0
    for t in range(2):
        corners = [_vertex(f.transforms[tid], f.pv, px * sign, py) for px, py in SM.POSITIONS[3 * t:3 * t + 3]]
        X, Y, z = [], [], []
        for cx, cy, cz, cw in corners:
            assert cw >= F(2.0 ** -10) and abs(cx) <= F(64.0) * cw and abs(cy) <= F(64.0) * cw, "the transcription does not clip"
            sx = F(F(F(F(cx / cw) * F(0.5)) + F(0.5)) * F(W))
            sy = F(F(F(F(cy / cw) * F(0.5)) + F(0.5)) * F(H))
            X.append(math.floor(F(F(sx * F(256.0)) + F(0.5))))
            Y.append(math.floor(F(F(sy * F(256.0)) + F(0.5))))
            z.append(F(cz / cw))
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        if area == 0:
            continue
        if area < 0:
            X, Y, z = [X[0], X[2], X[1]], [Y[0], Y[2], Y[1]], [z[0], z[2], z[1]]
        tris.append((X, Y, z, abs(area)))
    return rgba, tid, tris


def _slow_fragment(tri, px, py):
    """The depth of the fragment of `tri` at pixel (px, py), or None: top-left rule, depth in (0, 1]."""
    X, Y, z, area = tri
    cx, cy = 256 * px + 128, 256 * py + 128
    e = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        v = dx * (cy - Y[a]) - dy * (cx - X[a])
        if v < 0 or (v == 0 and not (dy > 0 or (dy == 0 and dx < 0))):
            return None
        e.append(v)
    d = F(((float(e[0]) * float(z[0]) + float(e[1]) * float(z[1])) + float(e[2]) * float(z[2])) * (1.0 / float(area)))
    return d if d > 0 and not d > 1 else None


def slow_draw(f, stages, fmt):
    W, H = f.extent
    n = f.counts[0]
    sprites = [_slow_sprite(f, k, W, H) for k in range(n)]
    depth = f.depth.copy()
    vis = np.full((H, W), SM.EMPTY, np.uint32) if f.clear else f.vis.copy()
    color = f.color_in(fmt).copy()
    with np.errstate(all="ignore"):
        for stage in (SM.VIS, SM.COLOR):
            if not stages & stage:
                continue
            for py in range(H):
                for px in range(W):
                    for s in sprites:
                        if s is None:
                            continue
                        rgba, tid, tris = s
                        for tri in tris:
                            d = _slow_fragment(tri, px, py)
                            if d is None or not d >= depth[py, px]:
                                continue
                            depth[py, px] = d
                            if stage == SM.VIS:
                                vis[py, px] = tid
                                continue
                            a = rgba[3]
                            if fmt == SM.B10G11R11:
                                dst = [c[0] for c in PR.unpack_b10g11r11(color[py, px])]
                                out = [F(F(rgba[c] * a) + F(dst[c] * F(F(1.0) - a))) for c in range(3)]
                                color[py, px] = PR.pack_b10g11r11(*out)[0]
                            else:
                                dst = [F(v) for v in color[py, px].view(np.float16)]
                                out = [F(F(rgba[c] * a) + F(dst[c] * F(F(1.0) - a))) for c in range(3)] + [F(a + F(dst[3] * F(F(1.0) - a)))]
                                color[py, px] = [PR.channel_half(v) for v in out]
    out = dict(depth=depth)
    if stages & SM.VIS:
        out["vis"] = vis
    if stages & SM.COLOR:
        out["color"] = color
    return out


def _same(got, want, label):
    assert got.keys() == want.keys()
    for k in got:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        g, w = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert g.shape == w.shape and (g == w).all(), f"{label}: {k}: {int((g != w).sum())} elements differ"


@functools.lru_cache(None)
def _frames():
    tilted = SF.stack_frame((13, 11), n=5, same_depth=False)
    tilted.transforms[1] = SF.quad(13, 11, 6, 5, 7, 8, 0.5, angle=0.8, mirror=True)
    tilted.transforms[2] = SF.quad(13, 11, 5, 6, 0, 0, 0.5)  # zero scale: zero area
    tilted.sprites[3, 1] |= SM.FLIP_X
    return {"golden": SF.golden_frame(), "stack": SF.stack_frame(), "tilted": tilted}


@pytest.mark.parametrize("fmt", SF.FORMATS)
@pytest.mark.parametrize("stages", SF.STAGES)
@pytest.mark.parametrize("name", ["golden", "stack", "tilted"])
def test_the_checker_equals_the_slow_transcription(name, stages, fmt):
    f = _frames()[name]
    _same(SF.want(f, stages, fmt), slow_draw(f, stages, fmt), f"{name} stages {stages} format {fmt}")


def test_the_golden_fixture_is_the_checkers_output():
    f = SF.golden_frame()
    with np.load(SF.GOLDEN) as g:
        for name in ("sprites", "materials", "transforms", "depth", "color", "pv"):
            assert (np.ascontiguousarray(g["in_" + name]).view(np.uint8) == np.ascontiguousarray(getattr(f, name)).view(np.uint8)).all(), name
        for fmt in SF.FORMATS:
            for stages in SF.STAGES:
                _same(SF.want(f, stages, fmt), {k: g[f"{k}_format{fmt}_stages{stages}"] for k in SF.want(f, stages, fmt)}, f"format {fmt} stages {stages}")
        assert (g[f"vis_format0_stages{SM.ALL}"] != SM.EMPTY).any() and (g[f"color_format0_stages{SM.ALL}"] != f.color).any()


def test_order_shows_and_the_two_stage_rule_hides_it():
    """Eight translucent sprites at one depth: the reversed list gives another image, and the vis word is the last sprite's.  Back to front
    against front to back: the colour stage alone differs, both stages do not (S7)."""
    f = SF.stack_frame()
    r = dataclasses.replace(f, sprites=f.sprites[::-1].copy())
    for stages in SF.STAGES:
        a, b = SF.want(f, stages), SF.want(r, stages)
        key = "vis" if stages == SM.VIS else "color"
        assert (a[key] != b[key]).any(), stages
    stats = {}
    top = SF.want(f, SM.VIS, stats=stats)["vis"]
    last = stats["blends"][7] > 0  # where the last sprite has a fragment (all are at one depth: every fragment passes) the word is its transform
    assert last.sum() > 20 and (top[last] == 7).all() and (top[~last] != 7).all()
    g = SF.stack_frame(same_depth=False)
    back = dataclasses.replace(g, sprites=g.sprites[::-1].copy())
    assert (SF.want(g, SM.COLOR)["color"] != SF.want(back, SM.COLOR)["color"]).any()
    _same(SF.want(g, SM.ALL), SF.want(back, SM.ALL), "both stages")


@pytest.mark.parametrize("fmt", SF.FORMATS)
def test_the_quantisation_between_sprites_shows(fmt):
    f = SF.stack_frame()
    assert (SF.want(f, SM.COLOR, fmt)["color"] != SF.want(f, SM.COLOR, fmt, requantize=False)["color"]).any()


def test_no_pixel_of_a_diagonal_sprite_blends_twice_and_none_is_missed():
    """A rotated and a sheared sprite, alpha 0.5: along the shared edge of the two triangles every pixel takes exactly one fragment."""
    W, H = 33, 21
    d, color = SF.background(W, H)
    f = SF.Frame(SF.sprites_of([(0, 0), (1, 0)]), SF.materials_of([(1.0, 0.5, 0.25, 0.5)]),
                 np.stack([SF.quad(W, H, 10, 10, 14, 9, 0.5, angle=0.6), SF.quad(W, H, 22, 11, 12, 10, 0.5, shear=0.5)]), d, color)
    stats = {}
    SF.want(f, SM.COLOR, stats=stats)
    for k in (0, 1):
        count = stats["blends"][k]
        assert count.max() == 1 and count.sum() > 60
        rows = [np.flatnonzero(row) for row in count if row.any()]
        assert all((np.diff(r) == 1).all() for r in rows), "a hole inside a convex sprite's row"


# ---- the host helpers through the library ------------------------------------------------------------------------------------------------------
def _add(render_flags, position_y, transform_id, material_id, distance):
    """RenderQueue2D::add, glm::packHalf1x16 as the round-to-nearest-even conversion."""
    half = lambda v: int(np.array([v], np.float32).astype(np.float16).view(np.uint16)[0])  # noqa: E731
    h = lambda v: 0x7E00 if v != v else half(v)  # noqa: E731
    with np.errstate(all="ignore"):
        return ((material_id & 0xFFFF) | (h(position_y) << 16), (render_flags & 0xFFFF) | (h(distance) << 16), transform_id)


def _greater(a, b) -> bool:
    """SpriteGPUData::operator>."""
    key = lambda s: (((s[1] >> 16) & 0xFFFF) << 32) | ((((~(s[0] >> 16)) & 0xFFFF) if (s[0] >> 16) & 0x8000 else ((s[0] >> 16) | 0x8000)) if s[1] & 1 else 0)  # noqa: E731
    return key(a) > key(b)


TIE = 1.0 + 2.0 ** -11  # exactly between two halves
Y_VALUES = [0.0, -0.0, 1.0, -1.0, 3.5, -3.5, TIE, np.nextafter(F(TIE), F(2.0)), np.nextafter(F(TIE), F(0.0)), -TIE, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, 1e6,
            -1e6, 6e-8, 2.0 ** -25, np.nextafter(F(2.0 ** -25), F(1.0)), 2.0 ** -24, 6.1e-5, 1e-10, float("inf"), float("-inf"), float("nan")]


def test_pack_sprite_is_render_queue_add():
    from oxylus_amd import renderer as R

    with np.errstate(all="ignore"):
        for y in Y_VALUES:
            for dist in (0.0, 2.5, -7.0, TIE):
                for flags, tid, mat in ((0, 0, 0), (3, 0xFFFFFFFF, 0x12345), (0x1FFFF, 77, 65535)):
                    got = R.pack_sprite(flags, y, tid, mat, dist)
                    assert got == _add(flags, float(F(y)), tid, mat, float(F(dist))) == SM.pack_sprite(flags, y, tid, mat, dist), (y, dist, flags, tid, mat, got)
    rng = np.random.default_rng(3)
    bits = np.concatenate([rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32), np.arange(0x33000000 - 64, 0x33000000 + 64, dtype=np.uint32),
                           np.arange(0x477FE000 - 64, 0x477FE000 + 8300, 97, dtype=np.uint32)])
    with np.errstate(all="ignore"):
        for v in bits.view(np.float32):
            assert R.pack_sprite(0, float(v), 0, 0, 0.0)[0] >> 16 == _add(0, float(v), 0, 0, 0.0)[0] >> 16, hex(int(v.view(np.uint32)))
    lib = R.L.load()
    assert lib.oxc_pack_sprite(0, 0.0, 0, 0, 0.0, None) == R.L.OXC_INVALID_ARG


def test_sort_sprites_is_render_queue_sort_and_stable():
    from oxylus_amd import renderer as R

    rng = np.random.default_rng(11)
    ys = [float(F(v)) for v in Y_VALUES if v == v]
    entries = []
    for i in range(400):
        flags = int(rng.integers(0, 4))  # SORT_Y on about half of them
        entries.append(_add(flags, ys[int(rng.integers(len(ys)))], i, int(rng.integers(0, 5)), [0.5, 1.0, 2.0, -1.0][int(rng.integers(4))]))
    sprites = np.array(entries, np.uint32)
    got = R.sort_sprites(sprites.copy())
    for a, b in zip(got[:-1], got[1:]):
        assert not _greater(tuple(int(v) for v in b), tuple(int(v) for v in a)), "not descending"
        if not _greater(tuple(int(v) for v in a), tuple(int(v) for v in b)):
            assert a[2] < b[2], "equal keys must keep submission order"
    assert (got == SM.sort_sprites(sprites)).all()
    assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, sprites.tolist()))
    one = sprites[:1].copy()
    assert (R.sort_sprites(one.copy()) == one).all()
    assert R.sort_sprites(np.zeros((0, 3), np.uint32)).shape == (0, 3)
    lib = R.L.load()
    assert lib.oxc_sort_sprites(None, 0) == R.L.OXC_OK and lib.oxc_sort_sprites(None, 2) == R.L.OXC_INVALID_ARG
    assert ctypes.sizeof(R.L.Sprite) == 12
