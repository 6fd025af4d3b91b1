"""raster_model (the header's unclipped rules in Python) against the C checker on every frame of raster_frames, `predict` against the walker
each case was written for and against hand-worked answers at each boundary, and the proofs that the stride frames are not vacuous.  CPU."""
import numpy as np
import pytest
import torch

import raster_frames as RF
import raster_model as RM


def _same(case_or_frame, form=0):
    f = getattr(case_or_frame, "frame", case_or_frame)
    image, setups = f.model_image()
    want = f.oracle_image(form).numpy().view(np.uint64)
    bad = np.argwhere(image != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), [(hex(int(image[y, x])), hex(int(want[y, x]))) for y, x in bad[:4]])
    return image, setups


def _check_case(case):
    case.check_intent()
    image, setups = _same(case)
    if case.expect is not None:
        got = [RM.predict(t)[0] for t in setups]
        assert got == case.expect, list(zip(got, case.expect))
    return image, setups


@pytest.mark.parametrize("name", sorted(RF.threshold_cases()))
def test_threshold_case_model_equals_oracle_and_takes_its_walker(oracle_lib, name):
    case = RF.threshold_cases()[name]
    image, setups = _check_case(case)
    assert image.any()
    # the vectorised evaluation against the same rule in Python integers, at every pixel of a small image and a lattice of a large one
    f = case.frame
    step = 1 if f.W * f.H <= 1024 else 7
    for y in range(0, f.H, step):
        for x in range(0, f.W, step):
            assert int(image[y, x]) == max(RM.pixel(t, v[0], x, y) if t else 0 for t, v in zip(setups, f.model_frame())), (x, y)


def test_predict_hand_worked_boundaries():
    def p(tri, W, H):
        t = RM.setup(([v[0] for v in tri], [v[1] for v in tri], [RM.F(0.5)] * 3), W, H)
        return RM.predict(t)

    # a front face has negative area before orientation: (0,0) (0,h) (w,0)
    assert p([(512, 512), (512, 2560), (2560, 512)], 32, 32) == (RM.SMALL, 0, False)          # centres 2..9 in x and y: 8 x 8
    assert p([(512, 512), (512, 2560), (2561 + 255, 512)], 32, 32) == (RM.RECT32, 0, True)    # 2816 - 128 = 2688 = 10.5 px: centres 2..10: 9 wide
    assert p([(512, 512), (512, 2560), (2560 + 127, 512)], 32, 32) == (RM.SMALL, 0, False)    # 2687 - 128 < 2560: still 8 wide
    assert p([(512, 512), (512, 2560), (2560 + 128, 512)], 32, 32) == (RM.RECT32, 0, True)    # a centre exactly on the maximum counts: 9 wide
    assert p([(512, 512), (2560, 512), (512, 2560)], 32, 32) == (RM.DROPPED, 0, False)        # the other winding
    assert p([(512, 512), (512, 2560), (512, 4000)], 32, 32) == (RM.DROPPED, 0, False)        # zero area
    assert p([(-2560, 512), (-2560, 2560), (-512, 512)], 32, 32) == (RM.DROPPED, 0, False)    # left of the image: empty clamped box
    assert p([(2048, 2048), (2048, -2047), (-2047, 2048)], 16, 16) == (RM.SMALL, 0, False)    # spread 4095, clamped box 8 x 8
    assert p([(2048, 2048), (2048, -2047), (-2048, 2048)], 16, 16) == (RM.RECT32, 0, True)    # spread 4096
    assert p([(512, 512), (512, 512 + 64 * 256), (512 + 64 * 256, 512)], 128, 128) == (RM.RECT32, 0, True)
    assert p([(512, 512), (512, 512 + 64 * 256), (512 + 65 * 256, 512)], 128, 128) == (RM.TILES32, 2, True)
    assert p([(512, 512), (512, 512 + 65 * 256), (512 + 65 * 256, 512)], 128, 128) == (RM.TILES32, 4, True)
    assert p([(512, 512), (512, 512 + 65 * 256), (512 + 65 * 256, 512)], 66, 66) == (RM.RECT32, 0, True)  # clamped to 64 x 64 by the extent
    assert p([(0, 0), (0, 32767), (32767, 0)], 128, 128) == (RM.TILES32, 4, True)
    assert p([(0, 0), (0, 32767), (32768, 0)], 128, 128) == (RM.TILES64, 4, True)
    assert p([(0, 0), (0, 32768), (32767, 0)], 128, 128) == (RM.TILES64, 4, True)
    assert p([(0, 0), (0, 32767), (32767, 0)], 64, 64) == (RM.RECT32, 0, True)
    assert p([(0, 0), (0, 32768), (32767, 0)], 64, 64) == (RM.RECT64, 0, True)
    assert p([(0, 0), (0, 1025 * 256), (1025 * 256, 0)], 2048, 2048) == (RM.TILES64, 289, True)
    t = RM.setup(([0, 0, 32768], [0, 32767, 0], [RM.F(0.5)] * 3), 128, 128)
    assert RM.setup_uses_wide_area(t) and t["area"] == 32768 * 32767
    assert not RM.setup_uses_wide_area(RM.setup(([0, 0, 32767], [0, 32767, 0], [RM.F(0.5)] * 3), 128, 128))


def test_depth_rule_and_equal_depth_by_hand(oracle_lib):
    c = RF.threshold_cases()
    image, _ = _same(c["depth-flat"])
    depth = (image >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert (depth[:, 0:8] == 1.0).any() and not image[:, 8:].any()  # 1.0 kept; the next binary32 above 1, 0 and -0.5 dropped
    image, _ = _same(c["depth-slope"])
    depth = (image >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert (depth[1:8, 8] == 1.0).all() and not image[:, 9:17].any() and (depth[1, 1:8] > 0).all()  # kept up to exactly 1.0, dropped above
    assert not image[:, 17:26].any() and (depth[1, 26:] > 0).all()  # dropped up to exactly 0.0, kept above
    half = RF.half_depth_case()
    image, _ = _check_case(half)
    assert image[:, :8].any() and not image[:, 8:].any()
    image, _ = _same(c["equal-depth"])
    vis = (image & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert vis[4, 4] == 1 << 8 and vis[2, 8] == 0  # where both cover, the larger vis


@pytest.mark.parametrize("s", [8, 40, 200])
def test_shared_diagonal_is_owned_once_in_each_walker(oracle_lib, s):
    case = RF.threshold_cases()[f"diagonal-{s}"]
    f = case.frame
    a, _ = f.model_image(f.draw[:1])
    b, _ = f.model_image(f.draw[1:])
    quad = np.zeros((f.H, f.W), dtype=bool)
    quad[2:2 + s, 2:2 + s] = True
    assert np.array_equal((a != 0) ^ (b != 0), quad) and not ((a != 0) & (b != 0)).any()
    on_diagonal = [(x, 3 + s - x) for x in range(2, 2 + s)]
    assert all((a[y, x] != 0) != (b[y, x] != 0) for x, y in on_diagonal)
    for part, img in ((f.draw[:1], a), (f.draw[1:], b)):
        assert np.array_equal(f.oracle_image(draw=part).numpy().view(np.uint64), img)


@pytest.mark.parametrize("W,H", RF.RASTER_EXTENTS, ids=RF.RASTER_EXTENT_IDS)
def test_extent_case_model_equals_oracle(oracle_lib, W, H):
    case = RF.extent_case(W, H)
    image, setups = _check_case(case)
    assert image.all()  # the far triangle covers every pixel
    kinds = [RM.predict(t)[0] for t in setups]
    assert kinds[9] == RM.DROPPED  # the triangle wholly outside: empty clamped box
    vis = (image & np.uint64(0xFFFFFFFF)).astype(np.uint32) >> 8
    for n, (x, y) in enumerate(((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))):
        assert vis[y, x] >= 10  # a corner pixel shows one of the one-pixel triangles (10..13; the same one where corners coincide)
    assert vis[H - 1, W - 1] == 13


@pytest.mark.parametrize("form", [0, 1, 2])
def test_stride_frame_model_equals_oracle_in_every_index_form(oracle_lib, form):
    f = RF.stride_frame()
    draw = RF.stride_draw(1025)
    image, _ = f.model_image(draw)
    assert np.array_equal(f.oracle_image(form, draw).numpy().view(np.uint64), image)


def test_stride_frame_is_not_vacuous(oracle_lib):
    """Every triangle of the 1025-triangle list owns pixels (so leaving any one out changes the image).  Exchanging the instances of two
    entries one grid step (256 entries) apart changes the image whenever the two name different triangles of the mesh (with the same
    triangle the exchange is the same set of triangles, listed in another order); and an entry drawn with the instance of the entry one
    step before it -- what a stale MeshletInstance record amounts to -- changes it for every entry."""
    f = RF.stride_frame()
    draw = list(RF.stride_draw(1025))
    assert len({i for i, _, _ in draw}) >= 300 and len(set(draw)) == 1025
    full = f.oracle_image(draw=draw)
    shown = set(np.unique(full.numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)).tolist())
    assert all(f.vis(*d) in shown for d in draw)  # each vis is unique, so its pixels are nobody else's
    _, setups = f.model_image(draw)
    assert all(RM.predict(t)[0] == RM.SMALL and t["px1"] - t["px0"] < 3 and t["py1"] - t["py0"] < 3 for t in setups)
    for n in (0, 300, 768):  # leaving one out, by the draw itself
        assert not torch.equal(f.oracle_image(draw=draw[:n] + draw[n + 1:]), full)
    exchanged = 0
    for n in range(0, 1025 - 256):
        (ia, ka, ja), (ib, kb, jb) = draw[n], draw[n + 256]
        assert ia != ib
        stale = list(draw)
        stale[n + 256] = (ia, kb, jb)
        assert not torch.equal(f.oracle_image(draw=stale), full), n
        if (ka, ja) != (kb, jb):
            swapped = list(draw)
            swapped[n], swapped[n + 256] = (ib, ka, ja), (ia, kb, jb)
            assert not torch.equal(f.oracle_image(draw=swapped), full), n
            exchanged += 1
    assert exchanged > 500
    for n in range(1024):
        assert draw[n][0] != draw[n + 1][0] or draw[n][1:] != draw[n + 1][1:]


def test_clipped_stride_frame_crosses_the_camera_plane(oracle_lib):
    import oracle

    f = RF.clipped_stride_frame()
    vd = f.oracle_image()
    assert oracle.draw_clipped_count() >= 130
    assert len(np.unique(vd.numpy().view(np.uint64) & np.uint64(0xFFFFFFFF))) > 100  # most of the slivers show


def test_clipped_pairs_go_through_the_clipper(oracle_lib):
    import oracle

    for W in (8, 64):
        vd = RF.clipped_pair(W).frame.oracle_image()
        assert oracle.draw_clipped_count() == 2 and (vd != 0).any()


def test_tile_overflow_case_model_equals_oracle(oracle_lib):
    case = RF.tile_overflow_case()
    image, setups = _check_case(case)
    big = [t for t in setups if t is not None]
    assert len(big) == RF.TILE_BIG and all(t["px1"] - t["px0"] + 1 == 1025 and t["py1"] - t["py0"] + 1 == 1025 for t in big)
    assert sum(RM.predict(t)[1] for t in setups) == RF.TILE_BIG * 289 > 8192
    assert len(np.unique(image[image != 0] & np.uint64(0xFFFFFFFF))) == RF.TILE_BIG  # every big triangle shows somewhere


@pytest.mark.parametrize("count", [0, 1, 2, 3, 7, 8, 15])
def test_trailing_indices_are_ignored(oracle_lib, count):
    f = RF.index_count_frame().frame
    want, _ = f.model_image(f.draw[:count // 3])
    assert np.array_equal(f.oracle_image(count=count).numpy().view(np.uint64), want)
    assert (want != 0).any() == (count >= 3)
