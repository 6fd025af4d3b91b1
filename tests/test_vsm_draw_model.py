"""The checker of oxc_draw_physical_pages (tests/vsm_draw_model.py) against hand-derived answers, and pinned to the oracle's
orc_draw_visbuffer on the rules the two draws share (no GPU needed)."""
import numpy as np
import torch

import vsm_draw_model as DM

# the hand cases' shape: 8 x 8 virtual pages of 16 texels (V = 128), a 64 x 64 physical image (P = 4: 16 physical pages), 3 clipmaps
N, PS, PHYS, COUNT = 8, 16, 64, 3
V = N * PS


def _draw(tris_xyz, table, flags, clipmaps=None, image=1.0, shape=(N, PS, PHYS, COUNT)):
    n, ps, phys, count = shape
    s, idx = DM.flat_scene(tris_xyz)
    img = np.full((phys, phys), image, dtype=np.float32)
    return DM.draw(img, s, s.meshlet_instances, idx, [idx.numel(), 1, 0, 0, 0], table, DM.pixel_clipmaps(count, n * ps) if clipmaps is None else clipmaps,
                   flags, page_size=ps, page_table_size=n, physical_page_table_size=phys, clipmap_count=count)


def _table(entries, count=COUNT, n=N):
    """{(clipmap, wrapped y, wrapped x): entry} -> uint32 [count, n, n]"""
    t = np.zeros((count, n, n), dtype=np.uint32)
    for (c, y, x), e in entries.items():
        t[c, y, x] = e
    return t


def _right_triangle_sets(x0, y0, leg):
    """Pixel centres strictly inside the triangle (x0, y0), (x0, y0 + leg), (x0 + leg, y0), and those on its diagonal."""
    inside = {(x, y) for y in range(V) for x in range(V) if x >= x0 and y >= y0 and x + y + 1 < x0 + y0 + leg}
    diag = {(x, y) for y in range(V) for x in range(V) if x >= x0 and y >= y0 and x + y + 1 == x0 + y0 + leg}
    return inside, diag


def _written(img, value=1.0):
    ys, xs = np.nonzero(img != np.float32(value))
    return {(int(x), int(y)) for x, y in zip(xs, ys)}


def test_a_triangle_lands_on_its_physical_texels_through_a_wrapping_page_offset():
    """Clipmap 1, page_offset (3, -2): the triangle's pixels lie in virtual page (5, 1) (x 80..95, y 16..31), which wraps to
    ((5 + 3) mod 8, (1 - 2) mod 8) = (0, 7).  That entry holds physical page 6 = (6 % 4, 6 / 4) = (2, 1): texel (32, 16) + (x - 80, y - 16)."""
    clip = DM.pixel_clipmaps(COUNT, V, offsets=[(0, 0), (3, -2), (0, 0)])
    img = _draw([[(82, 18, 0.5), (82, 30, 0.5), (94, 18, 0.5)]], _table({(1, 7, 0): DM.entry(6)}), [0, 1, 0], clipmaps=clip)
    inside, diag = _right_triangle_sets(82, 18, 12)
    to_phys = lambda s: {(32 + x - 80, 16 + y - 16) for x, y in s}  # noqa: E731
    got = _written(img)
    assert to_phys(inside) <= got <= to_phys(inside | diag) and len(inside) > 50
    assert all(img[y, x] == np.float32(0.5) for x, y in got)


def test_unbacked_and_clean_pages_and_a_clean_clipmap_get_nothing():
    tri = [[(82, 18, 0.5), (82, 30, 0.5), (94, 18, 0.5)]]  # virtual page (5, 1) in every clipmap (page_offset 0)
    table = _table({(0, 1, 5): DM.entry(1), (1, 1, 5): DM.entry(2, DM.VISIBLE | DM.BACKED), (2, 1, 5): DM.entry(3, DM.VISIBLE | DM.DIRTY)})
    assert not _written(_draw(tri, table, [0, 1, 1]))  # clipmap 0 is drawable but its dirty flag is 0; 1 is clean, 2 unbacked
    assert _written(_draw(tri, table, [1, 1, 1]))      # the same table with clipmap 0 active


def test_both_windings_are_drawn():
    table = _table({(0, 1, 1): DM.entry(0), (0, 1, 2): DM.entry(1)})  # pages (1, 1) -> physical (0, 0), (2, 1) -> physical (1, 0)
    a = [(20, 20, 0.5), (20, 28, 0.5), (28, 20, 0.5)]  # negative fixed-point area (front face of the visbuffer draw)
    b = [(36, 20, 0.5), (44, 20, 0.5), (36, 28, 0.5)]  # the other winding
    got_a, got_b = _written(_draw([a], table, [1, 0, 0])), _written(_draw([b], table, [1, 0, 0]))
    ia, da = _right_triangle_sets(20, 20, 8)
    ib, db = _right_triangle_sets(36, 20, 8)
    assert {(x - 16, y - 16) for x, y in ia} <= got_a <= {(x - 16, y - 16) for x, y in ia | da}
    assert {(x - 32 + 16, y - 16) for x, y in ib} <= got_b <= {(x - 32 + 16, y - 16) for x, y in ib | db}


def test_two_triangles_sharing_an_edge_cover_every_pixel_once():
    """A quad split along its diagonal, the halves wound oppositely, depths 0.25 and 0.75: drawn alone they cover disjoint sets whose union
    is the quad; drawn together every texel holds the depth of the one triangle that covers it."""
    table = _table({(0, 0, 0): DM.entry(5)})  # page (0, 0) -> physical (1, 1): texel (16, 16) + (x, y)
    a = [(2, 2, 0.25), (2, 10, 0.25), (10, 2, 0.25)]
    b = [(10, 2, 0.75), (10, 10, 0.75), (2, 10, 0.75)]
    ia, ib = _draw([a], table, [1, 0, 0]), _draw([b], table, [1, 0, 0])
    wa, wb = _written(ia), _written(ib)
    quad = {(16 + x, 16 + y) for y in range(2, 10) for x in range(2, 10)}
    assert not (wa & wb) and (wa | wb) == quad
    both = _draw([a, b], table, [1, 0, 0])
    assert _written(both) == quad
    assert np.array_equal(both.view(np.uint32), np.minimum(ia.view(np.uint32), ib.view(np.uint32)))


def test_the_smaller_depth_wins():
    table = _table({(0, 0, 0): DM.entry(0)})
    near = [(2, 2, 0.25), (2, 12, 0.25), (12, 2, 0.25)]
    far = [(3, 3, 0.625), (3, 13, 0.625), (13, 3, 0.625)]
    img = _draw([far, near], table, [1, 0, 0])
    assert img[4, 4] == np.float32(0.25) and img[12, 3] == np.float32(0.625)  # overlap: the nearer; far alone: its own
    assert np.array_equal(img, _draw([near, far], table, [1, 0, 0]))


def test_depth_outside_zero_one_is_dropped():
    table = _table({(0, 0, 0): DM.entry(0)})
    tri = lambda z: [(2, 2, z), (2, 10, z), (10, 2, z)]  # noqa: E731
    assert not _written(_draw([tri(-0.25)], table, [1, 0, 0], image=2.0), 2.0)
    assert not _written(_draw([tri(1.5)], table, [1, 0, 0], image=2.0), 2.0)
    assert set(np.unique(_draw([tri(0.0)], table, [1, 0, 0], image=2.0)).tolist()) == {0.0, 2.0}
    assert set(np.unique(_draw([tri(1.0)], table, [1, 0, 0], image=2.0)).tolist()) == {1.0, 2.0}


def test_the_command_list_is_descending_and_copies_the_source_command():
    src = [300, 1, 7, 0, 2]
    cmds, cnt, cl = DM.build_draw_commands([1, 0, 1, 1], 4, src, commands=np.full((4, 5), -7), clipmaps=np.full(4, -7))
    assert cnt == 3 and cl.tolist() == [3, 2, 0, 0xFFFFFFF9]
    assert cmds[:3].tolist() == [src] * 3 and cmds[3].tolist() == [0xFFFFFFF9] * 5
    assert DM.build_draw_commands([0, 0], 2, src)[1] == 0


def test_a_command_with_instance_count_zero_draws_nothing():
    s, idx = DM.flat_scene([[(2, 2, 0.5), (2, 10, 0.5), (10, 2, 0.5)]])
    img = np.ones((PHYS, PHYS), np.float32)
    out = DM.draw(img, s, s.meshlet_instances, idx, [idx.numel(), 0, 0, 0, 0], _table({(0, 0, 0): DM.entry(0)}), DM.pixel_clipmaps(COUNT, V), [1, 0, 0],
                  page_size=PS, page_table_size=N, physical_page_table_size=PHYS, clipmap_count=COUNT)
    assert np.array_equal(out, img)


def grid_scene(cells=12, step=10, seed=3):
    """A jittered grid of cells x cells quads split in two, every triangle wound like the visbuffer draw's front faces, per-vertex depths
    in (0.1, 0.9): no two triangles overlap."""
    rng = np.random.default_rng(seed)
    g = np.zeros((cells + 1, cells + 1, 3))
    for j in range(cells + 1):
        for i in range(cells + 1):
            jx, jy = (rng.integers(-8, 9, 2) / 4.0) if 0 < i < cells and 0 < j < cells else (0.0, 0.0)
            z = float(np.float16(rng.uniform(0.1, 0.9)))
            g[j, i] = (4 + i * step + jx, 4 + j * step + jy, z)
    tris = []
    for j in range(cells):
        for i in range(cells):
            p00, p10, p01, p11 = (tuple(g[j, i]), tuple(g[j, i + 1]), tuple(g[j + 1, i]), tuple(g[j + 1, i + 1]))
            tris += [[p00, p01, p10], [p10, p01, p11]]
    return tris


def test_pinned_to_the_oracle_visbuffer_draw_on_the_shared_rules():
    """Identity page mapping (P = n, physical = V, every page Backed && Dirty, page_offset 0), one active clipmap, a front-facing scene without
    overlaps: the texels the checker writes and their depths are the pixels and depths of oracle.draw_visbuffer with the same matrix."""
    import oracle

    n, ps = 8, 16
    Vp = n * ps
    s, idx = DM.flat_scene(grid_scene())
    table = np.array([[[DM.entry(y * n + x) for x in range(n)] for y in range(n)]], dtype=np.uint32)
    clip = DM.pixel_clipmaps(1, Vp)
    img = DM.draw(np.ones((Vp, Vp), np.float32), s, s.meshlet_instances, idx, [idx.numel(), 1, 0, 0, 0], table, clip, [1], page_size=ps,
                  page_table_size=n, physical_page_table_size=Vp, clipmap_count=1)
    pv = np.frombuffer(clip[:64].tobytes(), dtype=np.float32).tolist()
    vd = torch.zeros((Vp, Vp), dtype=torch.int64)
    oracle.draw_visbuffer(s, s.meshlet_instances, idx, pv, Vp, Vp, vd)
    depth, _ = oracle.resolve_visbuffer(vd)
    depth = depth.numpy()
    covered = depth > 0
    assert covered.sum() > 5000
    assert np.array_equal(img < 1.0, covered)
    assert np.array_equal(img[covered].view(np.uint32), depth[covered].view(np.uint32))


# ---- the path predictor and the hand-written frames of tests/vsm_draw_frames.py ----------------------------------------------------------------------
import pytest  # noqa: E402

import vsm_draw_frames as VF  # noqa: E402
import vsm_pages_model as VM  # noqa: E402


@pytest.mark.parametrize("name", sorted(VF.all_frames()))
def test_every_frame_sits_on_its_intended_path(name):
    """`intent`: the setup snaps the frame's corners to exactly the 1/256-px integers it was written for; `expect`: predict gives every
    triangle the path (and drawable-page and tile counts) the frame claims, in its first active clipmap."""
    vf = VF.all_frames()[name]
    rows = vf.first_clipmap()
    for t, want in enumerate(vf.intent or []):
        assert sorted(zip(rows[t]["X"], rows[t]["Y"])) == sorted(zip(*want)), (name, t, rows[t], want)
    for t, want in enumerate(vf.expect or []):
        if want is None:
            continue
        path, pages, tiles = want if isinstance(want, tuple) else (want, None, None)
        assert rows[t]["path"] == path, (name, t, rows[t])
        assert pages is None or (rows[t]["pages"], rows[t]["tiles"]) == (pages, tiles), (name, t, rows[t])
    st = vf.model()[1]
    kept = [r for r in vf.predict() if r["path"] != DM.DROPPED]
    assert st["pairs"] == len(kept) and st["big_pairs"] == sum(r["path"] in (DM.DIRECT, DM.TILED) for r in kept) and st["tiles"] == sum(r["tiles"] for r in kept)


def test_predict_splits_on_the_box_and_the_spread_but_on_the_box_alone_behind_the_clipper():
    pm = np.zeros((8, 8, 2), np.int64)
    X, Y = np.array([[0, 2048, 0], [-2048, 2048, 2048], [-2047, 2048, 2048]]), np.array([[0, 0, 2048], [256, 256, 2304], [256, 256, 2304]])
    k = DM.classify(X, Y, 128, pm, 16)
    assert k["spread"].tolist() == [2048, 4096, 4095] and k["small"].tolist() == [True, False, True] and k["big"].tolist() == [False, True, False]
    assert DM.classify(X, Y, 128, pm, 16, from_clipper=[True] * 3)["small"].tolist() == [True] * 3
    pm[...] = -1
    assert not DM.classify(X, Y, 128, pm, 16)["kept"].any()


def test_direct_or_tiled_follows_the_cut_page_box():
    """The box is cut to the rectangle of the clipmap's drawable pages before its pages are counted: one drawable page under a triangle over
    the whole 16 x 16-page viewport is a 1-page box (direct); two in opposite corners make a 256-page box (tiled, 2 tiles)."""
    X, Y = np.array([[0, 0, 2 * 65536]]), np.array([[0, 2 * 65536, 0]])
    pm = np.full((16, 16, 2), -1, np.int64)
    pm[5, 9] = 0
    k = DM.classify(X, Y, 256, pm, 16)
    assert (k["pages"][0], k["box_pages"][0], bool(k["tiled"][0]), k["tiles"][0]) == (1, 1, False, 0)
    pm[15, 15] = pm[0, 0] = 0
    k = DM.classify(X, Y, 256, pm, 16)
    assert (k["pages"][0], k["box_pages"][0], bool(k["tiled"][0]), k["tiles"][0]) == (3, 256, True, 3)


def test_the_stride_frames_make_every_loop_step_with_one_block():
    assert VF.RF.STRIDE_INSTANCES > 256 and set(VF.RF.STRIDE_COUNTS) == {255, 256, 257, 512, 513, 769, 1025}
    for n in VF.RF.STRIDE_COUNTS:
        st = VF.stride_frame(n).model()[1]
        assert st["pairs"] == n and st["big_pairs"] == st["clipped_pairs"] == 0  # every triangle on the in-wave path
    assert VF.clip_stride_frame().model()[1]["clipped_pairs"] == 136 >= 130  # three steps of one 64-thread block
    st = VF.big_stride_frame().model()[1]
    assert st["big_pairs"] >= 9 and st["tiles"] >= 9 and any(r["path"] == DM.DIRECT for r in VF.big_stride_frame().predict())
    n = VF.wide_table_frame().shape[0]
    assert n * n // 32 == 288 > 256
    assert any((y * n + x) // 32 >= 256 for c in range(2) for y, x in zip(*np.nonzero(VF.wide_table_frame().table[c] & 6 == 6)))


@pytest.mark.parametrize("n", VF.BITMAP_NS)
def test_the_bitmap_frames_put_their_page_where_they_say(n):
    for which, want in zip(VF.BITMAP_BITS, (lambda b: b == 0, lambda b: b == 31, lambda b: 0 < b < 31)):
        vx, vy = VF.bitmap_page(n, which)
        assert want((vy * n + vx) & 31) and (vy * n) >> 5 != (vy * n + n - 1) >> 5
        assert VF.bitmap_frame(n, which, 0).model()[1]["pairs"] == 1
    assert VF.bitmap_frame(n, "mid", 16).model()[1]["pairs"] == 0  # address P * P: no page
    assert VF.corners_frame(n).model()[1]["pairs"] == 3


def test_the_box_shape_frame_covers_every_shape_and_fills_its_waves_as_claimed():
    vf = VF.box_shapes_frame()
    rows = vf.first_clipmap()
    assert {(r["bw"], r["bh"]) for r in rows.values() if r["path"] == DM.SMALL_PATH} == {(w, h) for w in range(1, 9) for h in range(1, 9)}
    cnt = [rows[t]["bw"] * rows[t]["bh"] if rows[t]["path"] == DM.SMALL_PATH else 0 for t in range(len(rows))]
    waves = [cnt[i:i + 64] for i in range(0, len(cnt), 64)]
    assert len(waves) == 2 and sum(waves[0]) > 64
    assert waves[0][0] == 0 and waves[1][-1] == 0 and any(a and not b and c for w in waves for a, b, c in zip(w, w[1:], w[2:]))


def test_the_threshold_frames_sit_on_both_sides_of_each_switch():
    c = VF.threshold_frames()
    rows = c["spread-4095-4096"].first_clipmap()
    assert [rows[t]["spread"] for t in range(8)] == [4095] * 4 + [4096] * 4 and all(rows[t]["bw"] <= 8 and rows[t]["bh"] <= 8 for t in range(8))
    assert c["spread-4095-4096"].model()[1]["big_pairs"] == 4
    for s in (32767, 32768):
        rows = c[f"spread-{s}"].first_clipmap()
        assert [rows[t]["spread"] for t in range(4)] == [s] * 4
    rows = c["box-8x8-9x8-8x9"].first_clipmap()
    assert [(rows[t]["bw"], rows[t]["bh"]) for t in range(3)] == [(8, 8), (9, 8), (8, 9)]


def test_the_page_count_frames_sit_on_both_sides_of_each_switch():
    c = VF.direct_tiled_frames()
    box = {k: v.first_clipmap()[0]["box_pages"] for k, v in c.items()}
    assert box == {"4-pages": 16, "5-pages": 16, "64-page-box": 64, "72-page-box": 72, "65-page-box": 65, "second-batch": 81}
    t = c["second-batch"].table[0]
    inside = [(x, y) for y, x in zip(*np.nonzero(t & 6 == 6)) if 1 <= x <= 9 and 1 <= y <= 9]
    assert len(inside) == 3 and all((y - 1) * 9 + (x - 1) >= 64 for x, y in inside)  # the first batch of 64 pages holds none


def test_the_overflow_frames_overflow_what_they_claim():
    c = {k: v.model()[1] for k, v in VF.overflow_frames().items()}
    cap = VF.CAPACITY
    assert c["tiles"]["tiles"] == 150 > 2 * cap > 100 and c["tiles"]["big_pairs"] == 3
    assert c["big"]["big_pairs"] > cap >= c["big"]["clipped_pairs"] > 0 and c["big"]["tiles"] == 0
    assert any(r["fan"] >= 0 and r["path"] == DM.DIRECT for r in VF.overflow_frames()["big"].predict())  # some big pairs come from the clipper
    assert c["clip"]["clipped_pairs"] > cap and c["clip"]["big_pairs"] == 0
    assert c["big-and-clip"]["clipped_pairs"] > cap and c["big-and-clip"]["big_pairs"] > cap and c["big-and-clip"]["tiles"] == 0
    assert not any(r["fan"] >= 0 and r["path"] in (DM.DIRECT, DM.TILED) for r in VF.overflow_frames()["big-and-clip"].predict())


@pytest.mark.parametrize("n", VF.OFFSET_NS)
def test_the_wrap_of_extreme_page_offsets(n):
    """floor_mod(v + page_offset, n) in unbounded integers: vsm_pages_model.wrap works in int64 whatever its inputs' types, so int32 offsets
    at either end of their range do not overflow; page_map reads the entries that puts under each virtual page."""
    v = np.arange(n)
    for off in VF.offset_values(n):
        want = [(int(x) + off) % n for x in v]
        assert VM.wrap(v, off, n).tolist() == want
        assert VM.wrap(v.astype(np.int32), np.int32(off), n).tolist() == want
        assert VM.wrap(np.int32(n - 1), np.array([off], np.int32), n).tolist() == [(n - 1 + off) % n]
    for i in range(8):
        vf = VF.offset_frame(n, i)
        ox, oy = VF.offset_values(n)[i], VF.offset_values(n)[(i + 3) % 8]
        assert VM.unpack_clipmaps(vf.clipmaps)[1][0].tolist() == [ox, oy]
        pm = DM.page_map(vf.table, vf.clipmaps, 1, n, 16, vf.shape[2])[0]
        addr = pm[..., 1] * (vf.shape[2] // 16) + pm[..., 0]
        assert len(set(addr.reshape(-1).tolist())) == n * n
        for vy, vx in ((0, 0), (n - 1, 0), (3, n - 2)):
            assert addr[vy, vx] == vf.table[0, (vy + oy) % n, (vx + ox) % n] >> 16


def test_negative_zero_fragments_are_kept_and_lower_no_positive_value():
    vf = VF.neg_zero_frame()
    img, st = vf.model()
    before, after = vf.image.view(np.uint32), img.view(np.uint32)
    changed = before != after
    assert st["fragments"] > 100 and st["big_pairs"] == 1 and changed.sum() > 20
    assert (before[changed] == np.float32(-1.0).view(np.uint32)).all() and (after[changed] == VF.NEG_ZERO_BITS).all()


def test_depth_from_binary16_around_one():
    vf = VF.half_depth_frame()
    img = vf.model()[0]
    assert set(np.unique(img).tolist()) >= {1.0, 2.0} and img.max() == 2.0
    assert not any(r["path"] == DM.DROPPED for r in vf.predict())  # the page test keeps all eight; the depth test decides
    per = []
    for k in range(4):  # each meshlet alone
        one = VF.VFrame(vf.frame, vf.shape, vf.table, image=vf.image, draw=[(k, k, 0), (k, k, 1)])
        per.append(one.model()[1]["fragments"])
    assert per[0] > 200 and per[1] == 0 and 0 < per[2] < per[0] and per[2] < per[3] < per[0], per


@pytest.mark.parametrize("name", ["nan", "inf"])
def test_a_triangle_with_a_non_finite_vertex_is_dropped_whole(name):
    vf = VF.all_frames()[name]
    img, st = vf.model()
    assert st["pairs"] == 2 and st["clipped_pairs"] == 1  # it crosses every plane's test, and nothing comes out of the clipper
    alone = VF.VFrame(vf.frame, vf.shape, vf.table, draw=[vf.frame.draw[0], vf.frame.draw[2]])
    assert np.array_equal(alone.model()[0], img) and alone.model()[1]["fragments"] == st["fragments"] > 40


@pytest.mark.parametrize("s", [8, 40])
def test_a_shared_edge_with_opposite_windings_is_covered_once(s):
    vf = VF.shared_edge_frame(s)
    rows = vf.first_clipmap()
    area = lambda r: (r["X"][1] - r["X"][0]) * (r["Y"][2] - r["Y"][0]) - (r["Y"][1] - r["Y"][0]) * (r["X"][2] - r["X"][0])  # noqa: E731
    assert area(rows[0]) > 0 and area(rows[1]) > 0  # oriented; the list winds them oppositely:
    w = DM.fetch_world(vf.frame.scene, vf.frame.scene.meshlet_instances, vf.indices())
    sign = [np.sign((t[1, 0] - t[0, 0]) * (t[2, 1] - t[0, 1]) - (t[1, 1] - t[0, 1]) * (t[2, 0] - t[0, 0])) for t in w]
    assert sign[0] == -sign[1] != 0
    assert vf.model()[1]["fragments"] == s * s


def test_the_limit_frame_reaches_the_largest_viewport():
    vf = VF.limit_frame()
    assert vf.V == 16384 and int(((vf.table & 6) == 6).sum()) == 16
    img, st = vf.model()
    assert st["clipped_pairs"] == 2 and st["big_pairs"] >= 3 and st["fragments"] > 10000
    rows = vf.predict()
    assert max(max(abs(v) for v in r["X"] + r["Y"]) for r in rows) > 32 * 16384 * 256  # the guard band's fixed-point range is reached
    assert {r["clipmap"] for r in rows if r["path"] != DM.DROPPED} == {0, 1}
