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
