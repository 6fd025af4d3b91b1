"""The checker of oxc_draw_terrain (tests/terrain_draw_model.py) against hand-worked values, its own invariants and the golden fixture.  CPU only."""
import numpy as np
import pytest

import terrain_decode_frames as DF
import terrain_draw_frames as FR
import terrain_draw_model as TM

F = np.float32
JUST_ABOVE_3 = np.array(0x40400001, np.uint32).view(np.float32)


# ---- T3 ------------------------------------------------------------------------------------------------------------------------------------------
def test_hand_worked_subdivisions():
    assert TM.subdivide(1.0)[0] == 1 and TM.subdivide(1.0)[1].tolist() == [0.0, 1.0]
    n, t = TM.subdivide(1.5)  # fc = 1.5, n = 3, r = 2/3, s = (1 - 2/3) / 2
    r = F(1) / F(1.5)
    assert n == 3 and t.tolist() == [0.0, float((F(1) - r) * F(0.5)), float(F(1) - (F(1) - r) * F(0.5)), 1.0]
    n, t = TM.subdivide(3.0)  # three equal segments
    third = F(1) / F(3)
    assert n == 3 and t[1] == (F(1) - third) * F(0.5) and t[2] == F(1) - t[1] and abs(float(t[1]) - 1 / 3) < 1e-7
    n, t = TM.subdivide(JUST_ABOVE_3)  # n jumps to 5: two end segments of about 2^-25, three of about 1/3
    assert n == 5 and 0 < t[1] < 1e-7 and t[4] == F(1) - t[1] and abs(float(t[2]) - 1 / 3) < 1e-6 and t[3] == F(1) - t[2]
    n, t = TM.subdivide(62.5)
    r = F(1) / F(62.5)
    assert n == 63 and t[1] == (F(1) - F(61) * r) * F(0.5) and t[2] == t[1] + r and t[31] == t[1] + F(30) * r and t[32] == F(1) - t[31]
    for f in (63.0, 64.0, 1000.0, float("inf")):  # clamped at 63: 63 equal segments
        n, t = TM.subdivide(f)
        assert n == 63 and np.abs(np.diff(t.astype(np.float64)) - 1 / 63).max() < 2e-7
    for f in (0.0, -2.0, float("nan")):  # T3 alone clamps these to one segment (T2 discards the patch before)
        assert TM.subdivide(f)[0] == 1
    for f in (1.0, 1.5, 2.0, 3.0, float(JUST_ABOVE_3), 4.5, 17.25, 62.5, 63.0):
        n, t = TM.subdivide(f)
        assert n % 2 == 1 and len(t) == n + 1 and t[0] == 0 and t[n] == 1 and (np.diff(t) >= 0).all()


def test_projection_scale_helpers_agree():
    from oxylus_amd.renderer import terrain_projection_scale

    for res, fov in ((2160, 60.0), (1080, 90.0), (19, 53.13)):
        assert terrain_projection_scale(res, fov) == TM.projection_scale(res, fov)
    assert TM.projection_scale(1080, 90.0) == 540.0


# ---- T4 ------------------------------------------------------------------------------------------------------------------------------------------
LADDER = [(1, 1, 1, 1), (63, 1, 1, 1), (1, 63, 1, 1), (3, 3, 3, 3), (1.5, 2.5, 7.25, 4.0), (63, 63, 63, 63), (5, 1, 1, 1), (2.0, 9.5, 2.0, 31.0), (1, 1, 1, 6.5)]


@pytest.mark.parametrize("e4", LADDER)
def test_triangle_count_and_exact_cover_of_the_square(e4):
    """The count formula, every triangle counter-clockwise or degenerate, and every lattice point covered exactly once in exact integers."""
    lists, redone = TM.lists_of([F(e) for e in e4])
    ns = [n for n, _ in lists]
    u, v, tris = TM.topology(lists)
    if all(n == 1 for n in ns):
        assert len(tris) == 2 and redone == 0
    else:
        assert len(tris) == TM.triangle_count(ns) <= 7938
        assert ns[4] >= 3 and ns[5] >= 3
    if e4 == (63, 1, 1, 1):
        assert ns[:4] == [63, 1, 1, 1] and ns[4] == 3 and ns[5] == 63 and redone == 1  # one edge 63 against an inner 3 redone from 1
    if e4 == (63, 63, 63, 63):
        assert len(tris) == 7938
    cover = TM.lattice_coverage(u, v, tris, 16 if len(tris) > 1000 else 32)
    assert (cover == 1).all(), (e4, np.argwhere(cover != 1)[:4])


def test_every_ring_side_with_each_list_exhausted_first():
    """Every side takes outer steps, inner steps and ties, and runs out of inner points first.  The outer list cannot run out first: its
    last parameter is 1 and every inner parameter is below 1, so the step onto it is never taken while an inner point is left."""
    counts = {}
    for e4 in LADDER + [(9, 9, 9, 9), (2.5, 2.5, 2.5, 2.5)]:
        TM.topology(TM.lists_of([F(e) for e in e4])[0], counts)
    for side in range(4):
        for k in ("outer_steps", "inner_steps", "inner_exhausted_first", "ties"):
            assert counts.get(f"side{side}_{k}", 0) > 0, (side, k, counts)
        assert counts.get(f"side{side}_outer_exhausted_first", 0) == 0
    assert counts["patches_all_one"] == 1


# ---- T5 ------------------------------------------------------------------------------------------------------------------------------------------
def test_shared_edge_points_are_bit_identical():
    """Patches 0 | 1 (a u = 1 / u = 0 edge) and 1 | 4 (a v = 1 / v = 0 edge) of the 3 x 2 grid, with different interiors."""
    T, hm = FR.terrain((3, 2), target_edge_pixels=6.0), FR.heightmap()
    cam = FR.camera("oblique", 129, 65)
    patch = {}
    for p in (0, 1, 4):
        cs = TM.corners(T, hm, p)
        lists, _ = TM.lists_of(TM.factors(T, cam, cs))
        patch[p] = (cs, lists)
    assert [n for n, _ in patch[0][1]][4:] != [n for n, _ in patch[1][1]][4:]
    for (pa, ea, ua, va), (pb, eb, ub, vb) in ((((0, 2, 1.0, None)), (1, 0, 0.0, None)), ((1, 3, None, 1.0), (4, 1, None, 0.0))):
        (csa, la), (csb, lb) = patch[pa], patch[pb]
        ta, tb = la[ea][1], lb[eb][1]
        assert ta.tobytes() == tb.tobytes() and len(ta) > 2
        full = lambda x, t: np.full(len(t), x, np.float32)  # noqa: E731
        wa = TM.domain_points(T, hm, csa, full(ua, ta) if ua is not None else ta, full(va, ta) if va is not None else ta)
        wb = TM.domain_points(T, hm, csb, full(ub, tb) if ub is not None else tb, full(vb, tb) if vb is not None else tb)
        assert wa.tobytes() == wb.tobytes()


# ---- whole frames -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["ground", "oblique"])
@pytest.mark.parametrize("tep", [16.0, 1.0])
def test_a_frame_of_ground_has_no_uncovered_pixel(cam, tep):
    """Watertight seams and T6's facing: every pixel is a terrain texel with a depth in (0, 1]."""
    counts = {}
    w = FR.want(FR.frame((33, 19), (3, 2), cam, target_edge_pixels=tep), counts)
    assert (w["vis"] == TM.VIS).all() and (w["depth"] > 0).all() and (w["depth"] <= 1).all()
    assert counts["patches_drawn"] == 6 and counts["set_up"] > 0
    assert counts["fragments"] >= 33 * 19  # every pixel at least once; more where triangles overlap in depth


def test_seen_from_below_the_ground_is_culled():
    w = FR.want(FR.frame((33, 19), (3, 2), "below", target_edge_pixels=4.0))
    assert (w["vis"] != TM.VIS).mean() > 0.9


def test_counts_and_discards():
    counts = {}
    FR.want(FR.frame((17, 9), (3, 2), "ground", max_tessellation=0.0), counts)
    assert counts["patches_discarded"] == 6 and counts["patches_drawn"] == 0 and counts["triangles"] == 0
    counts = {}
    FR.want(FR.frame((17, 9), (3, 2), "ground", visible=[5, 6, 1], draw_cmd=[4, 5, 0, 1]), counts)
    assert counts["patches_skipped"] == 4 and counts["patches_drawn"] == 1  # index 6, and three entries past the list's end


def test_golden_fixture():
    z = np.load(FR.GOLDEN)
    f = FR.golden_frame()
    assert f.heightmap.tobytes() == z["heightmap"].tobytes() and f.cam.projection_view.tobytes() == z["pv"].tobytes()
    assert f.visible.tobytes() == z["visible"].tobytes() and f.draw_cmd.tobytes() == z["draw_cmd"].tobytes() and f.before.tobytes() == z["before"].tobytes()
    w = FR.want(f)
    for k in FR.OUTPUTS:
        assert w[k].tobytes() == z["out_" + k].tobytes(), k
    assert (w["vis"] == TM.VIS).all()


# ---- against the ray-marched stand-in of the decode tests ---------------------------------------------------------------------------------------------
# Measured here on the CPU (the figures are printed): with triangles under a pixel the tessellated surface is the bilinear heightmap sampled at the
# domain points, the stand-in the same surface ray-marched in binary64.  Largest |depth difference| over the four frames below: 1.26e-6 in
# reverse-Z depth (values near 5e-4; 3.2e-7, 1.26e-6, 4.9e-8 and 2.0e-7 per frame), so the bound is 4 x that, the project's habit for
# checker-accuracy bounds.
DEPTH_BOUND = 4 * 1.26e-6


@pytest.mark.parametrize("extent", [(17, 9), (33, 19)])
@pytest.mark.parametrize("grid", [(3, 2), (8, 8)])
def test_agrees_with_the_ray_marched_stand_in(extent, grid):
    W, H = extent
    T = FR.terrain(grid, target_edge_pixels=0.02)
    pv, ipv = DF.camera(W, H)
    cam = FR.camera("down", W, H)
    assert cam.projection_view.tobytes() == pv.tobytes()
    vis_s, depth_s = DF.draw(T, FR.heightmap(), W, H, pv, ipv)
    w = FR.want(FR.frame(extent, grid, cam, target_edge_pixels=0.02))
    on_map = w["vis"] == TM.VIS
    # off the map's silhouette: pixels whose 3 x 3 neighbourhood is all terrain in the drawn frame
    pad = np.pad(on_map, 1, constant_values=False)
    interior = np.ones_like(on_map)
    for dy in range(3):
        for dx in range(3):
            interior &= pad[dy:dy + H, dx:dx + W]
    assert interior.any() and (vis_s[interior] == w["vis"][interior]).all()
    diff = np.abs(w["depth"].astype(np.float64) - depth_s.astype(np.float64))[interior].max()
    print(f"{extent} {grid}: largest |depth difference| {diff:.3e} over {int(interior.sum())} pixels")
    assert diff <= DEPTH_BOUND


def test_the_vectorised_set_up_is_raster_models():
    """terrain_draw_model._snap and the pixel box of `raster` restate the snap, the range guards, cullMode eBack and the box for many
    triangles at once; raster_model.snap / setup are the one-triangle statement.  Held equal on random triangles, tiny to beyond the image,
    some with w <= 0 and some beyond the fixed-point range."""
    import raster_model as RM

    rng = np.random.default_rng(5)
    W, H = 33, 19
    K = 600
    centre = rng.uniform(-1.4, 1.4, (K, 1, 2))
    size = 10.0 ** rng.uniform(-3, 0.5, (K, 1, 1))
    xy = centre + rng.uniform(-1, 1, (K, 3, 2)) * size
    w = rng.uniform(0.2, 3.0, (K, 3, 1))
    w[::37, 1] = -0.5
    xy[5::41] *= 1e7
    clip = np.concatenate([xy * w, rng.uniform(0.0, 1.0, (K, 3, 1)) * w, w], axis=2).astype(np.float32)
    kept, X, Y, z = TM._snap(clip, W, H)
    seen = {"dropped": 0, "kept": 0}
    for k in range(K):
        s = RM.snap(clip[k], W, H)
        t = RM.setup(s, W, H) if s is not None else None
        assert (t is not None) == bool(kept[k]), k
        seen["kept" if t is not None else "dropped"] += 1
        if t is None:
            continue
        assert X[k].tolist() == t["X"] and Y[k].tolist() == t["Y"] and z[k].tobytes() == np.array(t["z"], np.float32).tobytes(), k
        px0, py0 = max((min(t["X"]) - 128 + 255) >> 8, 0), max((min(t["Y"]) - 128 + 255) >> 8, 0)  # the box as `raster` forms it
        px1, py1 = min((max(t["X"]) - 128) >> 8, W - 1), min((max(t["Y"]) - 128) >> 8, H - 1)
        assert (px0, py0, px1, py1) == (t["px0"], t["py0"], t["px1"], t["py1"]), k
    assert seen["kept"] > 100 and seen["dropped"] > 100
