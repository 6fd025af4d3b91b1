"""Without a GPU: the fixtures of tests/test_gpu_terrain_cull.py are not degenerate.  Each HiZ shape's terrain meets the conditions of
terrain_cull_frames.assert_exercised (or drops one with a stated reason), the flag-set terrain holds every class of patch, the seam grids
reach their totals, and the numpy restatement of the kernel's box rule sees the boxes the checker sees ("Terrain cull shapes
pinned by the tests").  `pytest -s` prints the counts."""
import numpy as np
import pytest
import torch

from hiz_frames import SHAPE_BY_ID, SHAPES
from terrain_cull_frames import (EDGE_CASES, EDGE_ROWS, FLAG_SETS, FRUSTUM, LATE, OCCLUSION, PASSES, SEAM_GRIDS, SEAM_TOTALS, World, _camera, _mask, _terrain,
                                 assert_exercised, checker, dropped_conditions, edge_case, edge_minmax, flag_classes, flag_frame, patch_boxes, shape_report, shape_want,
                                 small_pyramid, two_pass_want)


@pytest.mark.parametrize("shape_id", [s.id for s in SHAPES])
def test_terrain_exercises_the_pyramid(oracle_lib, shape_id):
    """Every level chosen, all four edge clamps, a raw mip beyond the top where the shape allows, 5 .. 95 % of the frustum survivors occluded;
    exercise_report itself asserts that the boxes it derives are the ones the checker's terrain cull sees."""
    shape, rep = SHAPE_BY_ID[shape_id], shape_report(shape_id)
    assert_exercised(shape, rep)
    lists, _ = shape_want(shape_id)
    assert lists[0].numel() > 0 and lists[1].numel() > 0
    print(f"\n{shape_id}: survivors {rep['survivors']}, none {rep['none']}, occluded {rep['removed']} ({rep['occluded']:.1%}), levels {sorted(rep['levels'])}, "
          f"edges {''.join(sorted(rep['edges']))}, exceeds {rep['exceeds']}, early {lists[0].numel()}, late {lists[1].numel()}, dropped {sorted(dropped_conditions(shape_id))}")


def test_every_dropped_condition_gives_its_reason():
    for s in SHAPES:
        for cond, why in dropped_conditions(s.id).items():
            assert cond in ("levels", "edges", "exceeds") and len(why) > 20, (s.id, cond)


def test_flag_set_terrain_holds_every_class_of_patch(oracle_lib):
    """Behind the camera, across the near plane (project_aabb returns none), emitted early, emitted late only, occluded, outside the frustum:
    at least 10 patches each, and the camera inside one patch's box."""
    classes = flag_classes()
    print("\n", classes)
    assert classes.pop("camera inside")
    assert all(n >= 10 for n in classes.values()), classes


def test_flag_sets_differ_from_each_other(oracle_lib):
    """The eight flag sets are not eight names for fewer behaviours: the emitted lists and masks take at least five distinct values, flags 0
    emits exactly the previously visible patches, and no set without OCCLUSION or LATE writes the mask."""
    world, mm, cam, pyr, mask, _ = flag_frame()
    seen = set()
    for flags in FLAG_SETS:
        m = mask.clone()
        lst = checker(world, mm, cam, flags, pyr.struct(), m)
        seen.add((tuple(lst.tolist()), tuple(m.tolist())))
        if not flags & (OCCLUSION | LATE):
            assert torch.equal(m, mask)
        if flags == 0:
            bits = (mask.view(-1, 1) >> torch.arange(32)) & 1
            assert lst.tolist() == torch.nonzero(bits.flatten()[:world.total]).flatten().tolist()
    assert len(seen) >= 5
    # LATE without FRUSTUM: boxes behind the camera reach project_aabb, return none and stay visible
    m = mask.clone()
    assert checker(world, mm, cam, LATE, pyr.struct(), m).numel() > checker(world, mm, cam, FRUSTUM | LATE, pyr.struct(), mask.clone()).numel() + 1000


def test_seam_grids_reach_their_totals(oracle_lib):
    by_total = {}
    for g in SEAM_GRIDS:
        by_total.setdefault(g[0] * g[1], []).append(g)
    assert tuple(sorted(by_total)) == SEAM_TOTALS
    for total, grids in by_total.items():
        assert any(1 in g for g in grids), total                      # a single row or column
        assert total in (1, 31) or any(1 not in g for g in grids), total  # and a 2-D grid where it factors (31 is prime)
    for g in SEAM_GRIDS:
        _, mask, lists, masks = two_pass_want(World(g), 100 + g[0], 7, True)
        if g[0] * g[1] >= 31:
            assert 0 < lists[0].numel() < g[0] * g[1] and 0 < lists[1].numel() < g[0] * g[1], g
            assert not torch.equal(masks[1], mask), g  # (thin strips all pass the early tests; the late pass adds the patches not seen before)


def test_patch_boxes_restate_the_kernel_rule(oracle_lib):
    """patch_boxes against hand-worked binary32 values: patch (1, 0) of a 3 x 2 grid on [-30, 60] x [10, 50], min / max {0.25, 0.75} and a flat
    patch; and the NaN / inverted rows of the edge image fall back to 1e-3."""
    f = np.float32
    mm = torch.tensor([[[0.0, 1.0], [0.25, 0.75], [0.5, 0.5]], [[0.0, 1.0]] * 3])
    c, e = patch_boxes(World((3, 2), (-30.0, 10.0), (90.0, 40.0), 2.0, 8.0), mm)
    x0, x1 = f(-30) + (f(1) / f(3)) * f(90), f(-30) + (f(2) / f(3)) * f(90)
    assert c[1].tolist() == [(x0 + x1) * f(0.5), f(2) + f(0.5) * f(8), f(20)] and e[1].tolist() == [x1 - x0, f(4), f(20)]
    assert e[2, 1] == f(1e-3) and c[2, 1] == f(6)
    world, _ = edge_case("height_scale-minus60")
    _, e = patch_boxes(world, edge_minmax())
    e = e.reshape(31, 33, 3)
    for row, what in EDGE_ROWS.items():
        if what in ("min == max", "NaN min", "NaN max", "NaN both", "+Inf both", "-0.0 both"):
            assert (e[row, :, 1] == f(1e-3)).all(), what
    assert (e[5, :, 1] > f(1e-3)).all()  # min > max under a negative scale: a positive height again


def test_edge_cases_decide_something(oracle_lib):
    """Each parameter set of the edge image emits some patches and culls some, in both passes."""
    hz = small_pyramid(96, 40, 4).struct()
    for name in EDGE_CASES:
        world, cam = edge_case(name)
        m = _mask(world.total, 3, 0.35)
        for flags in PASSES:
            n = checker(world, edge_minmax(), cam, flags, hz, m).numel()
            assert 0 < n < world.total, (name, flags, n)

