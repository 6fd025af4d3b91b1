"""oxc_draw_terrain on the GPU against tests/terrain_draw_model.py: every word of visdepth, depth and vis and every counter equal to the
checker's between poisoned guard bands (terrain_draw_frames.run)."""
import dataclasses

import numpy as np
import pytest
import torch

import terrain_draw_frames as FR
import terrain_draw_model as TM
from oxylus_amd import lib as L
from refusals import ALIGNED, NULL, SHORT, Raw, raises_refusal

pytestmark = pytest.mark.gpu
rep = dataclasses.replace
NAN = float("nan")


@pytest.fixture(scope="module")
def r(renderer):
    return renderer


@pytest.mark.parametrize("extent", FR.EXTENTS)
@pytest.mark.parametrize("grid", FR.GRIDS)
def test_extents_and_grids(r, extent, grid):
    """Mixed factors (4 px edges) under the oblique camera: inner grids, ring strips and all-one patches in one frame at the larger extents."""
    counts = {}
    FR.run(r, FR.frame(extent, grid, "oblique", target_edge_pixels=4.0), f"{extent} {grid}", counts)
    assert counts["patches_drawn"] == grid[0] * grid[1] and (counts["fragments"] > 0 or extent == (1, 1))


@pytest.mark.parametrize("name,kw,cam", [("all-one", dict(target_edge_pixels=1e6), "ground"), ("mixed", dict(target_edge_pixels=2.0), "oblique"),
                                         ("clamped at 63", dict(target_edge_pixels=1e-3), "ground"), ("max 5", dict(target_edge_pixels=1e-3, max_tessellation=5.0), "down")])
def test_factors(r, name, kw, cam):
    counts = {}
    FR.run(r, FR.frame((33, 19), (3, 2), cam, **kw), name, counts)
    if name == "all-one":
        assert counts["patches_all_one"] == 6 and counts["triangles"] == 12
    if name == "clamped at 63":
        assert counts["triangles"] == 6 * 7938  # more than one tile of the inner grid a side, every strip at its longest


@pytest.mark.parametrize("max_tessellation", [0.0, -3.0, NAN])
def test_max_tessellation_edge_values(r, max_tessellation):
    """<= 0 discards every patch (the image keeps its bytes under clear = False); a NaN loses in fminf and leaves the factor unclamped."""
    counts = {}
    f = FR.frame((17, 9), (3, 2), "ground", clear=False, max_tessellation=max_tessellation, target_edge_pixels=4.0)
    got = FR.run(r, f, f"max_tessellation {max_tessellation}", counts)
    if max_tessellation == max_tessellation:
        assert counts["patches_discarded"] == 6 and (got["visdepth"] == f.before).all()
    else:
        assert counts["patches_drawn"] == 6


def test_instance_count_zero(r):
    f = FR.frame((17, 9), (3, 2), "ground", visible=[], draw_cmd=[4, 0, 0, 0])
    got = FR.run(r, f, "instance_count 0")
    assert (got["visdepth"] == 0).all()


def test_subset_list_first_instance_and_bad_index(r):
    """A descending list read from first_instance = 2 on, with an index past the grid and the command's count reaching past the buffer."""
    counts = {}
    f = FR.frame((33, 19), (3, 2), "ground", visible=[0, 1, 5, 4, 77, 2, 0xFFFFFFFF], draw_cmd=[4, 7, 9, 2], target_edge_pixels=4.0)
    FR.run(r, f, "subset", counts)
    assert counts["patches_drawn"] == 3 and counts["patches_skipped"] == 4


@pytest.mark.parametrize("cam", ["grazing", "below"])
def test_camera_at_the_surface(r, cam):
    """Just above the surface: triangles through the camera plane (clipper), boxes beyond 8 x 8 and beyond 64 px (big list, tiles)."""
    counts = {}
    FR.run(r, FR.frame((129, 65), (3, 2), cam, target_edge_pixels=16.0), cam, counts)
    if cam == "grazing":
        assert counts["clipped"] > 0 and counts["big"] > 0
        # all-one patches from the same eye: two triangles a patch, their boxes beyond 64 px -- clipped pieces into the big list and its tiles
        FR.run(r, FR.frame((129, 65), (3, 2), cam, target_edge_pixels=1e6), cam + ", two triangles a patch")
        assert r.debug_raster_stats()["tiles"] > 0


def test_over_an_earlier_image_with_an_exact_depth_tie(r):
    """Drawn without clear over an image whose texels are the terrain's own depth with a mesh vis, one below and one above it: terrain wins
    the tie and the nearer one, loses to the farther-in-bits one."""
    base = FR.frame((33, 19), (3, 2), "ground", target_edge_pixels=4.0)
    d = FR.want(base)["visdepth"] >> np.uint64(32)
    ys, xs = np.mgrid[0:19, 0:33]
    k = (ys * 33 + xs) % 3
    before = ((d + np.where(k == 1, 1, 0).astype(np.uint64) - np.where(k == 2, 1, 0).astype(np.uint64)) << np.uint64(32)) | np.uint64(0x00012345)
    got = FR.run(r, rep(base, clear=False, before=before), "tie")
    assert (got["vis"][k == 0] == TM.VIS).all() and (got["vis"][k == 1] == 0x00012345).all() and (got["vis"][k == 2] == TM.VIS).all()


def test_early_then_late_call_without_clear(r):
    """Two halves of the list in two calls give the image of one call with all of it."""
    whole = FR.frame((33, 19), (3, 2), "oblique", target_edge_pixels=2.0)
    first = rep(whole, visible=whole.visible[:3], draw_cmd=np.array([4, 3, 0, 0], np.uint32))
    got1 = FR.run(r, first, "early")
    second = rep(whole, visible=whole.visible[3:], draw_cmd=np.array([4, 3, 0, 0], np.uint32), clear=False, before=got1["visdepth"])
    got2 = FR.run(r, second, "late")
    assert (got2["visdepth"] == FR.want(whole)["visdepth"]).all()


@pytest.mark.parametrize("blocks", [1, 3])
def test_grid_tuning(r, blocks):
    r.debug_set_tuning(L.TUNE_TERRAIN_DRAW_GRID, blocks)
    try:
        FR.run(r, FR.frame((33, 19), (8, 8), "oblique", target_edge_pixels=2.0), f"{blocks} blocks")
    finally:
        r.debug_set_tuning(L.TUNE_TERRAIN_DRAW_GRID, 0)


def test_two_identical_runs(r):
    """The counting instantiations first, then the plain kernels: the same image, small boxes, clipped pieces, big list and tiles in it."""
    f = FR.frame((129, 65), (8, 8), "grazing", target_edge_pixels=4.0)
    a, b = FR.run(r, f, "first"), FR.run(r, f, "second", stats=False)
    assert all((a[k].view(np.uint32) == b[k].view(np.uint32)).all() for k in a)


def test_captured_graph_replayed_twice(r):
    f = FR.frame((33, 19), (3, 2), "oblique", target_edge_pixels=2.0)
    gs = FR.guards(f)
    ctx = FR.context(f, gs)
    r.draw_terrain_for_visbuffer(ctx)  # the un-captured first call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.draw_terrain_for_visbuffer(ctx, stream=s)
    from gpu_passes import same

    for _ in range(2):
        gs["visdepth"].tensor.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        same(FR.got_of(gs, f), FR.want(f), "replay")


# ---- limits --------------------------------------------------------------------------------------------------------------------------------------
# changes to the filled C structure, as refusals.Raw takes them
_null = lambda field: {field: L.Buffer(None, 0)}  # noqa: E731
_shifted = lambda field, by, short=0: {field: lambda b: L.Buffer(b.dptr + by, (short or b.bytes) - by)}  # noqa: E731
_short = lambda field, need: {field: lambda b: L.Buffer(b.dptr, need - 1)}  # noqa: E731
_depth = lambda width=17, height=9, levels=1: {"depth_attachment.width": width, "depth_attachment.height": height, "depth_attachment.levels": levels}  # noqa: E731


EXTENT, MAPRES, PATCHES = "the extent must be 1 .. 16384 a side", "map_resolution: every side", "terrain.patch_count: every side"
BUFFERS = (("heightmap", 1, 24 * 20 * 2), ("visible_patches_buffer", 2, 4), ("draw_cmd_buffer", 2, 16), ("visdepth_buffer", 4, 17 * 9 * 8))
# (the fields of the filled C structure that are changed, the message, the field they touch), in the order of the header's limits paragraph
CASES = [(dict(width=0), EXTENT, "width"), (dict(width=16385), EXTENT, "width"), (dict(height=0), EXTENT, "height"), (dict(height=16385), EXTENT, "height"),
         (dict(map_resolution=(0, 20)), MAPRES, "map_resolution"), (dict(map_resolution=(24, 16385)), MAPRES, "map_resolution"),
         ({"terrain.patch_count": (0, 2)}, PATCHES, "patch_count"), ({"terrain.patch_count": (3, 4097)}, PATCHES, "patch_count")]
for _field, _by, _need in BUFFERS:
    CASES += [(_null(_field), _field + NULL, _field), (_shifted(_field, _by), _field + ALIGNED, _field), (_short(_field, _need), _field + SHORT, _field)]
CASES += [(_depth(width=16), "depth_attachment must be one R32F level", "depth_attachment"), (_depth(height=10), "depth_attachment must be one R32F level", "depth_attachment"),
          (_depth(levels=2), "depth_attachment must be one R32F level", "depth_attachment"),
          (_short("visbuffer_attachment", 17 * 9 * 4), "visbuffer_attachment smaller than width * height u32", "visbuffer_attachment")]


@pytest.fixture(scope="module")
def refusal(r):
    f = FR.frame((17, 9), (3, 2), "ground")
    gs = FR.guards(f)
    return f, gs, FR.context(f, gs)


def _refused(r, context, message, gs, f):
    raises_refusal(lambda: r.draw_terrain_for_visbuffer(context), message)
    FR.check_unwritten(gs, f, message)


def test_every_limit_on_its_own(r, refusal):
    f, gs, base = refusal
    for change, message, _ in CASES:
        _refused(r, Raw(base, **change), message, gs, f)
    FR.run(r, f, "the frame still draws")


def test_the_first_broken_rule_gives_the_message(r, refusal):
    """Every two rules broken at once, over all pairs of the header's order that touch different fields: the earlier one is named."""
    f, gs, base = refusal
    pairs = 0
    for i, (first, message, field) in enumerate(CASES):
        for later, _, other in CASES[i + 1:]:
            if other != field:
                _refused(r, Raw(base, **later, **first), message, gs, f)
                pairs += 1
    assert pairs > 200
    # within one buffer: null before aligned before small
    for field, by, need in BUFFERS:
        _refused(r, Raw(base, **_shifted(field, by, short=need - 1)), field + ALIGNED, gs, f)
    FR.run(r, f, "the frame still draws")


def test_null_context_and_short_struct_size(r, refusal):
    import ctypes as C

    f, gs, base = refusal
    lib = L.load()
    assert lib.oxc_draw_terrain(r._ctx, None, None) == L.OXC_INVALID_ARG
    assert lib.oxc_draw_terrain(None, None, None) == L.OXC_INVALID_ARG
    c = base.c()
    c.struct_size = C.sizeof(L.TerrainDrawContext) - 8
    assert lib.oxc_draw_terrain(r._ctx, C.byref(c), None) == L.OXC_INVALID_ARG
    assert b"struct_size" in lib.oxc_last_error(r._ctx)
    torch.cuda.synchronize()
    FR.check_unwritten(gs, f, "short struct_size")
