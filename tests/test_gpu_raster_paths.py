"""oxc_draw_visbuffer where random scenes do not reach: the stride loops of its kernels (OXC_TUNE_RASTER_GRID), the tile list's overflow,
each switch-over between the pixel walkers, the depth rule's ends, index counts that are no multiple of 3, and tiny and one-texel-wide
extents inside poisoned bands.  Every test draws a hand-written list (raster_frames) and compares all 64 bits of every texel with the C
checker; raster_model.predict says which walker a triangle has to take, and debug_raster_stats is held against it where it can tell."""
import numpy as np
import pytest
import torch

import raster_frames as RF
import raster_model as RM
from oxylus_amd import lib as L

pytestmark = pytest.mark.gpu

POISON64 = 0x7FC00BAD7FC00BAD  # around the packed image
FILL32, POISON32 = 0x5A5A5A5A, 0x7FC00BAD


def _draw(r, f, form=0, draw=None, count=None, instance_count=1, clear=True, visdepth=None, depth=None, visbuffer=None):
    """Uploads frame `f` with the index list of `draw` in `form`, draws `count` indices (default: all) and returns the packed image (CPU)."""
    from oxylus_amd.renderer import CullGeometryContext, PreparedFrame

    gpu = f.scene.to("cuda")
    frame = PreparedFrame.create(gpu, with_triangles=False)
    idx = f.indices(form, draw)
    frame.reordered_indices_buffer = (idx if idx.numel() else torch.zeros(6, dtype=torch.int32)).cuda()
    r.prepared_frame = frame
    n = idx.numel() // (2 if form == 2 else 1) if count is None else count
    cmd = torch.tensor([n, instance_count, 0, 0, 0], dtype=torch.int32, device="cuda")
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=0, cull_camera=gpu.cull_camera(), wide_triangle_index=form)
    got = torch.empty((f.H, f.W), dtype=torch.int64, device="cuda") if visdepth is None else visdepth
    r.draw_visbuffer(ctx, f.pv, f.W, f.H, got, clear=clear, depth=depth, visbuffer=visbuffer, draw_cmd=cmd)
    torch.cuda.synchronize()
    return got.cpu()


def _assert_same(got, want, label=""):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        y, x = bad[0].tolist()
        raise AssertionError(f"{label}: {bad.shape[0]} texels differ, the first at (x {x}, y {y}): got 0x{got[y, x].item() & (2 ** 64 - 1):016X}, want 0x{want[y, x].item() & (2 ** 64 - 1):016X}")


def _predicted(case):
    """(triangles the big list gets, tile-list items) by raster_model.predict."""
    _, setups = case.frame.model_image()
    p = [RM.predict(t) for t in setups]
    return sum(1 for k in p if k[2]), sum(k[1] for k in p)


@pytest.fixture(scope="module")
def small_renderer(oracle_lib):
    """A context whose big list holds 4096 triangles (16 per segment) and whose tile list holds 8192 items."""
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    r.debug_set_tuning(L.TUNE_RASTER_BIG_CAPACITY, 4096)
    yield r
    r.close()


@pytest.fixture
def capped(small_renderer):
    """The same context with every launch of the draw capped at one block: 4 waves, 256 triangles per grid step of k_draw_setup, 256 mesh
    instances per step of k_draw_rows, 64 queued ids per step of k_draw_clipped."""
    small_renderer.debug_set_tuning(L.TUNE_RASTER_GRID, 1)
    yield small_renderer
    small_renderer.debug_set_tuning(L.TUNE_RASTER_GRID, 0)


# ---- 1. stride loops -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2], ids=["packed", "wide", "pairs"])
@pytest.mark.parametrize("n", RF.STRIDE_COUNTS)
def test_setup_and_rows_stride_loops(capped, n, form):
    """k_draw_setup's software pipeline over 1..5 grid steps with full and partial last steps (the rotation nidx = nnidx, the next step's
    nmli, nnidx two steps ahead and their guards), k_draw_rows over 320 mesh instances with 256 threads."""
    f = RF.stride_frame()
    draw = RF.stride_draw(n)
    want = f.oracle_image(form, draw)
    _assert_same(_draw(capped, f, form, draw), want, f"{n} triangles, form {form}")
    st = capped.debug_raster_stats()
    assert st["big"] == 0 and st["clipped"] == 0 and st["tiles"] == 0, st


def test_the_cap_does_not_change_the_image(capped):
    f = RF.stride_frame()
    draw = RF.stride_draw(1025)
    want = f.oracle_image(0, draw)
    for cap in (2, 3, 0, 1):
        capped.debug_set_tuning(L.TUNE_RASTER_GRID, cap)
        _assert_same(_draw(capped, f, 0, draw), want, f"cap {cap}")


def test_clip_queue_stride_loop(capped):
    """136 triangles that cross the camera plane, 64 threads: k_draw_clipped<false> walks its queue in three steps."""
    f = RF.clipped_stride_frame()
    want = f.oracle_image()
    _assert_same(_draw(capped, f), want, "clipped stride")
    st = capped.debug_raster_stats()
    assert st["clipped"] == len(f.draw) >= 130, st


# ---- 2. tile-list overflow -------------------------------------------------------------------------------------------------------------------------
def test_tile_list_overflow(small_renderer):
    """30 x 289 = 8670 tile items for a list of 8192: the triangle that crosses the capacity has its tiles split between the list and the
    in-place walk of k_draw_big (first + k < tile_capacity), the ones after it are walked in place whole."""
    case = RF.tile_overflow_case()
    want = case.frame.oracle_image()
    got = _draw(small_renderer, case.frame)
    st = small_renderer.debug_raster_stats()
    print("tile overflow:", st)
    big, tiles = _predicted(case)
    assert st["tiles"] > 8192 and st["overflowed_segments"] == 0 and st["big"] == RF.TILE_BIG == big and st["tiles"] == tiles and st["clipped"] == 0, st
    _assert_same(got, want, "tile overflow")


# ---- 3. thresholds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RF.threshold_cases()))
def test_threshold_case(renderer, oracle_lib, name):
    case = RF.threshold_cases()[name]
    want = case.frame.oracle_image()
    got = _draw(renderer, case.frame)
    st = renderer.debug_raster_stats()
    print(name, st)
    _assert_same(got, want, name)
    big, tiles = _predicted(case)
    assert st["big"] == big and st["tiles"] == tiles and st["clipped"] == 0 and st["overflowed_segments"] == 0, (st, big, tiles)
    assert (want != 0).any()


@pytest.mark.parametrize("s", [8, 40, 200])
def test_each_half_of_the_diagonal_quad_alone(renderer, oracle_lib, s):
    f = RF.threshold_cases()[f"diagonal-{s}"].frame
    a, b = _draw(renderer, f, draw=f.draw[:1]), _draw(renderer, f, draw=f.draw[1:])
    _assert_same(a, f.oracle_image(draw=f.draw[:1]), "first half")
    _assert_same(b, f.oracle_image(draw=f.draw[1:]), "second half")
    quad = torch.zeros((f.H, f.W), dtype=torch.bool)
    quad[2:2 + s, 2:2 + s] = True
    assert torch.equal((a != 0) ^ (b != 0), quad) and not ((a != 0) & (b != 0)).any()


def test_half_depth_from_the_mesh(renderer, oracle_lib):
    f = RF.half_depth_case().frame
    want = f.oracle_image()
    _assert_same(_draw(renderer, f), want, "binary16 depth")
    assert (want[:, :8] != 0).any() and not (want[:, 8:] != 0).any()


@pytest.mark.parametrize("W,big", [(8, False), (64, True)], ids=["lane-walk", "push-big"])
def test_clipped_pieces_take_the_lane_walk_or_the_big_list(renderer, oracle_lib, W, big):
    f = RF.clipped_pair(W).frame
    want = f.oracle_image()
    got = _draw(renderer, f)
    st = renderer.debug_raster_stats()
    print("clipped pair", W, st)
    _assert_same(got, want, f"clipped pair {W}")
    assert st["clipped"] == 2 and (st["big"] > 0) == big and (want != 0).any(), st


@pytest.mark.parametrize("form", [0, 2], ids=["packed", "pairs"])
@pytest.mark.parametrize("count", [0, 1, 2, 3, 7, 8, 15])
def test_index_counts_that_are_no_multiple_of_three(renderer, oracle_lib, count, form):
    f = RF.index_count_frame().frame
    want = f.oracle_image(form, count=count)
    _assert_same(_draw(renderer, f, form, count=count), want, f"count {count}")
    assert (want != 0).any() == (count >= 3)


def test_an_empty_draw_clears_or_leaves_the_image(renderer, oracle_lib):
    f = RF.index_count_frame().frame
    pattern = torch.arange(f.W * f.H, dtype=torch.int64).view(f.H, f.W) * 0x100000001 + 7
    got = _draw(renderer, f, count=0, clear=True, visdepth=pattern.cuda())
    assert not (got != 0).any()
    got = _draw(renderer, f, count=0, clear=False, visdepth=pattern.cuda())
    assert torch.equal(got, pattern)
    got = _draw(renderer, f, form=2, instance_count=0, clear=False, visdepth=pattern.cuda())  # pairs: a wrapped cull call zeroed instanceCount
    assert torch.equal(got, pattern)
    got = _draw(renderer, f, form=2, instance_count=1, clear=False, visdepth=pattern.cuda())
    assert not torch.equal(got, pattern)


# ---- 4. extents and bands --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [False, True], ids=["packed-only", "with-resolves"])
@pytest.mark.parametrize("W,H", RF.RASTER_EXTENTS, ids=RF.RASTER_EXTENT_IDS)
def test_extent_inside_poisoned_bands(renderer, oracle_lib, W, H, outputs):
    from gpu_passes import Guard
    from oxylus_amd.renderer import ImageAttachment

    f = RF.extent_case(W, H).frame
    want = f.oracle_image()
    n, band = W * H, W + 64
    buf = torch.full((band + n + band,), POISON64, dtype=torch.int64, device="cuda")
    window = buf[band:band + n].view(H, W)
    depth = Guard("depth_attachment", (H, W), torch.float32, W, POISON32, 4, fill=FILL32) if outputs else None
    vis = Guard("visbuffer_attachment", (H, W), torch.int32, W, POISON32, 4, fill=FILL32) if outputs else None
    got = _draw(renderer, f, visdepth=window, depth=ImageAttachment.depth(depth.tensor) if outputs else None, visbuffer=vis.tensor if outputs else None)
    _assert_same(got, want, f"{W}x{H}")
    host = buf.cpu()
    assert (host[:band] == POISON64).all() and (host[band + n:] == POISON64).all(), "a band of the packed image changed"
    if outputs:
        w64 = want.numpy().view(np.uint64)
        want_depth, want_vis = (w64 >> np.uint64(32)).astype(np.uint32), (w64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        depth.check(f"{W}x{H}", want_depth)
        vis.check(f"{W}x{H}", want_vis)
        assert np.array_equal(depth.bits()[1].reshape(H, W), want_depth) and np.array_equal(vis.bits()[1].reshape(H, W), want_vis)
    assert (want != 0).all()
