"""oxc_build_meshlet_bounds where random meshes do not reach: the chunk seam (first != 0), the stride loops of the gather kernel, the
partial fold and the quantiser (OXC_TUNE_BOUNDS_CHUNK / OXC_TUNE_BOUNDS_GRID, and once at the real constants), every triangle-count
switch-over, the cone's decision thresholds, signed zeros across passes, threads and partial blocks, stale scratch rows, and
coordinates at the ends of binary32.  Every test runs a hand-assembled frame of bounds_frames and demands byte identity with the C
checker on the records, the quantised positions and the mesh box (compared as uint32)."""
import functools

import numpy as np
import pytest
import torch

import bounds_frames as BF
from oxylus_amd import lib as L

pytestmark = pytest.mark.gpu

CHUNKS, GRIDS = (1, 4, 5), (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _frames():
    f = {"count_ladder": BF.count_ladder(), "cone_thresholds": BF.cone_thresholds()}
    f.update({"signed_zeros/" + k: v for k, v in BF.signed_zeros().items()})
    f.update({"edge_values/" + k: v for k, v in BF.edge_values().items()})
    return f


SIGNED = ["signed_zeros/" + k for k in ("meshlets", "mesh_first_plus", "mesh_first_minus", "mesh_late_plus", "mesh_late_minus", "mesh_alternating")]
EDGES = ["edge_values/" + k for k in ("huge", "tiny", "fltmax", "nan", "posinf", "neginf", "bothinf", "half_bounds")]


@functools.lru_cache(maxsize=None)
def _want(name):
    """The checker's outputs for a frame, computed once and shared."""
    import oracle

    f = _frames()[name] if name in _frames() else _many_small(int(name))
    b, m6, q = oracle.build_meshlet_bounds(*f.args())
    return b.numpy().view(np.uint16), m6.numpy().view(np.uint32), q.numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _many_small(n):
    return BF.many_small(n)


@pytest.fixture(scope="module")
def bounds_renderer(oracle_lib):
    """A context of this module's own: its bounds scratch grows with these tests only."""
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    yield r
    r.close()


def _run(r, f):
    b, m6, q = r.build_meshlet_bounds(*f.cuda_args())
    torch.cuda.synchronize()
    return b.cpu().numpy().view(np.uint16), m6.cpu().numpy().view(np.uint32), q.cpu().numpy().view(np.uint16)


def _assert_same(got, want, label):
    (gb, gm, gq), (wb, wm, wq) = got, want
    if not np.array_equal(gb, wb):
        bad = np.flatnonzero((gb != wb).any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{label}: {len(bad)} records differ, the first is meshlet {i}: got {[hex(v) for v in gb[i]]}, want {[hex(v) for v in wb[i]]}")
    assert np.array_equal(gm, wm), f"{label}: mesh box got {[hex(v) for v in gm]}, want {[hex(v) for v in wm]}"
    assert np.array_equal(gq, wq), f"{label}: quantised positions differ"


def _tuned(r, chunk, grid):
    r.debug_set_tuning(L.TUNE_BOUNDS_CHUNK, chunk)
    r.debug_set_tuning(L.TUNE_BOUNDS_GRID, grid)


# ---- every fixture at the default tunings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["count_ladder", "cone_thresholds"] + SIGNED + EDGES)
def test_frames_match_the_checker(bounds_renderer, name):
    _assert_same(_run(bounds_renderer, _frames()[name]), _want(name), name)


# ---- chunk seam and stride loops with small frames -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["count_ladder"] + SIGNED)
def test_chunk_and_grid_tunings_do_not_change_a_byte(bounds_renderer, name):
    """Chunks of 1, 4 and 5 meshlets (first != 0 in all but the first, a ragged last one; a chunk of 1 puts every meshlet's normals into
    scratch row 0, behind which the previous meshlet's longer row is stale) under a gather grid of 1, 2, 3 blocks (4, 8, 12 meshlets per
    stride step) and a partial fold of 1, 2, 3 blocks whose threads fold meshlets 256, 512, 768 apart.  The mesh box is the same bytes
    for every setting: it equals the checker's each time."""
    f, want = _frames()[name], _want(name)
    try:
        for chunk in CHUNKS:
            for grid in GRIDS:
                _tuned(bounds_renderer, chunk, grid)
                _assert_same(_run(bounds_renderer, f), want, f"{name}, chunk {chunk}, grid {grid}")
        for chunk, grid in ((0, 1), (5, 0), (1 << 20, 2)):  # each knob alone; a chunk above 2^18 is clamped
            _tuned(bounds_renderer, chunk, grid)
            _assert_same(_run(bounds_renderer, f), want, f"{name}, chunk {chunk}, grid {grid}")
    finally:
        _tuned(bounds_renderer, 0, 0)


def test_small_call_after_a_large_one_ignores_the_stale_scratch(oracle_lib):
    """The scratch is laid out by its capacity: after a call with 3001 meshlets a call with the first 40 of the SAME meshlet array finds
    the first call's boxes, normals and counts behind its own rows (and, in the rows it rewrites, stale normals behind the valid ones,
    which the one-lane cone code loads in blocks of 8 but must not use).  A fresh context, so that the capacity is this test's."""
    from oxylus_amd.renderer import RendererInstance

    big = _many_small(3001)
    ladder = _frames()["count_ladder"]
    r = RendererInstance(0)
    try:
        _assert_same(_run(r, big), _want("3001"), "large call")
        small = BF.Frame("first 40", big.positions, big.meshlets[:40].contiguous(), big.vidx, big.micro)
        wb, _, wq = _want("3001")
        import oracle

        m6 = oracle.build_meshlet_bounds(*small.args())[1].numpy().view(np.uint32)
        _assert_same(_run(r, small), (wb[:40], m6, wq), "small call on the large call's scratch")
        _assert_same(_run(r, ladder), _want("count_ladder"), "ladder on the large call's scratch")  # rows of 64 normals, then short ones
        try:
            _tuned(r, 7, 2)
            _assert_same(_run(r, ladder), _want("count_ladder"), "ladder, chunk 7, grid 2, on the large call's scratch")
        finally:
            _tuned(r, 0, 0)
    finally:
        r.close()


# ---- the quantiser's stride loop -------------------------------------------------------------------------------------------------------------------
def test_quantize_vertex_streams_under_a_grid_of_one_block(bounds_renderer):
    """1000 vertices (no multiple of 256) through one block: four stride steps, the last one partial, in all three kernels."""
    import oracle

    g = torch.Generator().manual_seed(5)
    n = 1000
    pos = (torch.rand((n, 3), generator=g) - 0.5) * 300.0
    nrm = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=1)
    uv = torch.rand((n, 2), generator=g) * 4.0 - 1.0
    pos[::97, 1] = float("nan")
    pos[5::101, 2] = 70000.0
    want = oracle.quantize_vertex_streams(pos, nrm, uv)
    try:
        for grid in (1, 3, 0):
            bounds_renderer.debug_set_tuning(L.TUNE_BOUNDS_GRID, grid)
            got = bounds_renderer.quantize_vertex_streams(pos.cuda(), nrm.cuda(), uv.cuda())
            torch.cuda.synchronize()
            for w, g_, what in zip(want, got, ("positions", "normals", "texcoords")):
                assert torch.equal(w, g_.cpu()), f"{what}, grid {grid}"
    finally:
        bounds_renderer.debug_set_tuning(L.TUNE_BOUNDS_GRID, 0)


# ---- once at the real constants --------------------------------------------------------------------------------------------------------------------
def test_real_constants_in_one_call(bounds_renderer):
    """many_small(2^18 + 5), untuned: a second chunk with first = 2^18, the gather kernel's stride (4096 blocks for 65 536 steps of 4)
    and the partial fold's stride (threads fold meshlets 65 536 apart) in one call.  Measured on an MI355X: 0.11 s for the whole test, the checker's run and
    the copies included, so the fallback to many_small(70_001) is not needed."""
    n = (1 << 18) + 5
    _assert_same(_run(bounds_renderer, _many_small(n)), _want(str(n)), f"many_small({n})")
