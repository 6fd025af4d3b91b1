"""GPU: the triangle stage on the frames of tri_frames -- the visible count on every chunk and span seam (A), every meshlet shape in pipeline
slot 0, slot 15 and the last slot (B), expansion runs on the kEmitRun flush, every start inside a 16-byte granule and zero-count slots (C), the
fused kernel's static spans and drawn chunks and the grid-stride loops of the ordered pair (D), and the rule's comparisons at exact thresholds
(E).  Ordered calls are compared byte for byte with the oracle, unordered calls as sorted sets with every triangle's indices adjacent; both
output lists are pre-filled with a sentinel that must survive behind what the call wrote.  For the visible list that check is not general: a
plain call's visible buffer is exactly V entries long, so only the early list of a two-pass (late) frame of A to C has room behind it; the early
configurations and families D and E check the index list alone.  test_tri_frames proves on the CPU that the frames
reach the seams they name; DESIGN 35 has the table."""
import itertools

import numpy as np
import pytest
import torch

import tri_frames as TF
from oxylus_amd import lib as L
from oxylus_amd.renderer import CullGeometryContext, PreparedFrame
from util import assert_triangles_adjacent, gpu_frame, pairs_as_u64

pytestmark = pytest.mark.gpu

# every instantiation of the three bodies: ordered / fused x index form x small_triangle_cull x load policy (1 = nt, 2 = plain) x early / late
CONFIGS = list(itertools.product((False, True), (0, 1, 2), (False, True), (1, 2), (False, True)))
CONFIG_IDS = [f"{'fused' if u else 'ordered'}-form{f}-{'small' if s else 'plain'}-loads{p}-{'late' if l else 'early'}" for u, f, s, p, l in CONFIGS]


def _key(a, form):
    return pairs_as_u64(a) if form == 2 else a.view(np.uint32)


def _adjacent(a, form):
    if form == 2:
        u = a.view(np.uint32).reshape(-1, 3, 2)
        assert np.all(u[:, :, 0] == u[:, :1, 0]) and np.all(u[:, 1, 1] == u[:, 0, 1] + 1) and np.all(u[:, 2, 1] == u[:, 0, 1] + 2) and np.all(u[:, 0, 1] % 3 == 0)
    elif a.size:
        assert_triangles_adjacent(a, 9 if form else 8)


def _in_order(fr, form, small, visible):
    """The oracle's index list for the slots in the order `visible` names them."""
    import oracle

    v = torch.from_numpy(np.ascontiguousarray(visible)).to(torch.int32)
    return oracle.cull_triangles(fr.scene, fr.scene.cull_camera(), fr.scene.meshlet_instances, v, 0, v.numel(), wide=form, small_triangle_cull=small).numpy()


def run(r, fr, form, small, fused):
    """One call (early + late where the frame has early slots) on frame `fr`, compared with the oracle; returns the lists."""
    want = TF.want_cached(fr, form, bool(small))
    late, nw = fr.early > 0, TF.words(form)
    tags = ("early_", "late_") if late else ("",)

    def sentinel_behind(tag):
        f = r.prepared_frame
        torch.cuda.synchronize()
        idx = f.reordered_indices_buffer
        assert idx.data_ptr() % 16 == 0  # (what the copy of the bookkeeping takes for granted)
        assert bool((idx[want[tag + "indices"].size:] == TF.SENTINEL).all()), f"{fr.name}: the index list was written behind draw_index_count"
        if tag == "early_":
            assert bool((f.visible_meshlet_instances_indices_buffer[fr.early:] == TF.SENTINEL).all()), f"{fr.name}: the visible list was written behind its end"

    def before_pass(i, ctx):
        f = r.prepared_frame
        if i == 0:
            f.visible_meshlet_instances_indices_buffer.fill_(TF.SENTINEL)
        else:
            sentinel_behind("early_")
        f.reordered_indices_buffer.fill_(TF.SENTINEL)

    got = gpu_frame(r, fr.scene.to("cuda"), cull_flags=L.CULL_TEST_ALL if late else 0, use_hiz=late, hiz=TF.zero_pyramid("cuda") if late else None,
                    mask=fr.mask if late else None, two_pass=late, before_pass=before_pass, unordered_output=int(fused), wide_triangle_index=form,
                    small_triangle_cull=bool(small), max_tris=TF.cap(form))
    sentinel_behind(tags[-1])
    for tag in tags:
        vis, idx, wv, wi = got[tag + "visible"], got[tag + "indices"], want[tag + "visible"], want[tag + "indices"]
        assert idx.size == wi.size and idx.size % (3 * nw) == 0, (fr.name, tag, idx.size, wi.size)
        if not fused:
            assert np.array_equal(vis, wv) and np.array_equal(idx, wi), (fr.name, tag)
            continue
        assert np.array_equal(vis if late else np.sort(vis), wv), (fr.name, tag)  # (the HiZ meshlet stage keeps its ordered emit)
        assert np.array_equal(np.sort(_key(idx, form)), np.sort(_key(wi, form))), (fr.name, tag)
        _adjacent(idx, form)
        if vis.size <= TF.FUSED_SPAN:  # a single item: the order is the visible list's
            assert np.array_equal(idx, _in_order(fr, form, small, vis)), (fr.name, tag)
    if late:
        assert (got["early"], got["late"]) == (fr.early, fr.V) and np.array_equal(got["mask"], want["mask"])
    return got


class _Policy:
    """TUNE_TRI_LOADS for the block, and what debug_tri_loads_mode has to say after every call in it."""

    def __init__(self, r, policy, small):
        self.r, self.policy, self.expect = r, policy, 1 if small else policy  # (the small-triangle instantiations keep the streaming loads)

    def __enter__(self):
        self.r.debug_set_tuning(L.TUNE_TRI_LOADS, self.policy)
        return self

    def check(self):
        assert self.r.debug_tri_loads_mode() == self.expect

    def __exit__(self, *exc):
        self.r.debug_set_tuning(L.TUNE_TRI_LOADS, 0)


def _profiled(r, fr, form, small, fused, late):
    """One call under the profile: the launches of the form asked for, and no others of the triangle stage."""
    r.profile_begin()
    run(r, fr, form, small, fused)
    ran = r.profile_end()["kernels"]
    tests = ["cull_triangles_test"] + (["cull_triangles_test_late"] if late else [])  # (a late frame is an early and a late call)
    assert all(ran[k]["launches"] == 1 for k in tests), ran
    emit = sorted(k for k in ran if k.startswith("cull_triangles_emit"))
    if fused:
        assert not emit, sorted(ran)
    else:
        assert emit == [k.replace("test", "emit") for k in tests] and all(ran[k]["launches"] == 1 for k in emit), sorted(ran)


@pytest.mark.parametrize("fused,form,small,policy,late", CONFIGS, ids=CONFIG_IDS)
def test_visible_counts_on_the_chunk_and_span_seams(renderer, oracle_lib, fused, form, small, policy, late):
    with _Policy(renderer, policy, small) as p:
        for V in TF.A_COUNTS:
            run(renderer, TF.a_frame(V, late), form, small, fused)
            p.check()
        _profiled(renderer, TF.a_frame(129, late), form, small, fused, late)


@pytest.mark.parametrize("fused,form,small,policy,late", CONFIGS, ids=CONFIG_IDS)
def test_meshlet_shapes_in_the_first_the_last_and_the_clamped_slot(renderer, oracle_lib, fused, form, small, policy, late):
    with _Policy(renderer, policy, small) as p:
        for rot in TF.b_rotations(form):
            for cut in TF.B_CUTS:  # (every shape, at its own boff & 3, ends a list: the slot the clamped slots beyond V do again)
                run(renderer, TF.b_frame(form, rot, late, cut), form, small, fused)
                p.check()
        _profiled(renderer, TF.b_frame(form, 0, late), form, small, fused, late)


@pytest.mark.parametrize("fused,form,small,policy,late", CONFIGS, ids=CONFIG_IDS)
def test_expansion_runs_on_the_flush_the_granule_and_zero_count_slots(renderer, oracle_lib, fused, form, small, policy, late):
    with _Policy(renderer, policy, small) as p:
        for name in TF.c_names(form):
            for shares_of_the_fused_form in (False, True):  # both share sizes through either form: a frame is on its seams in the form it was cut for
                run(renderer, TF.c_frame(form, name, shares_of_the_fused_form, late), form, small, fused)
                p.check()
        _profiled(renderer, TF.c_frame(form, "masks", fused, late), form, small, fused, late)


@pytest.fixture
def one_block_per_cu(renderer):
    renderer.debug_set_tuning(L.TUNE_TRI_BLOCKS_PER_CU, 1)
    try:
        yield renderer
    finally:
        renderer.debug_set_tuning(L.TUNE_TRI_BLOCKS_PER_CU, 8)


def _twice_on_one_context(r, fr, form, fused):
    """Two calls on ONE seeded context: the ticket counters and index_count restart from zero in the call's prepare kernel."""
    want = TF.want_cached(fr, form)
    gpu = fr.scene.to("cuda")
    frame = PreparedFrame.create(gpu, with_triangles=True, max_tris=TF.cap(form), index_words=TF.words(form))
    r.prepared_frame = frame
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=0, cull_camera=gpu.cull_camera(), stages=L.STAGE_ALL, unordered_output=int(fused), wide_triangle_index=form)
    r.seed_meshlet_instances(ctx, gpu.n_meshlet_instances)
    wi = np.sort(_key(want["indices"], form))
    for rep in range(2):
        frame.reordered_indices_buffer.fill_(TF.SENTINEL)
        r.cull_geometry(ctx)
        c = r.read_counters(ctx)
        assert (c.cull_triangles_cmd_x, c.draw_index_count * TF.words(form)) == (fr.V, want["indices"].size), (fr.name, rep)
        idx = frame.reordered_indices_buffer[:want["indices"].size].cpu().numpy()
        assert bool((frame.reordered_indices_buffer[want["indices"].size:] == TF.SENTINEL).all()), (fr.name, rep)
        if fused:
            assert np.array_equal(np.sort(_key(idx, form)), wi), (fr.name, rep)  # a lost or doubled item changes the set
            _adjacent(idx, form)
        else:
            assert np.array_equal(idx, want["indices"]), (fr.name, rep)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("form", [0, 2], ids=["packed", "pairs"])
@pytest.mark.parametrize("which", range(7))
def test_fused_work_distribution_by_static_spans_and_drawn_chunks(one_block_per_cu, oracle_lib, which, form):
    fr = TF.d_frame(TF.d_fused_counts(_cus())[which])
    _twice_on_one_context(one_block_per_cu, fr, form, True)


@pytest.mark.parametrize("form", [0, 2], ids=["packed", "pairs"])
@pytest.mark.parametrize("which", range(2), ids=["test-loop", "emit-loop"])
def test_ordered_grid_stride_loops_reach_their_second_iteration(one_block_per_cu, oracle_lib, which, form):
    fr = TF.d_frame(TF.d_ordered_counts(_cus())[which])
    _twice_on_one_context(one_block_per_cu, fr, form, False)


def test_family_d_launches(one_block_per_cu, oracle_lib):
    C = _cus()
    for fused, V in ((True, TF.d_fused_counts(C)[1]), (False, TF.d_ordered_counts(C)[0])):
        _profiled(one_block_per_cu, TF.d_frame(V), 0, False, fused, False)


@pytest.mark.parametrize("form", [0, 2], ids=["packed", "pairs"])
@pytest.mark.parametrize("small", [False, True], ids=["plain", "small"])
@pytest.mark.parametrize("fused", [False, True], ids=["ordered", "fused"])
def test_rule_thresholds(renderer, oracle_lib, fused, small, form):
    """det == 0.0001f and its neighbours, clip.z == +0, -0, -FLT_MIN, +FLT_MIN; boxes exactly on pixel centres, w == 0 and w < 0: the decisions
    test_tri_frames spells out, which do not depend on the evaluation order."""
    for fr in (TF.e_plain_frame(), TF.e_small_frame()):
        run(renderer, fr, form, small, fused)
    if form == 0:
        _profiled(renderer, TF.e_plain_frame(), form, small, fused, False)
