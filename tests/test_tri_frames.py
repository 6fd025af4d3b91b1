"""The frames of tri_frames are what they claim (CPU only): every claim is held against the oracle, the Python copy of expand_slots_wide's
bookkeeping and the model of tris_fused_body's item sequence.  Nothing here runs a kernel; a frame that does not reach the seam it names
fails here."""
import random

import numpy as np
import pytest
import torch

import tri_frames as TF

FORMS = [0, 1, 2]
FORM_IDS = ["packed", "wide9", "pairs"]


def _assert_oracle_is_the_intent(oracle, fr, form):
    """Every slot visible, in order; the oracle's index list is the one the pass flags spell out; the fast-math build agrees (decisive frames)."""
    w = TF.want_cached(fr, form)
    if fr.early:
        assert (w["early"], w["late"]) == (fr.early, fr.V) and fr.early % 2 == 1
        assert np.array_equal(w["early_visible"], np.arange(fr.early)) and np.array_equal(w["late_visible"], np.arange(fr.early, fr.n))
        assert np.array_equal(w["early_indices"], fr.meant(form, 0, fr.early)) and np.array_equal(w["late_indices"], fr.meant(form))
    else:
        assert np.array_equal(w["visible"], np.arange(fr.n))
        assert np.array_equal(w["indices"], fr.meant(form))
        with oracle.variant("fast"):
            assert np.array_equal(TF.want(fr, form)["indices"], w["indices"])


def test_the_late_frames_pyramid_is_what_an_all_far_depth_image_gives(oracle_lib):
    from util import oracle_hiz

    data, levels, offs = oracle_hiz(torch.zeros((128, 128)), 64, 64)
    att = TF.zero_pyramid()
    assert (levels, list(offs)) == (att.levels, list(att.level_offset)) and torch.equal(data, att.data)


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
def test_family_a_puts_the_visible_count_on_every_chunk_and_span_seam(oracle_lib, late):
    seams = {k * s + d for s in (TF.CHUNK, TF.FUSED_SPAN, TF.SPAN) for k in (1, 2) for d in (-1, 0, 1)}
    assert {63, 64, 65, 127, 128, 129, 255, 256, 257}.issubset(seams & set(TF.A_COUNTS)) and {1, 15, 16, 17, 191, 192, 193, 513}.issubset(TF.A_COUNTS)
    for V in TF.A_COUNTS:
        fr = TF.a_frame(V, late)
        assert fr.V == V and fr.early == (TF.EARLY if late else 0)
        fr.check_intent()
        (i1, s1), (i0, s0) = fr.slot(fr.n - 1), (fr.slot(fr.n - 2) if fr.n > 1 else (None, None))
        for form in FORMS:
            assert s1.count(form) > 0
            assert s0 is None or s0.mask(form) != s1.mask(form)  # a clamped slot that leaked the last slot's mask would change the list
            assert all(1 <= fr.slot(i)[1].T <= 3 for i in range(fr.n))
            _assert_oracle_is_the_intent(oracle_lib, fr, form)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_family_b_puts_every_shape_into_slot_0_slot_15_and_the_last_slot(oracle_lib, form):
    shapes = TF.b_shapes(form)
    combos = {(s.vcount, s.T) for s in shapes}
    assert combos == {(v, t) for v in TF.B_VCOUNTS for t in TF.b_tcounts(form)}
    assert all({s.boff for s in shapes if (s.vcount, s.T) == c} == {0, 1, 2, 3} for c in combos)
    assert any(s.dangling for s in shapes) and all(s.T == 0 for s in shapes if s.dangling)
    assert all(not any(s.passes) for s in shapes if s.vcount == 1)
    first, last, end = set(), set(), set()
    for r in TF.b_rotations(form):
        fr = TF.b_frame(form, r)
        assert fr.n % TF.CHUNK != 0  # the list ends inside a chunk
        for i in range(fr.n):
            s = fr.slot(i)[1]
            if (i % TF.CHUNK) // 4 == 0:
                first.add(s.key)
            if (i % TF.CHUNK) // 4 == 15:
                last.add(s.key)
            if s.T and s.vcount >= 3:  # the lane-clamp edge: the last triangle ends on the last vertex
                assert max(s.corners()[-1]) == s.vcount - 1
            if s.dangling:  # between populated meshlets
                assert fr.slot((i - 1) % fr.n)[1].T or fr.slot((i + 1) % fr.n)[1].T
        for cut in TF.B_CUTS:  # the last visible slot is the one every clamped slot does again: each shape, at its own boff & 3, ends a list
            for late in (False, True):
                fc = TF.b_frame(form, r, late, cut)
                assert fc.V == len(shapes) - cut and fc.V % TF.CHUNK != 0 and fc.slot(fc.n - 1)[1] is shapes[(r - 1 - cut) % len(shapes)]
            end.add(fc.slot(fc.n - 1)[1].key)
            if cut and r % 32 == 0:
                _assert_oracle_is_the_intent(oracle_lib, TF.b_frame(form, r, False, cut), form)
        # micro offsets: what the Meshlet records say, with no padding between meshlets
        rows = fr.scene.meshlets.numpy()
        for i in range(fr.n):
            s = fr.slot(i)[1]
            assert rows[i, 1] % 4 == s.boff and rows[i, 2] == s.vcount and rows[i, 3] == s.T
        if r % 16 == 0:
            fr.check_intent()
            _assert_oracle_is_the_intent(oracle_lib, fr, form)
            _assert_oracle_is_the_intent(oracle_lib, TF.b_frame(form, r, True), form)
    keys = {s.key for s in shapes}
    assert first == keys and last == keys and end == keys
    # T = 200 is cut to 64 / 128: triangles meant to pass lie behind the cut, and neither the intent nor the oracle lists them
    cut = [s for s in shapes if s.T == 200 and any(s.passes)]
    assert cut and all(any(s.passes[TF.cap(form):]) and s.count(form) < sum(s.passes) for s in cut)
    fr = TF.b_frame(form, 0)
    ids = (TF.want_cached(fr, form)["indices"].reshape(-1, 2)[:, 0] if form == 2 else TF.want_cached(fr, form)["indices"] >> (9 if form else 8))
    for i in range(fr.n):
        if fr.slot(i)[1].T == 200:
            assert int((ids == i).sum()) == 3 * fr.slot(i)[1].count(form) < 3 * sum(fr.slot(i)[1].passes) or not any(fr.slot(i)[1].passes)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_family_c_reaches_every_seam_of_the_expansion(oracle_lib, form):
    for fused in (False, True):
        reached = set()
        for name in TF.c_names(form):
            fr = TF.c_frame(form, name, fused)
            if name in TF.BASE_NAMES:  # two spans of the emit kernel in either case; nothing is claimed for the fused form (its second item's base is not determined)
                assert fr.n == 2 * TF.SPAN and sum(fr.counts(form)[:TF.SPAN]) == 4 + int(name[-1])
                if fused:
                    _assert_oracle_is_the_intent(oracle_lib, fr, form)
                    continue
            else:
                assert fr.n == 4 * (32 if fused else 64)  # one item of the fused kernel / one span of the emit kernel, four wave shares
            fr.check_intent()
            _assert_oracle_is_the_intent(oracle_lib, fr, form)
            late = TF.c_frame(form, name, fused, True)
            assert late.counts(form) == fr.counts(form)
            _assert_oracle_is_the_intent(oracle_lib, late, form)
            # the copy of the bookkeeping reproduces the oracle's list length wave by wave
            waves = TF.expansion(fr.counts(form), form, fused)
            assert sum(e[2] for w in waves for e in w["events"] if e[0] == "flush") == TF.want_cached(fr, form)["indices"].size
            reached |= TF.expansion_seams(fr.counts(form), form, fused)
        missing = TF.c_required(form, fused) - reached
        assert not missing, (form, fused, sorted(missing))
    masks = [TF.MASK_SHAPES[k].mask(form) for k in ("bit0", "bit63", "ones", "alt")]
    assert masks == [1, 1 << 63, (1 << 64) - 1, int("01" * 32, 2)]
    assert form == 0 or TF.MASK_SHAPES["bit127"].mask(form) == 1 << 127


def test_the_copy_of_the_bookkeeping_on_runs_written_out_by_hand():
    # 341 triangles fill 1023 dwords; the next slot flushes them: head 0, 255 16-byte stores, tail 3
    (w,) = TF.expansion([64] * 5 + [21, 1], 0, False)
    assert [e for e in w["events"] if e[0] == "flush"] == [("flush", 0, 1023, 0, 255, 3, "full"), ("flush", 3, 3, 1, 0, 2, "end")]
    # a second wave starting on dword 3 of a granule: one head dword, one 16-byte store, one tail dword
    w = TF.expansion([1] + [0] * 63 + [2], 0, False)[1]
    assert w["pad0"] == 3 and w["events"][-1] == ("flush", 3, 6, 1, 1, 1, "end")
    assert TF.expansion([170, 1], 2, True)[0]["events"][1][:3] == ("flush", 0, 1020)


def test_family_d_model_hands_every_chunk_out_exactly_once():
    C = TF.LARGEST_CUS
    assert max(TF.d_fused_counts(C) + TF.d_ordered_counts(C)) == 256 * C + 1 == 65537
    rng = random.Random(2025)
    for cus in (C, 8):
        for V in TF.d_fused_counts(cus):
            for grid in (1, 2, 15, 16, 17, 256, cus):
                for pick in (None, lambda ready: ready[-1], rng.choice):
                    static_chunks, Kc, handed = TF.fused_items(V, grid, TF.ticket_count(V), pick)
                    assert sorted(handed) == list(range(-(-V // TF.CHUNK))), (V, grid)
                    assert static_chunks % 2 == 0 or static_chunks == -(-V // TF.CHUNK)
    # the seams the counts are there for, at the grid the tests run (one block per CU)
    nchunks = lambda V: -(-V // TF.CHUNK)  # noqa: E731
    s = {V: TF.fused_items(V, C, TF.ticket_count(V)) for V in TF.d_fused_counts(C)}
    assert s[128 * C][0] == nchunks(128 * C) == 2 * C                                  # nspans == grid: nothing drawn
    assert s[128 * C + 1][0] == 2 * C and nchunks(128 * C + 1) == 2 * C + 1           # nspans == grid + 1: one chunk drawn
    assert nchunks(128 * C + 65) - s[128 * C + 65][0] == 2                            # a whole span drawn as two chunks
    assert nchunks(128 * C + 64 * 17) - s[128 * C + 64 * 17][0] == 17                 # more chunks than ticket counters
    assert nchunks(256 * C - 64) % 2 == 1 and s[256 * C - 64][0] == nchunks(256 * C - 64)  # one round short of a whole round; odd: the last span is one chunk
    assert s[256 * C - 63][0] == nchunks(256 * C - 63) == 4 * C                        # two whole rounds
    assert s[256 * C + 1][0] == 4 * C and nchunks(256 * C + 1) == 4 * C + 1
    assert s[128 * C + 1][1] < TF.TICKET_COUNTERS == s[256 * C + 1][1]                 # Kc limited by ticket_count, and by 16


def test_family_d_frames_are_one_triangle_meshlets_with_a_marked_few(oracle_lib):
    C = TF.LARGEST_CUS
    for V in TF.d_fused_counts(C) + TF.d_ordered_counts(C):
        fr = TF.d_frame(V)
        counts = fr.counts(0)
        assert fr.V == V and set(counts) == {1, 2} and 0 < counts.count(2) < V // 50
        assert all(2 in counts[k:k + TF.SPAN] for k in range(0, V - TF.SPAN, TF.SPAN))
        fr.check_intent()
        for form in (0, 2):
            w = TF.want(fr, form)
            assert np.array_equal(w["visible"], np.arange(V)) and np.array_equal(w["indices"], fr.meant(form))


def test_family_e_decisions_are_the_comparisons_not_the_evaluation_order(oracle_lib):
    oracle = oracle_lib
    cases, _ = TF.e_plain_cases()
    fr = TF.e_plain_frame()
    for form in (0, 2):
        for small in (False, True):
            w = TF.want_cached(fr, form, small)
            assert np.array_equal(w["visible"], np.arange(len(cases)))
            with oracle.variant("fast"):
                assert np.array_equal(TF.want(fr, form, small)["indices"], w["indices"])
    kept = set((TF.want_cached(fr, 0)["indices"] >> 8).tolist())
    assert [i in kept for i in range(len(cases))] == [c[3] for c in cases]
    kept_small = set((TF.want_cached(fr, 0, True)["indices"] >> 8).tolist())
    assert kept_small == {i for i, c in enumerate(cases) if c[3] and c[0].startswith("z-")}  # 0.2-px triangles go, 2048-px ones stay
    flags = oracle.triangle_boundary_flags(fr.scene, fr.scene.cull_camera(), fr.scene.meshlet_instances, torch.arange(fr.n, dtype=torch.int32), 0, fr.n)
    assert [bool(f) for f in flags[:, 0].tolist()] == [c[4] for c in cases]
    # the values the cases are named for
    k = [float(fr.worlds[i][0, 0]) for i in range(5)]
    assert k[0] == float(TF.T0001) and k[1] < k[0] < k[2] and np.nextafter(TF.F(k[1]), TF.F(1)) == TF.T0001 == np.nextafter(TF.F(k[2]), TF.F(0)) and k[3:] == [0.0, -k[0]]
    z = [fr.clip(c[1], fr.records[c[2]].positions()[0])[2] for c in cases[5:]]
    assert z[0] == 0 and not np.signbit(z[0]) and z[1] == 0 and np.signbit(z[1]) and z[2] == -TF.MIN_NORMAL and z[3] == TF.MIN_NORMAL


def test_family_e_small_triangle_boxes_sit_exactly_on_pixel_centres(oracle_lib):
    oracle = oracle_lib
    cases, fr = TF.e_small_cases(), TF.e_small_frame()
    for i, (name, tri, kept, _) in enumerate(cases):
        for v, (X, Y, wq) in enumerate(tri):
            c = fr.clip(0, fr.records[i].positions()[v])
            assert c[3] == wq and c[2] == 0.5
            if wq:  # the screen position is exactly the pixel coordinate the case names, in every evaluation order
                assert ((c[0] / c[3]) * TF.F(0.5) + TF.F(0.5)) * TF.F(64) == X and ((c[1] / c[3]) * TF.F(0.5) + TF.F(0.5)) * TF.F(64) == Y, name
    for form in (0, 2):
        plain, small = TF.want_cached(fr, form, False), TF.want_cached(fr, form, True)
        assert np.array_equal(plain["indices"], fr.meant(form))  # without the small-triangle cull every case is kept
        for sm, w in ((False, plain), (True, small)):
            with oracle.variant("fast"):
                assert np.array_equal(TF.want(fr, form, sm)["indices"], w["indices"])
    kept = set((TF.want_cached(fr, 0, True)["indices"] >> 8).tolist())
    assert [i in kept for i in range(len(cases))] == [c[2] for c in cases]
