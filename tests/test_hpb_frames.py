"""The conditions that make the cases of tests/test_gpu_hpb_shapes.py meaningful, proved from the checker alone, without a GPU (DESIGN.md,
"HPB shapes"): each is a plain assertion over hpb_frames.census, which is printed per case (pytest -s)."""
import numpy as np
import pytest
import torch

import oracle
from hpb_frames import (DIRTY_PATTERNS, LAYOUTS, LIST_LENGTHS, OFFSET_SHAPES, ONE_TEXEL, POLARITIES, SHAPES, build_or_mips, census, census_line, dirty_case,
                        full_levels, inside_mask, level_dims, list_length_case, none_case, offset_case, page_offset_table, page_table, pyramid, relaid, round_case,
                        shape_case, shape_id)
from oxylus_amd.renderer import HpbAttachment


def _census(case):
    c = census(case)
    print(census_line(case, c))
    return c


def _tot(c, key):
    return sum(v[key] for v in c["views"])


def test_reordered_layout_is_what_it_says():
    for w, h, layers, levels, _ in SHAPES:
        offs, total = LAYOUTS["reordered"](w, h, layers, levels)
        assert all(o % 2 == 1 for o in offs) and offs == sorted(offs, reverse=True)
        inside = inside_mask(w, h, layers, levels, offs, total)
        edges = np.flatnonzero(np.diff(np.concatenate([[True], inside, [True]]).astype(np.int8)))  # [gap start, gap end, ...]
        assert len(edges) == 2 * (levels + 1) and (edges[1::2] - edges[0::2]).min() >= w + 64, (w, h)


def test_or_mips_are_the_producers_on_any_extent(oracle_lib):
    for shape in SHAPES:
        w, h, layers, levels, _ = shape
        want = HpbAttachment.create(w, h, layers, levels, "cpu")
        oracle.generate_hpb(page_table(shape, "ff", 3), oracle.make_hpb(want.data, w, h, layers, levels, want.level_offset))
        got = HpbAttachment.create(w, h, layers, levels, "cpu")
        got.level(0).copy_(want.level(0))
        build_or_mips(got)
        assert torch.equal(got.data, want.data), shape


def test_polarities_are_what_they_say(oracle_lib):
    for shape in SHAPES:
        w, h, layers, levels, count = shape
        for pol, (gap, density) in POLARITIES.items():
            p = pyramid(shape, pol, 5)
            l0 = p.level(0).numpy()
            if w * h >= 64:
                assert abs((l0[:count] != 0).mean() - density) < 0.08, (shape, pol, (l0[:count] != 0).mean())
            if pol == "00":
                assert set(np.unique(l0[:count])) <= {0, 0x80, 0x02, 0xFF, 0x01} and (w * h < 8 or len(np.unique(l0[:count])) == 5)
            for k, (mw, mh) in enumerate(level_dims(w, h, levels)):
                assert (p.level(k).numpy()[count:] == (0xFF if pol == "ff" else 0)).all()
            r = relaid(p, "reordered", gap)
            gaps = ~inside_mask(w, h, layers, levels, r.level_offset, r.data.numel())
            assert gaps.sum() >= (levels + 1) * (w + 64) and (r.data.numpy()[gaps] == gap).all()


@pytest.mark.parametrize("polarity", list(POLARITIES))
@pytest.mark.parametrize("sid", [shape_id(s) for s in SHAPES])
def test_shape_case_is_not_degenerate(oracle_lib, sid, polarity):
    case = shape_case(sid, "reordered", polarity)
    w, h, layers, levels, count = case.shape
    c = _census(case)
    assert c["candidates"] > 0
    if case.shape == ONE_TEXEL:
        # one byte decides every page test of a polarity: clear in "ff" (nothing visible), set in "00" (every candidate visible) -- both outcomes
        # occur, in the two cases
        assert (_tot(c, "passed") == 0, _tot(c, "failed") == 0) == ((True, False) if polarity == "ff" else (False, True))
        assert (c["nobody"] > 0) == (polarity == "ff")
    else:
        assert _tot(c, "passed") > 0 and _tot(c, "failed") > 0
        assert c["nobody"] > 0
    mips = {m for v in c["views"] for m in v["mips"]}
    if levels > 1:
        assert len(mips) >= 2, mips
    if levels < full_levels(w, h):
        assert _tot(c, "clamped") > 0
    # the poison can be seen: a kernel that read gap bytes for pyramid bytes would give another list
    want = case.want()["visible"]
    flood = HpbAttachment(torch.full_like(case.hpb.data, POLARITIES[polarity][0]), w, h, layers, levels, case.hpb.level_offset)
    assert not torch.equal(case.want(hpb=flood)["visible"], want)
    # layers, records and dirty words past the views decide nothing
    other = HpbAttachment(case.hpb.data.clone(), w, h, layers, levels, case.hpb.level_offset)
    for k in range(levels):
        other.level(k)[count:] ^= 0xFF
    assert torch.equal(case.want(hpb=other, flip_guards=True)["visible"], want)
    if count >= 15 and polarity == "ff":
        assert c["first"][14] > 0 and (count < 16 or c["first"][15] > 0), c["first"]
        assert case.other_views and all(c["views"][v]["in_frustum"] > 0 for v in case.other_views)  # views whose same_mask bit is clear


def test_shape_cases_share_one_list_between_layouts(oracle_lib):
    for s in SHAPES:
        for pol in POLARITIES:
            a, b = shape_case(shape_id(s), "packed", pol), shape_case(shape_id(s), "reordered", pol)
            assert torch.equal(a.want()["visible"], b.want()["visible"])


@pytest.mark.parametrize("sid", [shape_id(s) for s in OFFSET_SHAPES])
def test_offset_cases_wrap_and_straddle(oracle_lib, sid):
    wrapped, seam, signs = [0, 0], [0, 0], set()
    for turn in (0, 4, 9):
        case = offset_case(sid, turn)
        c = _census(case)
        assert _tot(c, "passed") > 0 and _tot(c, "failed") > 0
        for a in (0, 1):
            wrapped[a] += sum(v["wrapped"][a] for v in c["views"])
            seam[a] += sum(v["seam"][a] for v in c["views"])
            signs |= {(a, int(np.sign(o))) for o in case.offs[:, a]}
    assert min(wrapped) > 0 and min(seam) > 0, (wrapped, seam)
    assert signs == {(a, s) for a in (0, 1) for s in (-1, 0, 1)}


def test_offset_table_is_the_issues():
    assert page_offset_table(64) == [0, 1, -1, 63, -63, 64, -64, 65, -65, 2**20 + 3, -(2**20 + 3), 2**31 - 1, -2**31]


@pytest.mark.parametrize("pattern", list(DIRTY_PATTERNS))
def test_dirty_cases(oracle_lib, pattern):
    case = dirty_case(pattern)
    c = _census(case)
    dirty = case.dirty != 0
    assert all((c["first"][v] == 0 and c["views"][v]["in_frustum"] == 0) for v in range(16) if not dirty[v])
    assert (c["visible"] > 0) == bool(dirty.any())
    if pattern == "last":
        assert c["first"][15] > 0
    if pattern == "odd-words":
        assert sorted(set(case.dirty.astype(np.int64) & 0xFFFFFFFF)) == [0, 2, 0x100, 0x80000000]
        assert sum(c["views"][v]["in_frustum"] > 0 for v in range(16) if dirty[v]) >= 5


@pytest.mark.parametrize("n", list(LIST_LENGTHS))
def test_list_lengths_are_reached(oracle_lib, n):
    case = list_length_case(n)
    assert case.want()["mli"].shape[0] == n
    if n in (1, 257, 1025):  # the lengths whose triangle stage runs: something reaches it
        c = _census(case)
        assert c["n"] == n and c["visible"] > 0


def test_round_sizes(oracle_lib):
    c = _census(round_case("bands"))
    totals = [t for run in c["runs"] for t in run.values()]
    print("round totals:", totals)
    assert any(t == 256 for t in totals) and any(129 <= t <= 191 for t in totals) and any(193 <= t <= 255 for t in totals) and any(1 <= t <= 63 for t in totals)
    c = _census(round_case("instances"))
    print("instances per run:", [len(run) for run in c["runs"]])
    assert any(len(run) >= 64 for run in c["runs"]) and len(c["runs"][0]) == 256


def test_none_paths(oracle_lib):
    c = _census(none_case("z_near"))
    v = c["views"][1]
    assert v["in_frustum"] > 0 and v["none"] == v["in_frustum"] and v["passed"] + v["failed"] == 0 and c["first"][1] > 0
    assert _tot(c, "passed") > 0 and _tot(c, "failed") > 0 and c["nobody"] > 0
    c = _census(none_case("perspective"))
    v = c["views"][1]
    assert v["none"] > 0 and v["passed"] + v["failed"] > 0 and v["only"] > 0, v
    assert c["nobody"] > 0
