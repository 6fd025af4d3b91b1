"""oxc_cull_geometry(use_hpb) -- k_cull_meshlets_hpb_test, test_vsm_page, project_aabb's two "none" exits, prepare's view rows and the host
checks -- off the 64 x 64 x 10 reference shape: the shape table in two layouts and two poison polarities, the page-offset table, the dirty
patterns, list lengths and round sizes around the kernel's seams, the two paths without a page test, one context across view counts, the
producer feeding the consumer, a captured graph and every argument rule.  Every comparison is exact, against the checker
(oracle.cull_meshes / cull_meshlets_hpb / cull_triangles); what makes the cases meaningful is asserted without a GPU in
tests/test_hpb_frames.py ("HPB shapes")."""
import numpy as np
import pytest
import torch

import oracle
from hpb_frames import (DIRTY_PATTERNS, LIST_LENGTHS, OFFSET_SHAPES, POLARITIES, SHAPES, Upload, assert_equals_checker, dirty_case, list_length_case,
                        make_case, none_case, offset_case, page_table, round_case, shape_case, shape_id)
from oxylus_amd import lib as L
from oxylus_amd.renderer import HpbAttachment, ImageAttachment, RendererInstance

pytestmark = pytest.mark.gpu


def _check(renderer, case, triangles=False):
    up = Upload(case, triangles)
    got = up.run(renderer)
    assert_equals_checker(case.want(triangles=triangles), got, case.name)
    up.assert_inputs_untouched()
    return up


@pytest.mark.parametrize("polarity", list(POLARITIES))
@pytest.mark.parametrize("layout", ["packed", "reordered"])
@pytest.mark.parametrize("sid", [shape_id(s) for s in SHAPES])
def test_shape(renderer, oracle_lib, sid, layout, polarity):
    _check(renderer, shape_case(sid, layout, polarity))


@pytest.mark.parametrize("turn", [0, 4, 9])
@pytest.mark.parametrize("sid", [shape_id(s) for s in OFFSET_SHAPES])
def test_page_offsets(renderer, oracle_lib, sid, turn):
    _check(renderer, offset_case(sid, turn))


@pytest.mark.parametrize("polarity", list(POLARITIES))
@pytest.mark.parametrize("pattern", list(DIRTY_PATTERNS))
def test_dirty_patterns(renderer, oracle_lib, pattern, polarity):
    _check(renderer, dirty_case(pattern, polarity))


@pytest.mark.parametrize("n", list(LIST_LENGTHS))
def test_list_lengths(renderer, oracle_lib, n):
    case = list_length_case(n)
    assert case.want()["mli"].shape[0] == n
    _check(renderer, case, triangles=n in (1, 257, 1025))


@pytest.mark.parametrize("which", ["bands", "instances"])
def test_round_sizes(renderer, oracle_lib, which):
    _check(renderer, round_case(which))


@pytest.mark.parametrize("which", ["z_near", "perspective"])
def test_none_paths(renderer, oracle_lib, which):
    _check(renderer, none_case(which))


def test_view_counts_share_one_context(oracle_lib):
    """A fresh context: 1 view, 16 views, 1 view again, each on its own shape -- the scratch and the view rows grow and are reused; then the
    16-view call three times over: the ticket counters are re-armed by every call."""
    r = RendererInstance(0)
    try:
        one = Upload(shape_case(shape_id(SHAPES[0]), "reordered", "00"))
        sixteen = Upload(shape_case(shape_id((32, 128, 16, 8, 16)), "reordered", "ff"))
        for up in (one, sixteen, one):
            assert_equals_checker(up.case.want(), up.run(r), up.case.name)
        runs = [sixteen.run(r) for _ in range(3)]
        for got in runs:
            assert_equals_checker(sixteen.case.want(), got, "repeat")
        one.assert_inputs_untouched()
        sixteen.assert_inputs_untouched()
    finally:
        r.close()


@pytest.mark.parametrize("shape", [(128, 32, 12, 8, 9), (7, 9, 16, 4, 15)], ids=shape_id)
def test_producer_feeds_consumer_off_the_reference_shape(renderer, oracle_lib, shape):
    w, h, layers, levels, count = shape
    case = make_case("producer", shape, "ff", "packed", seed=80)
    pt = page_table(shape, "ff", 81)
    pt[count:] = 0  # (the layers past the views: the producer's bytes, not a guard)
    want_hpb = HpbAttachment.create(w, h, layers, levels, "cpu")
    want_hpb.data.fill_(0xAA)
    oracle.generate_hpb(pt, oracle.make_hpb(want_hpb.data, w, h, layers, levels, want_hpb.level_offset))
    case = case.with_hpb(want_hpb)
    up = Upload(case)
    up.hpb.data.fill_(0x55)
    renderer.generate_hpb(pt.cuda(), up.hpb)
    got = up.run(renderer)
    for k in range(levels):
        assert torch.equal(up.hpb.level(k).cpu(), want_hpb.level(k)), k
    want = case.want()
    assert_equals_checker(want, got, case.name)
    assert 0 < want["visible"].numel() < want["mli"].shape[0]


def test_captured_graph(renderer, oracle_lib):
    """One use_hpb cull captured after a warm-up call of the same shape (a call that had to grow scratch memory under capture returns
    OXC_INVALID_ARG, include/oxcull.h), replayed twice with the dirty words and the pyramid rewritten in place between the replays."""
    a = shape_case(shape_id((32, 128, 16, 8, 16)), "packed", "ff")
    b = make_case("graph-b", a.shape, "00", "packed", seed=90, dirty="alternating", scene=a.scene)
    up = Upload(a)
    s = torch.cuda.Stream()
    renderer.prepared_frame = up.frame
    ctx = up.context()
    with torch.cuda.stream(s):
        renderer.cull_geometry(ctx, stream=s)
    torch.cuda.synchronize()
    assert_equals_checker(a.want(), up.read(renderer, ctx), "warm-up")
    g = torch.cuda.CUDAGraph()
    error = None
    with torch.cuda.graph(g, stream=s):
        try:
            renderer.cull_geometry(ctx, stream=s)
        except L.OxcError as e:
            error = e
    if error is not None:  # not capturable in this form: the documented refusal
        assert error.status == L.OXC_INVALID_ARG
        return
    lists = []
    for case in (a, b):
        up.hpb.data.copy_(case.hpb.data)
        up.dirty.copy_(torch.from_numpy(case.dirty.astype(np.int32)))
        up.frame.visible_meshlet_instances_indices_buffer.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = up.read(renderer, ctx)
        assert_equals_checker(case.want(), got, case.name)
        lists.append(got["visible"])
    assert not torch.equal(lists[0], lists[1])


def test_invalid_arguments(renderer, oracle_lib):
    """Each rule of check_call's use_hpb block on its own: OXC_INVALID_ARG with the rule's message and nothing enqueued -- the outputs keep
    their sentinel; a valid call on the same context then equals the checker."""
    case = shape_case(shape_id((5, 3, 4, 3, 4)), "packed", "ff")
    w, h, layers, levels, count = case.shape
    up = Upload(case)
    renderer.prepared_frame = up.frame
    hpb = up.hpb

    def att(**over):
        kw = dict(data=hpb.data, width=w, height=h, layers=layers, levels=levels, level_offset=list(hpb.level_offset))
        kw.update(over)
        return HpbAttachment(**kw)

    hiz = ImageAttachment(torch.zeros(64, dtype=torch.float32, device="cuda"), 4, 4, 1, [0])
    end_at_4g = list(hpb.level_offset)
    end_at_4g[1] = 2**32 - layers * (w >> 1) * (h >> 1)
    rules = [
        ("exclusive", dict(use_hiz=True, hiz_attachment=hiz)),
        ("vsm_clipmap_count must be 1..16", dict(vsm_clipmap_count=0)),
        ("vsm_clipmap_count must be 1..16", dict(vsm_clipmap_count=17)),
        ("use_hpb needs vsm_clipmaps_buffer", dict(vsm_clipmaps_buffer=up.clip[:-1])),
        ("use_hpb needs vsm_clipmaps_buffer", dict(vsm_clipmap_dirty_flags_buffer=up.dirty.view(torch.uint8)[:-1])),
        ("without a valid hpb_attachment", dict(hpb_attachment=att(layers=count - 1))),
        ("without a valid hpb_attachment", dict(hpb_attachment=att(width=0))),
        ("without a valid hpb_attachment", dict(hpb_attachment=att(levels=0))),
        ("without a valid hpb_attachment", dict(hpb_attachment=att(levels=14, level_offset=[0] * 13))),
        ("larger than 4 GiB", dict(hpb_attachment=att(level_offset=end_at_4g))),
    ]
    sentinel = 0x5A5A5A5A
    for message, over in rules:
        up.frame.visible_meshlet_instances_indices_buffer.fill_(sentinel)
        up.frame.meshlet_instances_buffer.fill_(sentinel)
        torch.cuda.synchronize()
        with pytest.raises(L.OxcError) as e:
            renderer.cull_geometry(up.context(**over))
        assert e.value.status == L.OXC_INVALID_ARG and message in str(e.value), (message, str(e.value))
        torch.cuda.synchronize()
        assert bool((up.frame.visible_meshlet_instances_indices_buffer == sentinel).all()) and bool((up.frame.meshlet_instances_buffer == sentinel).all()), message
    assert_equals_checker(case.want(), up.run(renderer), "the valid call after the refused ones")
    up.assert_inputs_untouched()
