"""oxc_pick_transform and oxc_apply_highlight on the GPU against tests/highlight_model.py: every word of mask_bits, every byte of the mask
image, every word of the composite and the pick's word equal to the checker's between poisoned guard bands (highlight_frames.run / run_pick),
on the drawn 192 x 192 frame, at the word and tile boundaries, on hand-made frames, in a captured graph, and at every limit."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import highlight_frames as HF
import highlight_model as HM
import refusals as R
from gpu_passes import ALL_FLAGS, DrawnFrame, Guard, lights_tensor, same

pytestmark = pytest.mark.gpu
rep = dataclasses.replace
NAN, INF = float("nan"), float("inf")
FORMAT_IDS = ["rgba8-srgb", "bgra8-srgb", "rgba8-unorm"]


@pytest.fixture(scope="module")
def r(renderer):
    return renderer


@pytest.fixture(scope="module")
def drawn(r):
    """The drawn 192 x 192 frame, lit and tonemapped into the three 8-bit formats."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import TonemapContext

    d = DrawnFrame(r)
    d.passes()
    d.pbr_ctx = d.pbr(ALL_FLAGS, lights_tensor(d.four_lights()))
    r.apply_pbr(d.pbr_ctx)
    d.tone = {fmt: TonemapContext.create(d.pbr_ctx.final_attachment, 0, L.TONEMAP_ACES, output_format=fmt) for fmt in HF.FORMATS}
    for t in d.tone.values():
        r.apply_tonemap(t)
    torch.cuda.synchronize()
    return d


def drawn_frame(d, selected, fmt=0, **settings) -> HF.Frame:
    """The drawn frame's buffers as a highlight Frame (numpy)."""
    u32 = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)  # noqa: E731
    return HF.Frame(u32(d.vis), d.f.depth.cpu().numpy(), u32(d.tone[fmt].dst_attachment), u32(d.cpu.meshlet_instances).reshape(-1, 2), u32(d.cpu.mesh_instances).reshape(-1, 5),
                    d.dctx.meshlet_instance_count, np.asarray(selected, np.uint32), color_format=fmt, **settings)


def seen_transforms(f: HF.Frame) -> np.ndarray:
    """The transforms the frame shows, the most frequent first."""
    t = HM.texel_transform(f.vis, **f.records)
    values, counts = np.unique(t[t != HM.EMPTY], return_counts=True)
    return values[np.argsort(-counts, kind="stable")]


# ---- the drawn frame ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", HF.FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("which", ["one", "several", "all"])
def test_drawn_frame(r, drawn, which, fmt):
    """One, several and all of the mesh instances the frame shows selected, in the three formats and the three modes."""
    seen = seen_transforms(drawn_frame(drawn, []))
    assert len(seen) >= 3
    selected = {"one": seen[:1], "several": seen[::2], "all": seen}[which]
    for mode in HF.MODES:
        f = drawn_frame(drawn, selected, fmt, occluded_mode=mode)
        st = {}
        HF.run(r, f, f"drawn {which} format {fmt} mode {mode}", stats=st)
        assert st["selected"] > 100 and st["plain"] > 1000
        if which != "all":
            assert st["edge_occluded"] > 20, st
    print(which, fmt, {k: v for k, v in st.items() if isinstance(v, int)})


def test_drawn_frame_pick(r, drawn):
    f = drawn_frame(drawn, [])
    ys, xs = np.nonzero(f.vis != HM.EMPTY)
    texels = [(int(xs[i]), int(ys[i])) for i in (np.arange(14) * 2657) % len(xs)] + [(0, 0), (191, 191)]   # a stride that walks the columns too
    got = HF.run_pick(r, f, texels, "drawn")
    assert len(set(got)) >= 3


# ---- word and tile boundaries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 63, 64, 65, 127, 128, 129])
def test_extents(r, W):
    """Widths around one and two mask words by heights around the composite's 16-row tile; mask_bits pre-filled with ones, so the zeroed
    tail of a row's last word is seen.  Both stages in one call, then each alone."""
    for H in (1, 2, 17, 65):
        f = HF.frame((W, H), selected=(11, 13, HF.TERRAIN_TRANSFORM), occluded_mode=1)
        both = HF.run(r, f, f"{W}x{H}")
        mask = HM.mask_of_words(both["mask_bits"], W)
        same(HF.run(r, f, f"{W}x{H} composite alone", stages=HM.COMPOSITE, mask=mask)["dst"], both["dst"], "alone == together")
        same(HF.run(r, f, f"{W}x{H} mask alone", stages=HM.MASK)["mask_bits"], both["mask_bits"], "alone == together")


@pytest.mark.parametrize("radii", [(0, 0), (-7, 1), (1, 1), (5, 8), (8, 5), (63, 2), (64, 3), (65, 64), (255, 255), (2, 255), (255, 2)], ids=str)
def test_radii(r, radii):
    """Radii at and below zero (taken as 1), the engine's, at the word boundary, and at the cap; on 129 x 65 both 255s are larger than the
    image.  Single selected pixels in every corner, on every edge and in the middle, so a window is cut on each side."""
    W, H = 129, 65
    f = HF.frame((W, H), selected=(99,))
    vis = np.where(HM.texel_transform(f.vis, **f.records) == HM.EMPTY, f.vis, np.uint32(0x00000205)).astype(np.uint32)   # transform 12 everywhere but ~0u
    mi = f.mesh_instances.copy()
    mi[5, 3] = 99
    for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (64, 32)]:
        vis[y, x] = 5 << 8
    f = rep(f, vis=vis, mesh_instances=mi, dilate_radius=radii[0], outline_width=radii[1], occluded_mode=0)
    st = {}
    HF.run(r, f, f"radii {radii}", stats=st)
    assert st["selected"] == 9 and st["edge_occluded"] > 0 and st["edge_free"] > 0 and st["edge"].sum() >= 9 * 3


def test_radius_larger_than_a_small_image(r):
    f = HF.frame((17, 9), dilate_radius=200, outline_width=100)
    st = {}
    HF.run(r, f, "radii beyond 17 x 9", stats=st)
    assert st["selected"] > 0 and st["edge"].sum() == (~HF.want_mask(f)).sum()   # every unselected pixel is an edge


# ---- the selection list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 64, 65, 4097])
def test_selection_list_lengths(r, count):
    """The list is read 64 entries a step: none, one, exactly one step, one past it and many.  The hit sits in the last entry; the rest are
    transforms no texel has, ~0u and duplicates."""
    filler = np.array([HM.EMPTY, 777, 777, 1000, HM.EMPTY, 5], np.uint32)
    selected = filler[np.arange(count) % len(filler)]
    if count:
        selected[-1] = 13
    f = HF.frame((65, 17), selected=selected)
    st = {}
    HF.run(r, f, f"{count} entries", stats=st)
    assert (st["selected"] > 0) == (count > 0)
    if count > 1:
        early = selected.copy()
        early[0], early[-1] = 11, 777
        HF.run(r, rep(f, selected=early), f"{count} entries, the hit first")


def test_selection_of_nothing_but_empty_entries_and_duplicates(r):
    f = HF.frame((65, 17), selected=[HM.EMPTY] * 5)
    st = {}
    HF.run(r, f, "only ~0u", stats=st)
    assert st["selected"] == 0 and st["edge"].sum() == 0
    HF.run(r, rep(f, selected=np.array([11, 11, HM.EMPTY, 11, 13, 13], np.uint32)), "duplicates", stats=st)
    assert st["selected"] > 0


@pytest.mark.parametrize("terrain,listed", [(HF.TERRAIN_TRANSFORM, True), (HF.TERRAIN_TRANSFORM, False), (HM.EMPTY, True)])
def test_terrain_transform(r, terrain, listed):
    """The terrain's transform selected, not selected, and ~0u (never selected, though the list holds ~0u)."""
    f = HF.frame((33, 19), selected=[11] + ([terrain] if listed else []), terrain_transform_index=terrain)
    HF.run(r, f, f"terrain {terrain:#x} listed={listed}")
    on_terrain = HF.want_mask(f)[(f.vis >> 8) == HM.TERRAIN_INSTANCE]
    assert on_terrain.size and on_terrain.all() == (listed and terrain != HM.EMPTY) and on_terrain.any() == on_terrain.all()


def test_texels_beyond_the_count_and_an_unset_transform(r):
    """Texels at and far past meshlet_instance_count use the all-zero record (transform 0) and read nothing: the guard bands poison what
    lies past the records.  Mesh instance 4 holds transform ~0u and is never selected."""
    f = HF.frame((33, 19), selected=[0, HM.EMPTY])
    vis = f.vis.copy()
    vis[2, 3:9] = (f.meshlet_instance_count << 8) | 7
    vis[5, 10:20] = 0x7FFFFF00
    vis[8, 4:12] = 4 << 8
    f = rep(f, vis=vis)
    HF.run(r, f, "beyond the count")
    m = HF.want_mask(f)
    assert m[2, 3:9].all() and m[5, 10:20].all() and not m[8, 4:12].any()
    HF.run(r, rep(f, meshlet_instance_count=0), "count 0")
    HF.run_pick(r, f, [(3, 2), (10, 5), (4, 8)], "beyond the count")


# ---- the composite's number classes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3, -1])
def test_depth_classes_under_the_outline(r, mode):
    """0, 0.00001f, the next float above, NaN, +-Inf and a negative depth under edge pixels, in every mode and two values that are none."""
    f = HF.frame((33, 19), occluded_mode=mode)
    limit = np.float32(0.00001)
    specials = np.array([0.0, limit, np.nextafter(limit, np.float32(1)), NAN, INF, -INF, -1.0, 1e-40], np.float32)
    depth = specials[(np.arange(f.depth.size) * 3 + np.arange(f.depth.size) // 8) % len(specials)].reshape(f.depth.shape)
    st = {}
    HF.run(r, rep(f, depth=depth), f"depth classes, mode {mode}", stats=st)
    at = lambda v: st["edge"] & (depth.view(np.uint32) == np.float32(v).view(np.uint32))  # noqa: E731
    assert all(at(v).any() for v in specials)
    assert not (st["occluded"] & (at(0.0) | at(limit) | at(NAN) | at(-INF))).any() and (st["occluded"] | ~(at(specials[2]) | at(INF))).all()


@pytest.mark.parametrize("outline", [(1.0, 0.53, 0.0, 1.0), (0.04, 0.04045, 0.041, 0.5), (NAN, INF, -0.5, 1.0), (0.2, 0.4, 0.6, NAN), (0.2, 0.4, 0.6, INF), (0.7, 0.1, 0.3, 0.0)],
                         ids=str)
@pytest.mark.parametrize("fmt", HF.FORMATS, ids=FORMAT_IDS)
def test_outline_colours(r, fmt, outline):
    """The engine's colour, channels on both sides of 0.04045 and on it, NaN, Inf and a negative channel, a NaN, an infinite and a zero alpha;
    the colour image holds alpha 0, 128 and 255."""
    for mode in HF.MODES:
        f = HF.frame((33, 19), color_format=fmt, outline_color=outline, occluded_mode=mode)
        st = {}
        HF.run(r, f, f"outline {outline} format {fmt} mode {mode}", stats=st)
        alpha = f.color >> 24
        assert all(((alpha == a) & st["edge"]).any() and ((alpha == a) & ~st["edge"]).any() for a in (0, 128, 255))
        assert st["edge_occluded"] and st["edge_free"] and st["translucent"]


def test_every_byte_of_a_channel(r):
    """A 256 x 3 image: every byte value in every channel under alpha 255 (copied), 128 and 0, no selection and the whole image an outline."""
    v = np.arange(256, dtype=np.uint32)
    color = np.stack([(v | (v[::-1] << 8) | (((v * 7 + 3) & 0xFF) << 16) | (a << 24)).astype(np.uint32) for a in (255, 128, 0)])
    f = HF.frame((256, 3))
    for fmt in HF.FORMATS:
        HF.run(r, rep(f, color=color, selected=np.zeros(0, np.uint32), color_format=fmt), f"bytes, format {fmt}, no selection")
        for mode in HF.MODES:
            HF.run(r, rep(f, color=color, color_format=fmt, occluded_mode=mode, dilate_radius=255, outline_width=3), f"bytes, format {fmt}, mode {mode}")


# ---- stages apart -----------------------------------------------------------------------------------------------------------------------------
def test_each_stage_alone_with_the_other_stage_null_and_poisoned(r):
    f = HF.golden_frame()
    g = np.load(HF.GOLDEN)
    mask = HF.want_mask(f)
    for poisoned in (False, True):
        got = HF.run(r, f, f"mask alone, poisoned={poisoned}", stages=HM.MASK, poisoned_rest=poisoned)
        same(got["mask_bits"], g["mask_bits"], "the golden mask words")
        same(got["mask_attachment"], g["mask_attachment"], "the golden mask image")
        for fmt in HF.FORMATS:
            for mode in HF.MODES:
                got = HF.run(r, rep(f, color_format=fmt, occluded_mode=mode), f"composite alone, poisoned={poisoned}", stages=HM.COMPOSITE, poisoned_rest=poisoned, mask=mask)
                same(got["dst"], g[f"dst_format{fmt}_mode{mode}"], "the golden composite")
    HF.run(r, f, "no mask image", stages=HM.MASK, mask_image=False)


def test_composite_ignores_bits_past_the_width(r):
    """A composite that runs alone over mask words whose tail bits a caller left set."""
    f = HF.frame((65, 17))
    mask = HF.want_mask(f)
    gs = HF.guards(f, HM.COMPOSITE, mask=mask)
    words = gs["mask_bits"].tensor.view(-1).view(torch.int64).view(17, 2)
    words[:, 1] |= -2   # every bit past pixel 64
    r.prepared_frame = None
    r.apply_highlight(HF.context(f, gs, HM.COMPOSITE))
    torch.cuda.synchronize()
    same(HF.got_dst(gs, f), HF.want_composite(f, mask), "tail bits set")


def test_pick_every_texel_class(r):
    f = HF.frame((33, 19))
    vis = f.vis.copy()
    vis[1, 1], vis[1, 2], vis[1, 3], vis[1, 4], vis[1, 5] = HM.EMPTY, HF.TERRAIN_TEXEL | 0xFF, (f.meshlet_instance_count << 8), 4 << 8, (7 << 8) | 63
    f = rep(f, vis=vis)
    got = HF.run_pick(r, f, [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (0, 0), (32, 18), (32, 0), (0, 18)], "classes")
    assert got[:5] == [HM.EMPTY, HF.TERRAIN_TRANSFORM, 0, HM.EMPTY, 11]
    HF.run_pick(r, rep(f, terrain_transform_index=HM.EMPTY), [(2, 1)], "terrain ~0u")


# ---- captured graph -------------------------------------------------------------------------------------------------------------------------
def test_draw_pick_mask_tonemap_composite_in_one_graph(r, drawn):
    """draw -> pick -> mask -> decode .. lit -> tonemap -> composite captured into one graph, replayed three times; between the replays the
    selection and the picking texel's record are rewritten and the outputs poisoned."""
    from oxylus_amd.renderer import HighlightContext, ImageAttachment, PickingContext

    d = drawn
    W, H = d.W, d.H
    base = drawn_frame(d, [])
    seen = seen_transforms(base)
    selection = torch.zeros(3, dtype=torch.int32, device="cuda")
    ys, xs = np.nonzero(base.vis != HM.EMPTY)
    texel = (int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))
    tone = d.tone[0]
    n = HF.words_per_row(W)
    bits = Guard("mask_bits", (H, 2 * n), torch.int32, 2 * n, HF.POISON32, 8, fill=HF.FILL_ONES)
    dst = Guard("dst", (H, W), torch.int32, W, HF.POISON32, 4, fill=HF.FILL_DST)
    picked = Guard("transform_id", (1,), torch.int32, 1, HF.POISON32, 4, fill=0x0BADBAD0)
    pctx = PickingContext.over(d.vis, texel, HF.TERRAIN_TRANSFORM, d.dctx.meshlet_instance_count, picked.tensor)
    hctx = HighlightContext(HM.MASK, W, H, bits.tensor, visbuffer_attachment=d.vis, transform_indices=selection, terrain_transform_index=HF.TERRAIN_TRANSFORM,
                            meshlet_instance_count=d.dctx.meshlet_instance_count, depth_attachment=ImageAttachment.depth(d.f.depth), color_attachment=tone.dst_attachment,
                            dst_attachment=dst.tensor, occluded_mode=1)

    def chain(stream=None):
        d.passes(stream)
        r.pick_transform(pctx, stream=stream)
        r.apply_highlight(hctx, stream=stream)
        r.apply_pbr(d.pbr_ctx, stream=stream)
        r.apply_tonemap(tone, stream=stream)
        r.apply_highlight(rep(hctx, stages=HM.COMPOSITE), stream=stream)

    chain()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain(stream)
    for replay in range(3):
        chosen = np.array([seen[replay % len(seen)], seen[(replay + 1) % len(seen)], HM.EMPTY], np.uint32)
        selection.copy_(torch.from_numpy(chosen.view(np.int32)))
        for g in (bits, dst, picked):
            g.refill()
        graph.replay()
        torch.cuda.synchronize()
        f = rep(drawn_frame(d, chosen), occluded_mode=1)
        mask = HF.want_mask(f)
        want = HF.want_composite(f, mask)
        for g in (bits, picked):
            g.check(f"replay {replay}")
        dst.check(f"replay {replay}", want)
        same(bits.bits()[1].view(np.uint64).reshape(H, n), HM.mask_words(mask), f"replay {replay}: mask_bits")
        same(dst.bits()[1].reshape(H, W), want, f"replay {replay}: dst_attachment")
        assert int(picked.bits()[1][0]) == HF.want_pick(f, *texel)
        assert 0 < mask.sum() < mask.size


# ---- limits ---------------------------------------------------------------------------------------------------------------------------------
def _unwritten(gs, f, outputs):
    def check(label):
        for g in gs.values():
            g.check(label)
        for name in outputs:
            window = gs[name].bits()[1]
            assert (window == gs[name].fill).all(), f"{label}: {name} written after a refusal"
    return check


@pytest.mark.parametrize("stages", [HM.MASK, HM.COMPOSITE, HM.ALL], ids=["mask", "composite", "both"])
def test_highlight_limits_alone_and_in_pairs(r, stages):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    f = HF.golden_frame()
    W, H = f.extent
    mask = HF.want_mask(f)
    gs = HF.guards(f, stages, mask=None if stages & HM.MASK else mask)
    frame = HF.prepared_frame(gs, f)
    base = HF.context(f, gs, stages)
    t = lambda name: gs[name].tensor  # noqa: E731
    has_mask, has_composite = bool(stages & HM.MASK), bool(stages & HM.COMPOSITE)
    cases = [("struct_size", {"raw:struct_size": C.sizeof(L.HighlightContext) - 8}, "bad context / struct_size"),
             ("no stage", dict(stages=0), "stages must be"), ("an unknown stage", dict(stages=stages | 4), "stages must be"),
             ("width 0", dict(width=0), "the extent must not be zero"), ("height 0", dict(height=0), "the extent must not be zero"),
             ("65537 wide", dict(width=65537), "extent beyond 65536"), ("65537 tall", dict(height=65537), "extent beyond 65536")]
    if has_composite:
        depth = t("depth")
        one_level = "depth_attachment must be one R32F level at offset 0"
        cases += [("format 3", dict(color_format=3), "color_format must be 0, 1 or 2"),
                  ("radius 256", dict(dilate_radius=256), "dilate_radius and outline_width must be at most 255"),
                  ("width 256", dict(outline_width=256), "dilate_radius and outline_width must be at most 255"),
                  ("depth narrower", dict(depth_attachment=ImageAttachment(depth.view(-1), W - 1, H, 1, [0])), "depth_attachment extent differs"),
                  ("depth taller", dict(depth_attachment=ImageAttachment(depth.view(-1), W, H + 1, 1, [0])), "depth_attachment extent differs"),
                  ("two levels", dict(depth_attachment=ImageAttachment(depth.view(-1), W, H, 2, [0, 0])), one_level),
                  ("level offset", dict(depth_attachment=ImageAttachment(depth.view(-1), W, H, 1, [4])), one_level)]
    if has_mask:
        cases.append(("frame null", {"frame": None}, "the frame must not be null"))
        cases += R.buffer_cases("visbuffer_attachment", t("vis"), torch.int16)
        # a null list with selected_count 0 is accepted, so the count is kept beside it
        cases += [("transform_indices null", {"transform_indices": None, "raw:selected_count": len(f.selected)}, "transform_indices must not be null"),
                  ("transform_indices unaligned", {"transform_indices": R.later(t("selected"), torch.int16)}, "transform_indices must be aligned to its texel")]
        cases.append(("transform_indices small", {"raw:selected_count": len(f.selected) + 1}, "transform_indices is smaller than selected_count u32"))
    cases += R.buffer_cases("mask_bits", t("mask_bits"), torch.int32)
    if has_mask:
        cases.append(("mask_attachment small", dict(mask_attachment=base.mask_attachment[:-1]), "mask_attachment is smaller than its extent"))
    if has_composite:
        cases += [("depth null", dict(depth_attachment=R.null_image(W, H)), "depth_attachment must not be null"),
                  ("depth unaligned", dict(depth_attachment=ImageAttachment(R.later(t("depth"), torch.int16), W, H, 1, [0])), "depth_attachment must be aligned to its texel")]
        cases += R.buffer_cases("color_attachment", t("color"), torch.int16)
        cases += R.buffer_cases("dst_attachment", t("dst"), torch.int16)
    if has_mask:
        cases += R.buffer_cases("frame:meshlet_instances_buffer", t("meshlet_instances"), torch.int16, " is smaller than meshlet_instance_count records", "meshlet_instances_buffer")
        cases += R.buffer_cases("frame:mesh_instances", t("mesh_instances"), torch.int16, None, "mesh_instances_buffer")
        # the visbuffer's window starts at an odd multiple of 4 bytes: one word later it is aligned to 8
        cases += [("mask_bits over the visbuffer", dict(mask_bits=t("vis").view(-1)[1:]), "mask_bits must not overlap visbuffer_attachment")]
    if has_composite:
        words = t("dst").view(-1)
        cases += [("dst over the depth", dict(depth_attachment=ImageAttachment(words.view(torch.float32), W, H, 1, [0])), "dst_attachment must not overlap depth_attachment"),
                  ("dst over the colour", dict(color_attachment=words), "dst_attachment must not overlap color_attachment")]
    outputs = (("mask_bits", "mask_image") if has_mask else ()) + (("dst",) if has_composite else ())
    R.alone_and_in_pairs(r, "oxc_apply_highlight", cases, base, frame, _unwritten(gs, f, outputs))
    # accepted after all
    r.prepared_frame = frame
    r.apply_highlight(base)
    torch.cuda.synchronize()
    if has_mask:
        same(HF.got_mask_words(gs, f), HM.mask_words(mask), "accepted after the refusals")
    if has_composite:
        same(HF.got_dst(gs, f), HF.want_composite(f, mask), "accepted after the refusals")


def test_pick_limits_alone_and_in_pairs(r):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import PickingContext

    f = HF.golden_frame()
    W, H = f.extent
    gs = HF.guards(f, HM.MASK, mask_image=False)
    gs["transform_id"] = Guard("transform_id", (1,), torch.int32, 1, HF.POISON32, 4, fill=0x0BADBAD0)
    frame = HF.prepared_frame(gs, f)
    t = lambda name: gs[name].tensor  # noqa: E731
    base = PickingContext.over(t("vis"), (3, 4), f.terrain_transform_index, f.meshlet_instance_count, t("transform_id"))
    outside = "the texel lies outside the image"
    cases = [("struct_size", {"raw:struct_size": C.sizeof(L.PickContext) + 8}, "bad context / struct_size"),
             ("width 0", dict(width=0), "the extent must not be zero"), ("height 0", dict(height=0), "the extent must not be zero"),
             ("65537 wide", dict(width=65537), "extent beyond 65536"),
             ("x == width", dict(picking_texel=(W, 0)), outside), ("y == height", dict(picking_texel=(0, H)), outside), ("x huge", dict(picking_texel=(0xFFFFFFFF, 0)), outside),
             ("frame null", {"frame": None}, "the frame must not be null")]
    cases += R.buffer_cases("visbuffer_attachment", t("vis"), torch.int16)
    cases += R.buffer_cases("transform_id", t("transform_id"), torch.int16, None)
    cases.append(("transform_id small", dict(transform_id=t("transform_id").view(torch.int16)[:1]), "transform_id is smaller than its extent"))   # two bytes
    cases += R.buffer_cases("frame:meshlet_instances_buffer", t("meshlet_instances"), torch.int16, " is smaller than meshlet_instance_count records", "meshlet_instances_buffer")
    cases += R.buffer_cases("frame:mesh_instances", t("mesh_instances"), torch.int16, None, "mesh_instances_buffer")
    cases.append(("over the visbuffer", dict(transform_id=t("vis").view(-1)[5:6]), "transform_id must not overlap visbuffer_attachment"))
    R.alone_and_in_pairs(r, "oxc_pick_transform", cases, base, frame, _unwritten(gs, f, ("transform_id",)))
    r.prepared_frame = frame
    r.pick_transform(base)
    torch.cuda.synchronize()
    assert int(gs["transform_id"].bits()[1][0]) == HF.want_pick(f, 3, 4)


def test_null_contexts(r):
    from oxylus_amd import lib as L

    assert r._lib.oxc_apply_highlight(r._ctx, None, None, None) == L.OXC_INVALID_ARG and b"struct_size" in r._lib.oxc_last_error(r._ctx)
    assert r._lib.oxc_pick_transform(r._ctx, None, None, None) == L.OXC_INVALID_ARG and b"struct_size" in r._lib.oxc_last_error(r._ctx)
