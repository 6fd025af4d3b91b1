"""What the five VSM and per-pixel entry points say when they refuse an argument block: OXC_INVALID_ARG and the exact oxc_last_error
text, entry point's prefix included, and for a block that breaks two rules which of them is reported.  The other tests check the status
of a bad argument per pass; the text and the order of the checks are pinned here.  Every rejected call returns before any launch.

The surroundings are the smallest valid ones: page_table_size 8, page_size 16, physical_page_table_size 64, one clipmap, a 16 x 16
depth image.  oxc_contact_shadows reads no normal image and oxc_generate_ambient_occlusion writes no R32F image: the first has no
misaligned-normal case, and the second's output of another extent is its ambient_occlusion_attachment of 8 x 16 texels."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = dict(page_size=16, page_table_size=8, physical_page_table_size=64, clipmap_count=1)
W = H = 16
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]


def _zeros(shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def _image(w, h, levels=1):
    """An image header of w x h texels over a small allocation: the calls that get one are refused before anything reads it."""
    from oxylus_amd.renderer import ImageAttachment

    return ImageAttachment(_zeros(W * H * 2, torch.float32), w, h, levels, [0, 4 * W * H][:levels])


def _update():
    from oxylus_amd.renderer import VirtualShadowmapContext

    return VirtualShadowmapContext.create(torch.full((H, W), 0.5, dtype=torch.float32, device="cuda"), IDENTITY, (W, H), _zeros(76, torch.uint8),
                                          with_hpb=False, with_physical=True, virtual_extent=128.0, **SHAPE)


def _draw():
    from oxylus_amd.renderer import VsmDrawContext

    return VsmDrawContext.create(_update())


def _resolve():
    from oxylus_amd.renderer import ShadowResolveContext

    return ShadowResolveContext.create(_update(), _zeros((H, W, 4), torch.int16), (0.0, 1.0, 0.0), 100.0)


def _contact():
    from oxylus_amd.renderer import ContactShadowsContext

    return ContactShadowsContext.create(torch.full((H, W), 0.5, dtype=torch.float32, device="cuda"), IDENTITY, IDENTITY, IDENTITY, 0.1, (0.0, 1.0, 0.0))


def _ambient():
    from oxylus_amd.renderer import AmbientOcclusionContext

    return AmbientOcclusionContext.create(torch.full((H, W), 0.5, dtype=torch.float32, device="cuda"), _zeros((H, W, 4), torch.int16),
                                          _zeros((64, 64), torch.int16), IDENTITY, IDENTITY, 100.0)


# entry point -> (the prefix of its messages, its context, its ABI function)
PASSES = {"update": ("update_virtual_shadowmap", _update, "oxc_update_virtual_shadowmap"),
          "draw": ("draw_physical_pages", _draw, "oxc_draw_physical_pages"),
          "resolve": ("resolve_shadowmap", _resolve, "oxc_resolve_shadowmap"),
          "contact": ("contact_shadows", _contact, "oxc_contact_shadows"),
          "ambient": ("generate_ambient_occlusion", _ambient, "oxc_generate_ambient_occlusion")}
VSM = ("update", "draw", "resolve")
PIXEL = ("resolve", "contact", "ambient")


def refused(renderer, which, **edits):
    """The context of `which` with `edits` applied is refused with OXC_INVALID_ARG; returns oxc_last_error without the entry point's
    prefix.  The draw gets an empty PreparedFrame: its buffers are looked at after every rule tested here."""
    from oxylus_amd import lib as L

    prefix, make, fn = PASSES[which]
    c = dataclasses.replace(make(), **edits).c()
    args = (C.byref(L.PreparedFrame()), C.byref(c)) if which == "draw" else (C.byref(c),)
    st = getattr(renderer._lib, fn)(renderer._ctx, *args, renderer._stream(None))
    text = renderer._lib.oxc_last_error(renderer._ctx).decode()
    assert st == L.OXC_INVALID_ARG, (st, text)
    assert text.startswith(prefix + ": "), text
    return text[len(prefix) + 2:]


SHAPE_RULES = {"clipmap_count_0": (dict(clipmap_count=0), "clipmap_count must be 1..16"),
               "clipmap_count_17": (dict(clipmap_count=17), "clipmap_count must be 1..16"),
               "page_table_size_12": (dict(page_table_size=12), "page_table_size must be a multiple of 8 in [8, 256]"),
               "page_table_size_264": (dict(page_table_size=264), "page_table_size must be a multiple of 8 in [8, 256]"),
               "page_size_24": (dict(page_size=24), "page_size must be a multiple of 16 and divide physical_page_table_size"),
               "page_size_not_a_divisor": (dict(page_size=48), "page_size must be a multiple of 16 and divide physical_page_table_size"),
               "physical_pages_512x512": (dict(physical_page_table_size=8192), "more than 65536 physical pages (16 address bits)")}


@pytest.mark.parametrize("rule", SHAPE_RULES)
@pytest.mark.parametrize("which", VSM)
def test_vsm_shape_rule(renderer, which, rule):
    edits, text = SHAPE_RULES[rule]
    assert refused(renderer, which, **edits) == text


@pytest.mark.parametrize("which", VSM)
def test_vsm_table_and_clipmap_sizes(renderer, which):
    """Two clipmaps asked for, one of the buffers still sized for one."""
    two = dict(clipmap_count=2, virtual_page_table=_zeros((2, 8, 8), torch.int32), vsm_clipmaps_buffer=_zeros(2 * 76, torch.uint8))
    if which != "resolve":
        two["vsm_clipmap_dirty_flags_buffer"] = _zeros(2, torch.int32)
    assert refused(renderer, which, **{**two, "virtual_page_table": _zeros((1, 8, 8), torch.int32)}) == "virtual_page_table smaller than clipmap_count * n * n u32"
    assert refused(renderer, which, **{**two, "vsm_clipmaps_buffer": _zeros(2 * 76 - 1, torch.uint8)}) == "vsm_clipmaps_buffer smaller than clipmap_count records"
    if which != "resolve":
        assert refused(renderer, which, **{**two, "vsm_clipmap_dirty_flags_buffer": _zeros(1, torch.int32)}) == "vsm_clipmap_dirty_flags_buffer smaller than clipmap_count u32"


OUTPUT = {"resolve": ("resolved_shadows_attachment", "resolved_shadows_attachment must be one R32F level of the depth attachment's extent"),
          "contact": ("contact_shadows_attachment", "contact_shadows_attachment must be one R32F level of the depth attachment's extent")}
NORMAL = "normal_attachment must be 8-byte aligned u16x4 texels of the depth attachment's extent"


@pytest.mark.parametrize("which", PIXEL)
def test_pixel_pass_image_rules(renderer, which):
    assert refused(renderer, which, depth_attachment=_image(65537, H)) == "depth extent beyond 65536"
    assert refused(renderer, which, depth_attachment=_image(W, 65537)) == "depth extent beyond 65536"
    assert refused(renderer, which, depth_attachment=_image(W, H, levels=2)) == "depth_attachment must be one R32F level at offset 0"
    if which == "ambient":
        assert (refused(renderer, which, ambient_occlusion_attachment=_zeros((H, 8), torch.int16)) ==
                "noisy_occlusion and ambient_occlusion_attachment must be one aligned u16 per pixel")
    else:
        field, text = OUTPUT[which]
        assert refused(renderer, which, **{field: _image(8, H)}) == text
        assert refused(renderer, which, **{field: _image(W, H, levels=2)}) == text
    if which != "contact":
        misaligned = _zeros(W * H * 4 + 2, torch.int16)[2:]  # 4-byte aligned only
        assert misaligned.data_ptr() % 8 == 4
        assert refused(renderer, which, normal_attachment=misaligned) == NORMAL
        assert refused(renderer, which, normal_attachment=_zeros((H, 8, 4), torch.int16)) == NORMAL


def test_two_broken_rules_report_the_first(renderer):
    """Pairs whose checks sit in different groups of rules (shape, the entry point's own, images, tables): the order of the groups."""
    small_table = dict(virtual_page_table=_zeros(63, torch.int32))
    # update: shape, depth image, tables, dirty flags
    assert refused(renderer, "update", page_size=24, **small_table) == "page_size must be a multiple of 16 and divide physical_page_table_size"
    assert refused(renderer, "update", depth_attachment=_image(W, H, levels=2), **small_table) == "depth_attachment must be one R32F level at offset 0"
    assert (refused(renderer, "update", vsm_clipmap_dirty_flags_buffer=_zeros(1, torch.int16), **small_table) ==
            "virtual_page_table smaller than clipmap_count * n * n u32")
    # draw: shape, V and wide_triangle_index, tables, dirty flags, the draw command, the physical image
    big = dict(page_table_size=256, page_size=128, physical_page_table_size=128)
    assert (refused(renderer, "draw", **big, **small_table) ==
            "V = page_table_size * page_size must be <= 16384 (the guard band's fixed-point range)")
    assert refused(renderer, "draw", wide_triangle_index=3, **small_table) == "wide_triangle_index must be 0, 1 or 2"
    assert refused(renderer, "draw", clipmap_count=17, wide_triangle_index=3) == "clipmap_count must be 1..16"
    assert (refused(renderer, "draw", vsm_clipmap_dirty_flags_buffer=_zeros(1, torch.int16), physical_page_image=_image(32, 32)) ==
            "vsm_clipmap_dirty_flags_buffer smaller than clipmap_count u32")
    # resolve: shape, images, normals, tables, the physical image
    assert refused(renderer, "resolve", physical_page_table_size=8192, depth_attachment=_image(65537, H)) == "more than 65536 physical pages (16 address bits)"
    assert refused(renderer, "resolve", resolved_shadows_attachment=_image(8, H), **small_table) == OUTPUT["resolve"][1]
    assert refused(renderer, "resolve", normal_attachment=_zeros((H, 8, 4), torch.int16), **small_table) == NORMAL
    assert (refused(renderer, "resolve", vsm_clipmaps_buffer=_zeros(75, torch.uint8), physical_page_image=_image(32, 32)) ==
            "vsm_clipmaps_buffer smaller than clipmap_count records")
    assert refused(renderer, "resolve", physical_page_image=_image(32, 32)) == "physical_page_image must be one R32F level of physical_page_table_size^2"
    # contact shadows: images, then its settings
    assert refused(renderer, "contact", depth_attachment=_image(W, H, levels=2), steps=0) == "depth_attachment must be one R32F level at offset 0"
    assert refused(renderer, "contact", contact_shadows_attachment=_image(8, H), steps=65) == OUTPUT["contact"][1]
    # ambient occlusion: the depth image, the prefiltered depth, the buffers, then its settings
    assert refused(renderer, "ambient", depth_attachment=_image(65537, H), prefiltered_depth=_image(W, H, levels=2)) == "depth extent beyond 65536"
    assert (refused(renderer, "ambient", prefiltered_depth=_image(W, H, levels=2), normal_attachment=_zeros((H, 8, 4), torch.int16)) ==
            "prefiltered_depth must have the depth attachment's extent and exactly 5 levels")
    assert refused(renderer, "ambient", normal_attachment=_zeros((H, 8, 4), torch.int16), slice_count=0) == NORMAL


def test_counters_are_not_allocated_inside_a_capture():
    """A context that has never counted: the counting call inside a capture is refused with the message below and leaves the stream
    usable -- the plain call after it is captured, the capture ends, the graph replays the plain call's image, and a counting call
    outside the capture allocates the counters and counts."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    try:
        ctx = _contact()
        r.contact_shadows(ctx)
        torch.cuda.synchronize()
        eager = ctx.contact_shadows_attachment.data.cpu().numpy().copy()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 1)
            with pytest.raises(L.OxcError) as e:
                r.contact_shadows(ctx, stream=s)
            r.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 0)
            r.contact_shadows(ctx, stream=s)
        assert e.value.status == L.OXC_INVALID_ARG
        assert str(e.value).endswith(": contact_shadows: the counters are allocated by the first counting call; make one outside the capture")
        with pytest.raises(L.OxcError) as e:
            r.debug_contact_shadows_stats()
        assert str(e.value).endswith(": debug_contact_shadows_stats: no counting oxc_contact_shadows call on this context yet")
        ctx.contact_shadows_attachment.data.fill_(-5.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ctx.contact_shadows_attachment.data.cpu().numpy().view(np.uint32), eager.view(np.uint32))
        r.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 1)
        ctx.contact_shadows_attachment.data.fill_(-5.0)
        r.contact_shadows(ctx)
        counts = r.debug_contact_shadows_stats()
        torch.cuda.synchronize()
        assert counts["non_sky_pixels"] == W * H
        assert np.array_equal(ctx.contact_shadows_attachment.data.cpu().numpy().view(np.uint32), eager.view(np.uint32))
    finally:
        r.close()
