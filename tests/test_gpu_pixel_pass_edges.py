"""The three per-pixel passes on the GPU at the extents where their tiles, clamps and level counts degenerate -- 1 x 1 to 129 x 65, the case
table of tests/test_pixel_pass_edge_cases.py -- with every image a window in the middle of a larger poisoned buffer: oxc_generate_ambient_occlusion
(all five prefiltered levels in a reordered layout with poisoned gaps, depth_differences, noisy_occlusion, the final image and the device
counters), oxc_contact_shadows (two cameras, 1 / 2 / 64 steps, a sun per screen quadrant) and oxc_resolve_shadowmap (the 128 x 128 frame
resampled to each extent) byte for byte against their checkers.  A load outside an input reads NaN and shows as a parity failure; a store
outside an output changes a band, which is compared bit for bit."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

import ambient_occlusion_model as AM
import contact_shadows_model as CM
import vsm_resolve_model as RM
from gpu_passes import (DEVICE, FILL_F32, FILL_U16, FILL_U32, Frame, Guard, _signed, ao_context, ao_got_of, ao_want_of, contact_context, contact_got_of,
                        contact_want_of, same)
from scenes import (AO_FAR, AO_RESOLUTIONS, AO_WIDE, CS_SETTINGS, EXTENT_IDS, EXTENTS, HILBERT_POISON, I16, LIGHT, NAN16, NAN32, OUT16, OUT32, PROJ, Z_LENGTH, ao_inputs,
                    assert_resolve_sweep_is_not_degenerate, cs_depth, cs_runs, hilbert, resample, resolve_counts)

pytestmark = pytest.mark.gpu


class Pyramid:
    """The prefiltered depth in a layout of its own: the five levels in descending address order (level 4 first), a poisoned gap of at
    least W + 64 floats between neighbours and at both ends, every offset a multiple of four bytes."""

    def __init__(self, W, H):
        from oxylus_amd.renderer import ImageAttachment

        self.sizes = [max(1, W >> k) * max(1, H >> k) for k in range(5)]
        gaps = [W + 64 + g for g in (0, 1, 3, 6, 2, 5)]
        self.offs, off = [0] * 5, 0
        for i, k in enumerate((4, 3, 2, 1, 0)):
            off += gaps[i]
            self.offs[k] = off
            off += self.sizes[k]
        self.buf = torch.full((off + gaps[5],), _signed(OUT32, 4), dtype=torch.int32, device=DEVICE)
        self.refill()
        self.attachment = ImageAttachment(self.buf.view(torch.float32), W, H, 5, [4 * o for o in self.offs])

    def refill(self):
        for k in range(5):
            self.buf[self.offs[k]:self.offs[k] + self.sizes[k]].fill_(_signed(FILL_F32, 4))

    def check(self, label, want_levels):
        a = self.buf.cpu().numpy().view(np.uint32)
        inside = np.zeros(a.size, dtype=bool)
        for k in range(5):
            inside[self.offs[k]:self.offs[k] + self.sizes[k]] = True
            assert want_levels[k].size == self.sizes[k] and not (want_levels[k].view(np.uint32) == FILL_F32).any(), (label, k)
        bad = np.flatnonzero(~inside & (a != OUT32))
        if bad.size:
            e = int(bad[0])
            near = min(range(5), key=lambda k: min(abs(e - self.offs[k]), abs(e - (self.offs[k] + self.sizes[k] - 1))))
            raise AssertionError(f"{label}: prefiltered_depth: {bad.size} floats outside the five levels changed, the first at float {e} = level {near}'s "
                                 f"start {e - self.offs[near]:+d} (level {near} holds {self.sizes[near]} floats; value 0x{int(a[e]):X})")


def _where(got, want, limit=6):
    """The first (y, x) at which two images differ."""
    ys, xs = np.nonzero(np.atleast_2d(got) != np.atleast_2d(want))
    return [(int(y), int(x)) for y, x in zip(ys[:limit], xs[:limit])]


# ---- ambient occlusion ----------------------------------------------------------------------------------------------------------------------
class AoCase:
    """One extent's context: depth, normals and the Hilbert table inside NaN / 0x7E00 / 0xFFFF bands, the three output images inside
    poisoned bands, the pyramid in the reordered layout."""

    def __init__(self, W, H, resolution=None):
        depth, normal = ao_inputs(W, H)
        self.label = f"{W} x {H}" + (f" at resolution {resolution}" if resolution else "")
        self.inputs = [Guard("depth_attachment", (H, W), torch.float32, W, NAN32, 4, data=depth),
                       Guard("normal_attachment", (H, W, 4), torch.int16, 4 * W, NAN16, 8, data=normal),
                       Guard("hilbert_noise", (64, 64), torch.int16, 64, HILBERT_POISON, 2, data=hilbert())]
        self.outputs = {"depth_differences": Guard("depth_differences", (H, W), torch.int32, W, OUT32, 4, fill=FILL_U32),
                        "noisy_occlusion": Guard("noisy_occlusion", (H, W), torch.int16, W, OUT16, 2, fill=FILL_U16),
                        "ambient_occlusion": Guard("ambient_occlusion_attachment", (H, W), torch.int16, W, OUT16, 2, fill=FILL_U16)}
        self.pyramid = Pyramid(W, H)
        ctx = ao_context(self.inputs[0].tensor, self.inputs[1].tensor, I16, PROJ, AO_FAR, resolution=resolution)
        ctx.hilbert_noise = self.inputs[2].tensor
        ctx.prefiltered_depth = self.pyramid.attachment
        ctx.depth_differences, ctx.noisy_occlusion = self.outputs["depth_differences"].tensor, self.outputs["noisy_occlusion"].tensor
        ctx.ambient_occlusion_attachment = self.outputs["ambient_occlusion"].tensor
        self.ctx = ctx

    def refill(self):
        self.pyramid.refill()
        for g in self.outputs.values():
            g.refill()

    def compare(self, what, want):
        """All five levels, depth_differences, noisy_occlusion and the final image == `want`; every band and gap untouched."""
        label = f"{self.label}, {what}"
        got = ao_got_of(self.ctx)
        try:
            same(got, want)
        except AssertionError as e:
            first = {f"level {k}": _where(got["levels"][k].view(np.uint32), want["levels"][k].view(np.uint32)) for k in range(5)}
            first.update({name: _where(got[name], want[name]) for name in self.outputs})
            raise AssertionError(f"{label}: {e}; first differing (y, x): { {k: v for k, v in first.items() if v} }") from None
        self.pyramid.check(label, want["levels"])
        for name, g in self.outputs.items():
            g.check(label, want[name])
        for g in self.inputs:
            g.check(label)
        return got

    def run(self, renderer, what, **settings):
        """One setting: the counting instantiation (device counters == checker's), then the plain one (the same bytes)."""
        from oxylus_amd import lib as L

        for k, v in settings.items():
            setattr(self.ctx, k, v)
        st = {}
        want = ao_want_of(self.ctx, st)
        self.refill()
        renderer.debug_set_tuning(L.TUNE_AMBIENT_OCCLUSION_STATS, 1)
        try:
            renderer.generate_ambient_occlusion(self.ctx)
            self.compare(f"{what}, counting", want)
            dev = renderer.debug_ambient_occlusion_stats()
        finally:
            renderer.debug_set_tuning(L.TUNE_AMBIENT_OCCLUSION_STATS, 0)
        counts = AM.counters(st)
        print(self.label, what, "checker", counts)
        print(self.label, what, "device ", dev)
        assert dev == counts, f"{self.label}, {what}: device counters {dev} != checker's {counts}"
        self.refill()
        renderer.generate_ambient_occlusion(self.ctx)
        self.compare(f"{what}, plain", want)
        return counts


@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
def test_ambient_occlusion_extent(renderer, extent):
    """slice_count 3, samples_per_slice_side 8, effect_radius 400 (samples at all five levels at every extent, by
    tests/test_pixel_pass_edge_cases.py), then the engine's struct defaults on the same image."""
    case = AoCase(*extent)
    defaults = {k: getattr(case.ctx, k) for k in AO_WIDE}
    assert defaults == dict(slice_count=3, samples_per_slice_side=3, effect_radius=0.5)
    c = case.run(renderer, "radius 400", **AO_WIDE)
    assert all(c[f"mip{k}"] > 0 for k in range(5)) and c["fractional"] > 0 and c["non_sky_pixels"] >= 1, c
    case.run(renderer, "struct defaults", **defaults)


@pytest.mark.parametrize("extent,resolution", AO_RESOLUTIONS, ids=[f"{r[0]}x{r[1]}" for _, r in AO_RESOLUTIONS])
def test_ambient_occlusion_resolution_differs_from_the_extent(renderer, extent, resolution):
    case = AoCase(*extent, resolution=resolution)
    assert case.ctx.resolution == resolution
    case.run(renderer, "radius 400", **AO_WIDE)


# ---- contact shadows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
def test_contact_shadows_extent(renderer, extent):
    """The identity and the rotated camera, steps 1 / 2 / 64, four suns: image == checker, device counters == checker's, then the plain
    instantiation; depth inside NaN bands, the image inside poisoned bands."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    W, H = extent
    depth = Guard("depth_attachment", (H, W), torch.float32, W, NAN32, 4, data=cs_depth(W, H))
    out = Guard("contact_shadows_attachment", (H, W), torch.float32, W, OUT32, 4, fill=FILL_F32)
    for name, camera, steps, sun in cs_runs():
        label = f"{W} x {H}, {name} camera, steps {steps}, sun {sun}"
        ctx = contact_context(depth.tensor, camera, sun=sun, steps=steps, **CS_SETTINGS)
        ctx.contact_shadows_attachment = ImageAttachment.depth(out.tensor)
        st = {}
        want = contact_want_of(ctx, st)

        def compare(what):
            got = contact_got_of(ctx)
            bad = _where(got.view(np.uint32), want.view(np.uint32))
            assert not bad, f"{label}, {what}: contact_shadows_attachment differs from the checker, first at (y, x) {bad}"
            out.check(f"{label}, {what}", want)
            depth.check(f"{label}, {what}")

        out.refill()
        renderer.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 1)
        try:
            renderer.contact_shadows(ctx)
            compare("counting")
            dev = renderer.debug_contact_shadows_stats()
        finally:
            renderer.debug_set_tuning(L.TUNE_CONTACT_SHADOWS_STATS, 0)
        assert dev == CM.counters(st), f"{label}: device counters {dev} != checker's {CM.counters(st)}"
        out.refill()
        renderer.contact_shadows(ctx)
        compare("plain")


# ---- shadow resolve -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resolve_frame(renderer):
    """Frame(renderer, 128, 128, seed=67) with a third of its pages evicted before the resolve (the taps near a clipmap boundary are then
    served by the neighbouring clipmaps), its shadow path run once, and the CPU copies the checker needs."""
    f = Frame(renderer, 128, 128, seed=67, evict=True)
    f.shadow_path()
    f.check()
    phys = f.shape["physical_page_table_size"]
    cpu = dict(depth=f.depth.cpu().numpy(), normal=f.normal.cpu().numpy(), table=f.vctx.virtual_page_table.cpu().numpy(), clipmaps=f.clip.numpy(),
               physical=f.vctx.physical_page_image.data.view(phys, phys).cpu().numpy())
    return f, cpu


def _resolve_want(f, cpu, depth, normal, W, H, stats):
    return RM.resolve(depth, normal, cpu["table"], cpu["clipmaps"], cpu["physical"], f.inv, (W, H), LIGHT, Z_LENGTH, first_clipmap_width=f.fcw,
                      bias=f.vctx.clipmap_selection_bias, virtual_extent=f.vctx.virtual_extent, stats=stats, **f.shape)


@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
def test_shadow_resolve_extent(renderer, resolve_frame, extent):
    """The frame's depth and normals resampled by nearest neighbour to W x H, resolution = (W, H); page table, clipmaps and physical image
    are the frame's own.  Every pixel == checker, device counters == checker's, then the plain instantiation."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    f, cpu = resolve_frame
    W, H = extent
    label = f"{W} x {H}"
    d, n = resample(cpu["depth"], W, H), resample(cpu["normal"], W, H)
    assert not (d.view(np.uint32) == NAN32).any() and not (n.view(np.uint16) == NAN16).any()
    depth = Guard("depth_attachment", (H, W), torch.float32, W, NAN32, 4, data=d)
    normal = Guard("normal_attachment", (H, W, 4), torch.int16, 4 * W, NAN16, 8, data=n)
    out = Guard("resolved_shadows_attachment", (H, W), torch.float32, W, OUT32, 4, fill=FILL_F32)
    sub = copy.copy(f)
    sub.W, sub.H = W, H
    sub.rctx = dataclasses.replace(f.rctx, depth_attachment=ImageAttachment.depth(depth.tensor), normal_attachment=normal.tensor,
                                   resolved_shadows_attachment=ImageAttachment.depth(out.tensor), resolution=(float(W), float(H)))
    st = {}
    want = _resolve_want(f, cpu, d, n, W, H, st)

    def compare(what):
        got = sub.got()
        bad = _where(got.view(np.uint32), want.view(np.uint32))
        assert not bad, f"{label}, {what}: resolved_shadows_attachment differs from the checker, first at (y, x) {bad}"
        out.check(f"{label}, {what}", want)
        depth.check(f"{label}, {what}")
        normal.check(f"{label}, {what}")

    renderer.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 1)
    try:
        renderer.resolve_shadowmap(sub.rctx)
        compare("counting")
        dev = renderer.debug_vsm_resolve_stats()
    finally:
        renderer.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 0)
    c = resolve_counts(st, want)
    assert c["non_sky"] >= 1, (label, c)
    assert dev == {"non_sky_pixels": c["non_sky"], "taps": c["taps"], "misses": c["misses"], "fallback_minus": c["fallback_minus"],
                   "fallback_plus": c["fallback_plus"], "hard": c["hard"], "no_blocker": c["no_blocker"], "all_blockers": c["all_blockers"]}, (label, dev, c)
    out.refill()
    renderer.resolve_shadowmap(sub.rctx)
    compare("plain")


def test_shadow_resolve_sweep_on_the_device_frame_is_not_degenerate(resolve_frame):
    """The conditions tests/test_pixel_pass_edge_cases.py proves on the models' frame, on the frame the device drew."""
    f, cpu = resolve_frame
    per = {}
    for W, H in EXTENTS:
        st = {}
        got = _resolve_want(f, cpu, resample(cpu["depth"], W, H), resample(cpu["normal"], W, H), W, H, st)
        per[(W, H)] = resolve_counts(st, got)
    assert_resolve_sweep_is_not_degenerate(per)
