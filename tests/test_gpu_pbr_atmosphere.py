"""oxc_apply_pbr_atmosphere on the GPU against tests/pbr_atmosphere_model.py: every word of the image equal to the checker's, the output and the
four sky images between poisoned guard bands (pbr_atmosphere_frames.run).  The synthetic frames read random sky images, the last test the
LUTs and the cube the library's own three producers wrote."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import atmosphere_frames as AF
import pbr_atmosphere_frames as PF
import pbr_atmosphere_model as AP
import sky_ibl_frames as SF
from pbr_apply_model import HAS_ATMOSPHERE, HAS_CONTACT_SHADOWS, HAS_DIRECTIONAL_LIGHT, TRANSPARENT_BACKGROUND
from refusals import NULL, SHORT, raises_refusal
from scenes import EXTENT_IDS, EXTENTS, INV_PV, synthetic_inputs

pytestmark = pytest.mark.gpu

FLAG_SETS = [sum(c) for n in range(4) for c in itertools.combinations((HAS_DIRECTIONAL_LIGHT, HAS_CONTACT_SHADOWS, TRANSPARENT_BACKGROUND), n)]
FORMATS = dict(argvalues=[0, TRANSPARENT_BACKGROUND], ids=["b10g11r11", "rgba16f"])


@pytest.fixture(scope="module")
def r():
    from oxylus_amd.renderer import RendererInstance

    inst = RendererInstance(0)
    yield inst
    inst.close()


def _no_nan(image, label):
    if image.dtype == np.uint16:
        bad = ((image & 0x7C00) == 0x7C00) & ((image & 0x03FF) != 0) & (image != 0x7E00)
    else:  # UF11 / UF11 / UF10: a NaN channel is stored with an all-ones mantissa only
        bad = np.zeros(image.shape, bool)
        for shift, mbits in ((0, 6), (11, 6), (22, 5)):
            ch = (image >> shift) & ((1 << (5 + mbits)) - 1)
            m = ch & ((1 << mbits) - 1)
            bad |= ((ch >> mbits) == 31) & (m != 0) & (m != (1 << mbits) - 1)
    assert not bad.any(), f"{label}: a NaN bit pattern of the arithmetic reached the image"


@pytest.mark.parametrize("flags", FLAG_SETS, ids=[f"0x{f:03X}" for f in FLAG_SETS])
def test_flags(r, flags):
    """33 x 17 under the 8 combinations of the three flags that are read, the sun looking at one empty pixel.  The image a clear flag makes
    unread holds NaN, then is passed as null: the output does not change.  HasAtmosphere set or clear changes nothing."""
    from gpu_passes import lights_tensor, same, upload

    inp = PF.frame()
    sun, _ = PF.sun_at_empty_pixel(inp)
    A = PF.atmosphere("near")
    sky = PF.sky_images(A)
    counts = {}
    lt = lights_tensor(PF.TWO_LIGHTS)
    expected = PF.want(inp, flags, A, sky, lt.cpu().numpy(), sun_dir=sun, counts=counts)
    poisoned = dict(inp)
    if not flags & HAS_DIRECTIONAL_LIGHT:
        poisoned["resolved"] = np.full(inp["depth"].shape, np.nan, np.float32)
    if not flags & HAS_CONTACT_SHADOWS:
        poisoned["contact"] = np.full(inp["depth"].shape, np.nan, np.float32)
    PF.run(r, poisoned, flags, A, sky, "poisoned", PF.TWO_LIGHTS, expected=expected, sun_dir=sun)
    dev = upload(inp)
    dev["resolved"] = dev["resolved"] if flags & HAS_DIRECTIONAL_LIGHT else None
    dev["contact"] = dev["contact"] if flags & HAS_CONTACT_SHADOWS else None
    PF.run(r, inp, flags, A, sky, "null", PF.TWO_LIGHTS, dev=dev, expected=expected, sun_dir=sun)
    PF.run(r, inp, flags | HAS_ATMOSPHERE, A, sky, "HasAtmosphere set", PF.TWO_LIGHTS, expected=expected, sun_dir=sun)
    empty = int((inp["depth"] == 0).sum())
    if flags & TRANSPARENT_BACKGROUND:
        assert counts["transparent_empty"] == empty
    else:
        assert counts["sky_hit"] > 0 and counts["sky_in_disc"] > 0 and counts["sky_outside_disc"] > 0
    assert counts["aerial_near_slice"] > 0 and counts["aerial_zero_depth"] > 0 and counts["light_shaded"] > 0


@pytest.mark.parametrize("start", ["near", "far"])
@pytest.mark.parametrize("transparent", **FORMATS)
def test_both_aerial_arms(r, start, transparent):
    A = PF.atmosphere(start)
    counts = {}
    PF.run(r, PF.frame(), PF.ALL_READ | transparent, A, PF.sky_images(A), start, PF.TWO_LIGHTS, counts=counts)
    assert (counts["aerial_near_slice"] > 0) == (start == "near")


@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
@pytest.mark.parametrize("transparent", **FORMATS)
def test_extents(r, extent, transparent):
    W, H = extent
    A = PF.atmosphere("far")
    PF.run(r, synthetic_inputs(W, H, seed=11 + W), PF.ALL_READ | transparent, A, PF.sky_images(A), f"{W} x {H}", PF.TWO_LIGHTS)


@pytest.mark.parametrize("sizes", [dict(transmittance=(2, 2), sky_view=(2, 2), aerial=(1, 1, 1)), dict(aerial=(4, 4, 4)), dict(aerial=(2, 3, 1)),
                                   dict(transmittance=(17, 9), sky_view=(17, 9), aerial=(16, 16, 3))], ids=["2x2 1x1x1", "4x4x4", "2x3x1", "17x9 16x16x3"])
@pytest.mark.parametrize("cube_size", [1, 2, 32])
def test_lut_and_cube_sizes(r, sizes, cube_size):
    for start in ("near", "far"):
        A = PF.atmosphere(start, **sizes)
        PF.run(r, PF.frame(), PF.ALL_READ, A, PF.sky_images(A, cube_size), f"{sizes} cube {cube_size} {start}", PF.TWO_LIGHTS)


HALF_SPECIALS = (0x7E00, 0x7C00, 0xFC00, 0x0001, 0x83FF, 0x7BFF)  # NaN, +Inf, -Inf, denormals, HALF_MAX


def _hostile(image, seed):
    """Every third texel gets one special half in one channel."""
    image = image.copy()
    flat = image.reshape(-1, 4)
    rng = np.random.default_rng(seed)
    for i in range(0, flat.shape[0], 3):
        flat[i, rng.integers(0, 4)] = HALF_SPECIALS[(i // 3) % len(HALF_SPECIALS)]
    return image


@pytest.mark.parametrize("transparent", **FORMATS)
def test_hostile_texels(r, transparent):
    """NaN, Inf and denormal halves in the normal image, in each LUT and in the cube, one image at a time and all at once; cube alpha 0 (the
    never-written cube); a matrix whose h.w is 0 at depth 0; the sun straight up, straight down and at both smoothstep edges."""
    flags = PF.ALL_READ | transparent
    inp = PF.frame()
    A = PF.atmosphere("far")
    sky = PF.sky_images(A)
    bad_normal = dict(inp, normal=_hostile(inp["normal"], 1))
    _no_nan(PF.run(r, bad_normal, flags, A, sky, "normal", PF.TWO_LIGHTS), "normal")
    for k, name in enumerate(sky):
        _no_nan(PF.run(r, inp, flags, A, dict(sky, **{name: _hostile(sky[name], 2 + k)}), name, PF.TWO_LIGHTS), name)
    everything = {name: _hostile(sky[name], 9 + k) for k, name in enumerate(sky)}
    _no_nan(PF.run(r, bad_normal, flags, A, everything, "every image", PF.TWO_LIGHTS), "every image")
    zero_cube = dict(sky, cube=np.zeros_like(sky["cube"]))
    PF.run(r, inp, flags, A, zero_cube, "the never-written cube", PF.TWO_LIGHTS)
    zero_w = list(INV_PV)
    zero_w[15] = 0.0  # h.w = depth: 0 / 0 and x / 0 at the empty pixels
    _no_nan(PF.run(r, inp, flags, A, sky, "zero w", PF.TWO_LIGHTS, inv_projection_view=zero_w), "zero w")
    for sun in ((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.995, -0.1, 0.0), (0.954, 0.3, 0.0), (0.0, 0.0, 0.0)):
        _no_nan(PF.run(r, inp, flags, A, sky, f"sun {sun}", PF.TWO_LIGHTS, sun_dir=sun), f"sun {sun}")


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_light_counts(r, count):
    """16 x 16 around kLightChunk, the kernel's staging chunk of 256 lights."""
    from test_gpu_pbr_apply import many_lights

    A = PF.atmosphere("far")
    counts = {}
    PF.run(r, synthetic_inputs(16, 16, seed=5), PF.ALL_READ, A, PF.sky_images(A), f"{count} lights", many_lights(count), counts=counts)
    if count >= 255:
        assert all(counts[k] > 0 for k in AP.COUNT_NAMES[8:]), counts


# ---- the real chain ------------------------------------------------------------------------------------------------------------------------------
def test_the_real_chain_eager_and_in_one_graph(r):
    """generate_sky_luts -> draw_atmosphere -> generate_sky_ibl (two frames: the second has history) -> the library's own drawn frame ->
    apply_pbr_atmosphere, at small engine-shaped sizes: the image equals the checker fed the device's LUTs and cube and holds sky and lit
    pixels.  Then the chain captured into one graph with the default queue settings and replayed twice: each replay equals the eager result
    for the same frame_index (the cube zeroed before each, as before the eager run)."""
    from gpu_passes import ALL_FLAGS, DrawnFrame, lights_tensor, same
    from oxylus_amd.renderer import PBRAtmosphereContext, SkyIblContext, SkyLutContext

    frame = DrawnFrame(r)
    frame.passes()
    pbr = frame.pbr(ALL_FLAGS, lights_tensor(frame.four_lights()))
    A = AF.small_atmosphere(transmittance=(32, 8), sky_view=(24, 12), aerial=(8, 8, 4), aerial_perspective_start_km=0.05)
    cam = (tuple(float(v) for v in pbr.camera_position), [float(v) for v in pbr.inv_projection_view])
    sun = tuple(float(v) for v in pbr.sun_dir)
    table = torch.from_numpy(AF.hemisphere()).cuda()
    guards = AF.lut_guards(A)
    luts = SkyLutContext(AF.renderer_atmosphere(A), table, guards[0].tensor, guards[1].tensor)
    draw = AF.draw_context(A, guards, cam, sun, pbr.sun_intensity)
    cube = SF.guard("sky_cubemap", np.zeros((6, 8, 8, 4), np.uint16))
    ibl = [SkyIblContext(draw.atmosphere, guards[2].tensor, guards[0].tensor, cube.tensor, 8, sun, float(pbr.sun_intensity), cam[0], frame_index=k) for k in (0, 1)]
    out = PF.out_guard(frame.W, frame.H, False)
    ctx = dataclasses.replace(PBRAtmosphereContext.create(pbr, draw, ibl[0]), final_attachment=out.tensor)

    def chain(stream=None):
        r.generate_sky_luts(luts, stream=stream)
        r.draw_atmosphere(draw, stream=stream)
        r.generate_sky_ibl(ibl[0], stream=stream)
        r.generate_sky_ibl(ibl[1], stream=stream)
        frame.passes(stream)
        r.apply_pbr_atmosphere(ctx, stream=stream)

    chain()
    torch.cuda.synchronize()
    u16 = lambda g, shape: g.bits()[1].reshape(shape)  # noqa: E731
    t, v, a = A.transmittance_lut_size, A.sky_view_lut_size, A.aerial_perspective_lut_size
    sky = dict(transmittance=u16(guards[0], (t[1], t[0], 4)), sky_view=u16(guards[2], (v[1], v[0], 4)), aerial=u16(guards[3], (a[2], a[1], a[0], 4)),
               cube=u16(cube, (6, 8, 8, 4)))
    assert (sky["cube"][..., 3] == SF.HALF_ONE).all() and sky["cube"][..., :3].any()
    d = pbr.depth_attachment
    img = lambda x: x.data.view(d.height, d.width).cpu().numpy()  # noqa: E731
    counts = {}
    expected, _ = AP.apply_pbr_atmosphere(img(d), pbr.albedo_attachment.cpu().numpy(), pbr.normal_attachment.cpu().numpy(), pbr.emissive_attachment.cpu().numpy(),
                                          pbr.metallic_roughness_occlusion_attachment.cpu().numpy(), pbr.ambient_occlusion_attachment.cpu().numpy(),
                                          img(pbr.resolved_shadows_attachment), img(pbr.contact_shadows_attachment), pbr.scene_flags, pbr.inv_projection_view,
                                          pbr.camera_position, pbr.sun_dir, pbr.sun_intensity, A, sky["transmittance"], sky["sky_view"], sky["aerial"], sky["cube"],
                                          pbr.lights_buffer.cpu().numpy(), pbr.light_count, counts)
    eager = PF.got_of(out).reshape(expected.shape)
    out.check("eager", expected)
    same(eager, expected, "eager")
    assert counts["sky_hit"] + counts["sky_in_disc"] + counts["sky_outside_disc"] > 0 and counts["lit_nol_positive"] > 0, counts
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain(stream)
    for replay in range(2):
        cube.tensor.zero_()
        out.refill()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        out.check(f"replay {replay}")
        same(PF.got_of(out).reshape(expected.shape), eager, f"replay {replay}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal(r):
    from gpu_passes import lights_tensor, upload

    inp = synthetic_inputs(24, 16, seed=17)
    A = PF.atmosphere("far")
    sky = PF.sky_images(A)
    guards = PF.sky_guards(sky)
    out, tout = PF.out_guard(24, 16, False), PF.out_guard(24, 16, True)
    dev = upload(inp)
    lt = lights_tensor(PF.TWO_LIGHTS)
    return A, sky, guards, out, tout, PF.context(dev, PF.ALL_READ, A, guards, out.tensor, lt), PF.context(dev, PF.ALL_READ | TRANSPARENT_BACKGROUND, A, guards, tout.tensor, lt)


def _refused(r, ctx, word, outs):
    raises_refusal(lambda: r.apply_pbr_atmosphere(ctx), word, prefix="apply_pbr_atmosphere")
    for o in outs:
        o.check("refused")
        assert (o.bits()[1] == o.fill).all(), "the output was written"


ALIGNED = " must be aligned to 8 bytes"   # the sky buffers: to 8 bytes, not to a texel


def _limits(A, guards, ctx):
    """(changes to the context, the distinguishing word) of every limit on its own, in the header's order."""
    from oxylus_amd.renderer import ImageAttachment

    atm = AF.renderer_atmosphere(A)
    rep = dataclasses.replace
    H, W = ctx.depth_attachment.height, ctx.depth_attachment.width
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    i16 = lambda *shape: torch.zeros(shape, dtype=torch.int16, device="cuda")  # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    nan, inf = float("nan"), float("inf")
    m = list(INV_PV)
    m[5] = nan
    cases = [
        (dict(depth_attachment=ImageAttachment(ctx.depth_attachment.data.view(-1)[:0], 0, 0, 1, [0])), "must not be zero"),
        (dict(depth_attachment=ImageAttachment(ctx.depth_attachment.data.view(-1), W, H, 2, [0, 4 * W * H])), "one R32F level at offset 0"),
        (dict(atmosphere=rep(atm, transmittance_lut_size=(1, 3, 1))), "transmittance_lut_size"),
        (dict(atmosphere=rep(atm, transmittance_lut_size=(5, 4097, 1))), "transmittance_lut_size"),
        (dict(atmosphere=rep(atm, sky_view_lut_size=(7, 1, 1))), "sky_view_lut_size"),
        (dict(atmosphere=rep(atm, sky_view_lut_size=(4097, 4, 1))), "sky_view_lut_size"),
        (dict(atmosphere=rep(atm, aerial_perspective_lut_size=(5, 0, 2))), "every side must be in 1 .. 4096"),
        (dict(atmosphere=rep(atm, aerial_perspective_lut_size=(5, 3, 4097))), "every side must be in 1 .. 4096"),
        (dict(atmosphere=rep(atm, aerial_perspective_lut_size=(4096, 4096, 5))), "more than 2^26 texels"),
        (dict(cube_size=0), "cube_size must be in 1 .. 1024"),
        (dict(cube_size=1025), "cube_size must be in 1 .. 1024"),
        (dict(atmosphere=rep(atm, planet_radius=inf)), "planet_radius and atmos_radius must be finite"),
        (dict(atmosphere=rep(atm, planet_radius=0.0)), "planet_radius must be above 0"),
        (dict(atmosphere=rep(atm, atmos_radius=6360.0)), "atmos_radius must be above planet_radius"),
        (dict(atmosphere=rep(atm, aerial_perspective_start_km=nan)), "aerial_perspective_start_km"),
        (dict(atmosphere=rep(atm, aerial_perspective_exposure=inf)), "aerial_perspective_exposure"),
        (dict(inv_projection_view=m), "sun_intensity must be finite"),
        (dict(camera_position=(0.0, inf, 0.0)), "sun_intensity must be finite"),
        (dict(sun_dir=(nan, 0.0, 1.0)), "sun_intensity must be finite"),
        (dict(sun_intensity=inf), "sun_intensity must be finite"),
        (dict(resolved_shadows_attachment=None), "resolved_shadows_attachment"),
        (dict(contact_shadows_attachment=ImageAttachment.depth(f32(H + 1, W))), "contact_shadows_attachment"),
        (dict(albedo_attachment=None), "one aligned u32 per pixel"),
        (dict(emissive_attachment=i32(H - 1, W)), "one aligned u32 per pixel"),
        (dict(metallic_roughness_occlusion_attachment=i16(2 * H * W + 1)[1:]), "one aligned u32 per pixel"),
        (dict(normal_attachment=i16(H * W * 4 + 2)[2:]), "normal_attachment"),
        (dict(ambient_occlusion_attachment=i16(H - 1, W)), "ambient_occlusion_attachment"),
        (dict(lights_buffer=None), "lights_buffer"),
        (dict(lights_buffer=ctx.lights_buffer[:64]), "lights_buffer"),
    ]
    for name in ("sky_transmittance_lut", "sky_view_lut", "sky_aerial_perspective_lut", "sky_cubemap"):
        flat = getattr(ctx, name + "_attachment").view(-1)
        cases += [({name + "_attachment": None}, name + NULL), ({name + "_attachment": flat[2:]}, name + ALIGNED), ({name + "_attachment": flat[:-4]}, name + SHORT)]
    cases += [(dict(final_attachment=None), "final_attachment must be one aligned u32"), (dict(final_attachment=i32(H - 1, W)), "final_attachment must be one aligned u32")]
    return cases


def test_every_limit_on_its_own(r, refusal):
    A, sky, guards, out, tout, ctx, tctx = refusal
    for change, word in _limits(A, guards, ctx):
        _refused(r, dataclasses.replace(ctx, **change), word, (out, tout))
    i16 = torch.zeros(24 * 16 * 4 + 2, dtype=torch.int16, device="cuda")
    _refused(r, dataclasses.replace(tctx, final_attachment=i16[2:]), "final_attachment must be one aligned u32", (out, tout))  # 4-byte aligned only


def test_the_first_broken_rule_gives_the_message(r, refusal):
    """Each limit together with the next one of the header's order that has another message: the earlier one is named."""
    A, sky, guards, out, tout, ctx, tctx = refusal
    cases = _limits(A, guards, ctx)
    for k, (change, word) in enumerate(cases):
        later = next(((c, w) for c, w in cases[k + 1:] if w != word and not set(c) & set(change)), None)
        if later is not None:
            _refused(r, dataclasses.replace(ctx, **later[0], **change), word, (out, tout))


def test_the_output_overlapping_an_input(r, refusal):
    A, sky, guards, out, tout, ctx, tctx = refusal
    for name in ("albedo_attachment", "emissive_attachment", "metallic_roughness_occlusion_attachment"):
        _refused(r, dataclasses.replace(ctx, final_attachment=getattr(ctx, name)), "final_attachment must not overlap " + name, (out, tout))
    _refused(r, dataclasses.replace(ctx, final_attachment=ctx.depth_attachment.data.view(torch.int32)), "final_attachment must not overlap depth_attachment", (out, tout))
    _refused(r, dataclasses.replace(tctx, final_attachment=ctx.normal_attachment), "final_attachment must not overlap normal_attachment", (out, tout))
    big = PF.atmosphere("far", aerial=(24, 16, 2))
    gs = PF.sky_guards(PF.sky_images(big))
    c = dataclasses.replace(tctx, atmosphere=AF.renderer_atmosphere(big), sky_aerial_perspective_lut_attachment=gs["aerial"].tensor, final_attachment=gs["aerial"].tensor)
    _refused(r, c, "final_attachment must not overlap sky_aerial_perspective_lut", (out, tout))


def test_null_context_short_struct_size_and_the_context_still_runs(r, refusal):
    import ctypes as C

    from gpu_passes import same
    from oxylus_amd import lib as L

    A, sky, guards, out, tout, ctx, tctx = refusal
    lib = L.load()
    assert lib.oxc_apply_pbr_atmosphere(r._ctx, None, None) == L.OXC_INVALID_ARG
    assert lib.oxc_apply_pbr_atmosphere(None, None, None) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.struct_size = C.sizeof(L.PbrAtmosphereContext) - 8
    assert lib.oxc_apply_pbr_atmosphere(r._ctx, C.byref(c), None) == L.OXC_INVALID_ARG
    assert b"struct_size" in lib.oxc_last_error(r._ctx)
    torch.cuda.synchronize()
    assert (out.bits()[1] == out.fill).all() and (tout.bits()[1] == tout.fill).all()
    r.apply_pbr_atmosphere(ctx)
    inp = synthetic_inputs(24, 16, seed=17)
    from gpu_passes import lights_tensor

    same(PF.got_of(out).reshape(16, 24), PF.want(inp, PF.ALL_READ, A, sky, lights_tensor(PF.TWO_LIGHTS).cpu().numpy()), "after the refusals")
    out.refill()


def test_the_python_twin_still_refuses_the_flag(r):
    """Renderer.apply_pbr with HasAtmosphere raises and names the flag and the call to use instead."""
    from gpu_passes import ALL_FLAGS, pbr_context, upload

    ctx = pbr_context(upload(synthetic_inputs(8, 8, seed=3)), ALL_FLAGS | HAS_ATMOSPHERE)
    assert "oxc_apply_pbr_atmosphere" in raises_refusal(lambda: r.apply_pbr(ctx), "HasAtmosphere")
