"""oxc_apply_pbr on the GPU: every byte of the final image equal to tests/pbr_apply_model.py's and every device counter equal to the checker's
count -- the frame drawn, decoded, resolved, contact-shadowed and occluded by the library's own passes, in both output formats, under four
lights; the 16 flag combinations with the unread images poisoned or null; the tiny extents between guard bands; light counts around the
staging chunk; hand-made texels and Light records no sane scene has; all six passes in one captured graph replayed three times with the
lights changed in between; invalid arguments."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import pbr_apply_model as PM
from pbr_apply_model import HAS_ATMOSPHERE, HAS_CONTACT_SHADOWS, HAS_DIRECTIONAL_LIGHT, HAS_SKY, TRANSPARENT_BACKGROUND
from gpu_passes import ALL_FLAGS, FILL_U16, FILL_U32, DrawnFrame, Guard, lights_tensor
from gpu_passes import pbr_context as make_context
from gpu_passes import pbr_got_of as got_of
from gpu_passes import pbr_want_of as want_of
from gpu_passes import same, upload
from scenes import CAMERA, EXTENT_IDS, EXTENTS, INV_PV, NAN16, NAN32, SKY, SUN_INTENSITY
from scenes import PBR_SUN as SUN
from scenes import synthetic_inputs

pytestmark = pytest.mark.gpu

LIGHT_CHUNK = 256  # kLightChunk of oxcull_pbr_apply.hip: lights staged per round
FILL = -5          # 0xFFFFFFFB / 0xFFFB: a pattern the pass never writes (a NaN channel is stored with an all-ones mantissa / as 0x7E00)
U32 = lambda bits: np.uint32(bits)  # noqa: E731


def run_and_check(r, ctx, label="", want=None, st=None):
    """The counting instantiation, then the plain one: both images == the checker's, the device's counters == the checker's counts.
    `want` and `st`: the checker's image and stats where the caller has them already."""
    from oxylus_amd import lib as L

    if want is None:
        st = {}
        want = want_of(ctx, st)
    r.debug_set_tuning(L.TUNE_PBR_APPLY_STATS, 1)
    try:
        ctx.final_attachment.fill_(FILL)
        r.apply_pbr(ctx)
        dev = r.debug_pbr_apply_stats()
    finally:
        r.debug_set_tuning(L.TUNE_PBR_APPLY_STATS, 0)
    same(got_of(ctx), want, label + " (counting)")
    assert dev == PM.counters(st), f"{label}: device {dev} != checker {PM.counters(st)}"
    ctx.final_attachment.fill_(FILL)
    r.apply_pbr(ctx)
    same(got_of(ctx), want, label)
    return st


# ---- 1. the drawn frame, 6. one captured graph ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("transparent", [0, TRANSPARENT_BACKGROUND], ids=["b10g11r11", "rgba16f"])
def test_drawn_frame(renderer, transparent):
    """The library's own frame under four lights: the image and the counters equal the checker's, at least three of the five pixel classes
    and all four light outcomes occur (asserted from the checker's counts), and the Directional record changes nothing."""
    frame = DrawnFrame(renderer)
    frame.passes()
    lights = frame.four_lights()
    ctx = frame.pbr(ALL_FLAGS | transparent, lights_tensor(lights))
    st = run_and_check(renderer, ctx, "four lights")
    print("checker", PM.counters(st))
    classes = [k for k in PM.COUNTER_NAMES[:5] if st[k] > 0]
    assert len(classes) >= 3, classes
    assert all(st[k] > 0 for k in PM.COUNTER_NAMES[5:]), PM.counters(st)
    assert 3 * st["light_kind_skipped"] == st["light_attenuation_out"] + st["light_ndotl_out"] + st["light_shaded"]  # one record of four
    three = frame.pbr(ALL_FLAGS | transparent, lights_tensor(lights[:3]))
    renderer.apply_pbr(three)
    same(got_of(three), got_of(ctx), "without the Directional record")
    none = frame.pbr(ALL_FLAGS | transparent, None)
    renderer.apply_pbr(none)
    assert (got_of(none) != got_of(ctx)).any()  # the lights show


def test_six_passes_in_one_graph(renderer):
    """Draw -> decode -> resolve -> contact shadows -> ambient occlusion -> apply captured into one graph and replayed three times with the
    lights changed between the replays: every replay equals the eager frame under the same lights.  Captured with the default queue settings."""
    frame = DrawnFrame(renderer)
    frame.passes()
    sets = [lights_tensor(frame.four_lights(shift)) for shift in (0.0, 0.3, -0.2)]
    lights = sets[0].clone()
    ctx = frame.pbr(ALL_FLAGS, lights)
    eager = []
    for k, s in enumerate(sets):
        lights.copy_(s)
        renderer.apply_pbr(ctx)
        eager.append(got_of(ctx))
        same(eager[k], want_of(ctx), f"eager, light set {k}")
    assert (eager[0] != eager[1]).any() and (eager[1] != eager[2]).any()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        frame.passes(stream)
        renderer.apply_pbr(ctx, stream=stream)
    d, f, a = frame.dctx, frame.f, frame.actx
    outputs = (frame.vis, d.albedo_attachment, d.normal_attachment, d.emissive_attachment, d.metallic_roughness_occlusion_attachment,
               f.rctx.resolved_shadows_attachment.data, frame.cctx.contact_shadows_attachment.data, a.depth_differences, a.noisy_occlusion,
               a.ambient_occlusion_attachment, a.prefiltered_depth.data, ctx.final_attachment)
    for replay, s in enumerate(sets):
        for t in outputs:
            t.fill_(FILL)
        lights.copy_(s)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(got_of(ctx), eager[replay], f"replay {replay}")


# ---- 2. flags -------------------------------------------------------------------------------------------------------------------------------------
TWO_LIGHTS = [dict(kind=1, position=(0.2, 0.1, 1.5), range=3.0, color=(1.0, 0.5, 0.25), intensity=8.0),
              dict(kind=2, position=(-0.5, 0.4, 2.0), direction=(0.3, -0.2, -1.0), inner_cone_angle=0.2, outer_cone_angle=0.5, range=0.0, intensity=20.0)]
FLAG_SETS = [sum(c) for n in range(5) for c in itertools.combinations((HAS_DIRECTIONAL_LIGHT, HAS_CONTACT_SHADOWS, HAS_SKY, TRANSPARENT_BACKGROUND), n)]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=[f"0x{f:03X}" for f in FLAG_SETS])
def test_flags(renderer, flags):
    """33 x 17 with empty pixels under each of the 16 flag combinations.  The image a clear flag makes unread holds NaN, then is passed as
    null: the output does not change."""
    W, H = 33, 17
    inp = synthetic_inputs(W, H, seed=7)
    assert (inp["depth"] == 0).sum() > 20
    want_st = {}
    want = PM.apply_pbr(inp["depth"], inp["albedo"], inp["normal"], inp["emissive"], inp["mro"], inp["ao"], inp["resolved"] if flags & HAS_DIRECTIONAL_LIGHT else None,
                        inp["contact"] if flags & HAS_CONTACT_SHADOWS else None, flags, INV_PV, CAMERA, SUN, SUN_INTENSITY, lights_tensor(TWO_LIGHTS).cpu().numpy(),
                        stats=want_st, **SKY)
    poisoned = dict(inp)
    if not flags & HAS_DIRECTIONAL_LIGHT:
        poisoned["resolved"] = np.full((H, W), np.nan, np.float32)
    if not flags & HAS_CONTACT_SHADOWS:
        poisoned["contact"] = np.full((H, W), np.nan, np.float32)
    dev = upload(poisoned)
    ctx = make_context(dev, flags, lights_tensor(TWO_LIGHTS))
    run_and_check(renderer, ctx, "poisoned", want=want, st=want_st)
    empty = "transparent_empty" if flags & TRANSPARENT_BACKGROUND else "sky" if flags & HAS_SKY else "fallthrough_empty"
    assert want_st[empty] == int((inp["depth"] == 0).sum()) and want_st["light_shaded"] > 0
    null = dataclasses.replace(ctx, resolved_shadows_attachment=ctx.resolved_shadows_attachment if flags & HAS_DIRECTIONAL_LIGHT else None,
                               contact_shadows_attachment=ctx.contact_shadows_attachment if flags & HAS_CONTACT_SHADOWS else None)
    null.final_attachment.fill_(FILL)
    renderer.apply_pbr(null)
    same(got_of(null), want, "null")


# ---- 3. extents between guard bands -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
@pytest.mark.parametrize("transparent", [0, TRANSPARENT_BACKGROUND], ids=["b10g11r11", "rgba16f"])
def test_extent_between_guard_bands(renderer, extent, transparent):
    """Every image a window in the middle of a larger poisoned buffer: a load outside an input reads NaN and shows as a parity failure, a
    store outside the output changes a band."""
    from oxylus_amd.renderer import ImageAttachment, PBRContext

    W, H = extent
    inp = synthetic_inputs(W, H, seed=11 + W)
    flags = ALL_FLAGS | transparent
    g = {k: Guard(k, (H, W), torch.float32, W, NAN32, 4, data=inp[k]) for k in ("depth", "resolved", "contact")}
    g.update({k: Guard(k, (H, W), torch.int32, W, NAN32, 4, data=inp[k]) for k in ("albedo", "emissive", "mro")})
    g["normal"] = Guard("normal", (H, W, 4), torch.int16, 4 * W, NAN16, 8, data=inp["normal"])
    g["ao"] = Guard("ao", (H, W), torch.int16, W, NAN16, 2, data=inp["ao"])
    if transparent:
        out = Guard("final", (H, W, 4), torch.int16, 4 * W, FILL_U16, 8, fill=FILL_U16)
    else:
        out = Guard("final", (H, W), torch.int32, W, FILL_U32, 4, fill=FILL_U32)
    lights = lights_tensor(TWO_LIGHTS)
    ctx = PBRContext.create(g["depth"].tensor, g["albedo"].tensor, g["normal"].tensor, g["emissive"].tensor, g["mro"].tensor, g["ao"].tensor,
                            g["resolved"].tensor, g["contact"].tensor, flags, INV_PV, CAMERA, SUN, SUN_INTENSITY, lights=lights, **SKY)
    ctx = dataclasses.replace(ctx, final_attachment=out.tensor)
    assert isinstance(ctx.depth_attachment, ImageAttachment)
    want = want_of(ctx)
    renderer.apply_pbr(ctx)
    same(got_of(ctx), want, f"{W} x {H}")
    out.check(f"{W} x {H}", want)
    for guard in g.values():
        guard.check(f"{W} x {H}")


# ---- 4. light counts ------------------------------------------------------------------------------------------------------------------------------
def many_lights(n, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = (1, 2, 1, 2, 0, 3)[i % 6]
        out.append(dict(kind=kind, position=tuple(rng.uniform(-1.5, 1.5, 3) + (0, 0, 1.5)), range=float(rng.choice([0.0, 1.5, 4.0])),
                        color=tuple(rng.uniform(0.1, 1.0, 3)), intensity=float(rng.uniform(0.5, 6.0)), direction=tuple(rng.uniform(-1, 1, 3) - (0, 0, 1.0)),
                        inner_cone_angle=float(rng.uniform(0.05, 0.6)), outer_cone_angle=float(rng.uniform(0.6, 1.4))))
    return out


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, LIGHT_CHUNK - 1, LIGHT_CHUNK, LIGHT_CHUNK + 1])
def test_light_counts(renderer, count):
    """16 x 16 under 0 .. 257 lights: around a wave's width and around the kernel's staging chunk of 256 lights."""
    dev = upload(synthetic_inputs(16, 16, seed=5))
    ctx = make_context(dev, ALL_FLAGS, lights_tensor(many_lights(count)))
    assert ctx.light_count == count
    st = run_and_check(renderer, ctx, f"{count} lights")
    if count >= 63:
        assert all(st[k] > 0 for k in PM.COUNTER_NAMES[5:]), PM.counters(st)


def test_light_count_below_the_buffer(renderer):
    """light_count smaller than the buffer holds: the records beyond it are not read."""
    dev = upload(synthetic_inputs(16, 16, seed=5))
    ctx = dataclasses.replace(make_context(dev, ALL_FLAGS, lights_tensor(many_lights(9))), light_count=4)
    run_and_check(renderer, ctx, "4 of 9")
    four = make_context(dev, ALL_FLAGS, lights_tensor(many_lights(9)[:4]))
    renderer.apply_pbr(four)
    same(got_of(four), got_of(ctx), "4 of 9 against 4")


# ---- 5. hand-made texels and records ----------------------------------------------------------------------------------------------------------
def odd_inputs():
    """8 x 8 of texels no sane scene has, on top of synthetic_inputs: NaN and denormal halves in the normal image, the oct point (0, 0),
    roughness bytes 0 and 255, metallic 255, emissive words with exponent 31, NaN / negative / huge ambient-occlusion halves, depth 0."""
    inp = synthetic_inputs(8, 8, seed=13, empty=0.0)
    n, e, m, ao, d = inp["normal"], inp["emissive"], inp["mro"], inp["ao"], inp["depth"]
    n[0, 0] = (0x7E00, 0x3800, 0x3800, 0x7E00)       # NaN halves
    n[0, 1] = (0x0001, 0x83FF, 0x0200, 0x8001)       # denormal halves
    n[0, 2] = (0, 0, 0, 0)                           # the oct point (0, 0): +z
    n[0, 3] = (0x8000, 0x8000, 0x3C00, 0x3C00)       # -0, and the fold's corner (1, 1)
    n[0, 4] = (0x7C00, 0xFC00, 0x7BFF, 0xFBFF)       # infinities and the largest halves
    m[1, 0], m[1, 1], m[1, 2], m[1, 3] = 0x00FF00FF, 0x00FFFFFF, 0x00000000, 0xFFFF00FF  # roughness 0 / 255, metallic 255, occlusion 0
    e[2, 0] = (31 << 6) | (31 << 17) | (31 << 27)    # +Inf in all three
    e[2, 1] = ((31 << 6) | 1) | (((31 << 6) | 63) << 11) | (((31 << 5) | 7) << 22)  # NaNs
    e[2, 2] = 1 | (1 << 11) | (1 << 22)              # the smallest denormals
    e[2, 3] = 0xFFFFFFFF
    ao[3, 0], ao[3, 1], ao[3, 2], ao[3, 3], ao[3, 4] = 0x7E00, 0xBC00, 0x7C00, 0x0001, 0x7BFF  # NaN, -1, +Inf, a denormal, 65504
    d[4, 0], d[4, 1] = 0.0, -0.0                     # empty with no sky flag: the arithmetic runs on
    d[4, 2], d[4, 3], d[4, 4] = np.nan, np.inf, -1.0
    return inp


def odd_lights(world):
    """Records no sane scene has.  `world`: the world position of pixel (5, 5), for the light that sits exactly on a pixel."""
    nan, inf, ninf, nz = U32(0x7FC00000), U32(0x7F800000), U32(0xFF800000), U32(0x80000000)
    base = dict(kind=1, position=(0.1, 0.2, 1.2), range=2.5, intensity=5.0)
    spot = dict(kind=2, position=(0.0, 0.3, 1.8), direction=(0.1, -0.1, -1.0), inner_cone_angle=0.3, outer_cone_angle=0.7, range=0.0, intensity=9.0)
    out = [dict(base, position=tuple(U32(np.float32(w).view(np.uint32)) for w in world)),  # 0 / 0
           dict(base, intensity=0.0), dict(base, intensity=-1.0), dict(base, intensity=nz), dict(base, range=-1.0), dict(base, range=1e-3), dict(base, range=nz),
           dict(spot, inner_cone_angle=0.5, outer_cone_angle=0.5), dict(spot, direction=(0.0, 0.0, 0.0)), dict(spot, inner_cone_angle=0.9, outer_cone_angle=0.2),
           dict(spot, outer_cone_angle=3.0e7), dict(spot, inner_cone_angle=-0.3), dict(spot, outer_cone_angle=16777216.0),
           dict(base, kind=0xFFFFFFFF), dict(base, kind=3)]
    for field in ("position", "color", "direction"):
        for bits in (nan, inf, ninf):
            for k in range(3):
                v = [0.3, 0.4, 1.0]
                v[k] = bits
                out.append(dict(spot, **{field: tuple(v)}))
    for field in ("intensity", "range", "inner_cone_angle", "outer_cone_angle"):
        for bits in (nan, inf, ninf):
            out.append(dict(spot, **{field: bits}))
    return out


@pytest.mark.parametrize("transparent", [0, TRANSPARENT_BACKGROUND], ids=["b10g11r11", "rgba16f"])
def test_hand_made_texels_and_records(renderer, transparent):
    """The output still equals the checker's: no NaN bit pattern of the arithmetic can reach the image.  One light at a time first, so that a
    difference names its record, then all of them; then a matrix whose w row gives 0 at depth 0, and a camera that makes V + L cancel."""
    inp = odd_inputs()
    dev = upload(inp)
    st = {}
    flags = HAS_DIRECTIONAL_LIGHT | HAS_CONTACT_SHADOWS | transparent  # no sky: depth 0 falls through
    PM.apply_pbr(inp["depth"], inp["albedo"], inp["normal"], inp["emissive"], inp["mro"], inp["ao"], inp["resolved"], inp["contact"], flags, INV_PV, CAMERA, SUN,
                 SUN_INTENSITY, stats=st, **SKY)
    at = int(np.flatnonzero((st["ys"] == 5) & (st["xs"] == 5))[0])
    lights = odd_lights([w[at] for w in st["world"]])
    for i, light in enumerate(lights):
        ctx = make_context(dev, flags, lights_tensor([light]))
        renderer.apply_pbr(ctx)
        same(got_of(ctx), want_of(ctx), f"light {i}: {light}")
    all_st = run_and_check(renderer, make_context(dev, flags, lights_tensor(lights)), "every odd light")
    assert all_st["fallthrough_empty"] == (0 if transparent else 2) and all_st["light_kind_skipped"] > 0 and all_st["light_shaded"] > 0
    zero_w = list(INV_PV)
    zero_w[15] = 0.0  # h.w = depth: 0 / 0 and x / 0 at the empty pixels
    run_and_check(renderer, make_context(dev, flags, lights_tensor(lights[:8]), inv_projection_view=zero_w), "zero w")
    # V + L cancels at pixel (5, 5): the camera sits at world - L * t, so V = -normalize(L)
    w = np.array([c[at] for c in st["world"]], dtype=np.float64)
    sun = np.asarray(SUN, dtype=np.float64) / np.linalg.norm(SUN)
    ctx = make_context(dev, flags, None, camera_position=tuple(w - sun * 2.0), sun_dir=tuple(sun))
    run_and_check(renderer, ctx, "V + L cancels")


# ---- 7. invalid arguments ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    W, H = 24, 16
    dev = upload(synthetic_inputs(W, H, seed=17))
    lights = lights_tensor(TWO_LIGHTS)
    ctx = make_context(dev, ALL_FLAGS, lights)
    tctx = make_context(dev, ALL_FLAGS | TRANSPARENT_BACKGROUND, lights)
    ctx.final_attachment.fill_(FILL)
    tctx.final_attachment.fill_(FILL)

    def bad(word, base=ctx, **kw):
        """The call is refused, and for the reason the case is about: `word` is what tells that limit's message from the others."""
        c = dataclasses.replace(base, **kw)
        with pytest.raises(L.OxcError) as e:
            renderer.apply_pbr(c)
        assert e.value.status == L.OXC_INVALID_ARG, kw
        assert "apply_pbr: " in str(e.value) and word in str(e.value), (word, str(e.value))

    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    i16 = lambda *shape: torch.zeros(shape, dtype=torch.int16, device="cuda")  # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    for name in ("albedo_attachment", "emissive_attachment", "metallic_roughness_occlusion_attachment"):
        bad("one aligned u32 per pixel", **{name: None})
        bad("one aligned u32 per pixel", **{name: i32(H - 1, W)})
        bad("one aligned u32 per pixel", **{name: i16(2 * H * W + 1)[1:]})  # 2-byte aligned only
    bad("normal_attachment", normal_attachment=None)
    bad("normal_attachment", normal_attachment=i16(H - 1, W, 4))
    bad("normal_attachment", normal_attachment=i16(H * W * 4 + 2)[2:])  # 4-byte aligned only
    bad("ambient_occlusion_attachment", ambient_occlusion_attachment=None)
    bad("ambient_occlusion_attachment", ambient_occlusion_attachment=i16(H - 1, W))
    bad("ambient_occlusion_attachment", ambient_occlusion_attachment=torch.zeros(2 * H * W + 1, dtype=torch.int8, device="cuda")[1:])  # odd address
    for name in ("resolved_shadows_attachment", "contact_shadows_attachment"):
        bad(name, **{name: None})
        bad(name, **{name: ImageAttachment.depth(f32(H + 1, W))})
        bad(name, **{name: ImageAttachment(f32(2 * H * W).view(-1), W, H, 2, [0, 4 * W * H])})
        bad(name, **{name: ImageAttachment(f32(H * W + 1).view(-1), W, H, 1, [4])})
    bad("final_attachment", final_attachment=None)
    bad("final_attachment", final_attachment=i32(H - 1, W))
    bad("final_attachment", tctx, final_attachment=i32(H, W))              # half the bytes the u16x4 image needs
    bad("final_attachment", tctx, final_attachment=i16(H * W * 4 + 2)[2:])  # 4-byte aligned only
    bad("lights_buffer", lights_buffer=None)
    bad("lights_buffer", lights_buffer=lights[:64])
    bad("lights_buffer", lights_buffer=torch.zeros(129, dtype=torch.uint8, device="cuda")[1:])
    bad("must not be zero", depth_attachment=ImageAttachment(dev["depth"].view(-1)[:0], 0, 0, 1, [0]))
    taller = ImageAttachment.depth(f32(H + 1, W))  # the shadow images follow the depth, so it is the H x W texels of the u32 buffers that refuse it
    bad("one aligned u32 per pixel", depth_attachment=taller, resolved_shadows_attachment=taller, contact_shadows_attachment=taller)
    bad("one R32F level at offset 0", depth_attachment=ImageAttachment(dev["depth"].view(-1), W, H, 2, [0, 4 * W * H]))  # two levels
    bad("one R32F level at offset 0", depth_attachment=ImageAttachment(dev["depth"].view(-1), W, H, 1, [4]))
    # the 65536-a-side limit alone: a 65537 x 1 image with every buffer large enough for it, and 65536 x 1 is accepted
    wide = upload(synthetic_inputs(65537, 1, seed=19))
    wctx = make_context(wide, ALL_FLAGS, lights)
    bad("beyond 65536", wctx)
    row = lambda t: t[:, :65536].contiguous()  # noqa: E731
    run_and_check(renderer, make_context({k: row(v) for k, v in wide.items()}, ALL_FLAGS, lights), "65536 x 1")
    bad("HasAtmosphere", scene_flags=ALL_FLAGS | HAS_ATMOSPHERE)
    nan, inf = float("nan"), float("inf")
    m = list(INV_PV)
    m[5] = nan
    bad("finite", inv_projection_view=m)
    bad("finite", camera_position=(0.0, inf, 0.0))
    bad("finite", sun_dir=(nan, 0.0, 1.0))
    bad("finite", sun_intensity=inf)
    bad("finite", base_ambient_color=(0.03, nan, 0.03))
    bad("finite", sky_solid_color=(0.0, 0.0, 0.0, -inf))
    bad("finite", sky_ambient_color=(inf, 0.0, 0.0))
    lib, raw, stream = renderer._lib, renderer._ctx, renderer._stream(None)
    c = ctx.c()
    c.struct_size = 4
    assert lib.oxc_apply_pbr(raw, c, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.width += 1  # the extent differs from the depth's
    assert lib.oxc_apply_pbr(raw, c, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.width = c.height = 0
    assert lib.oxc_apply_pbr(raw, c, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.depth_attachment.dptr = None
    assert lib.oxc_apply_pbr(raw, c, stream) == L.OXC_INVALID_ARG
    assert lib.oxc_apply_pbr(raw, None, stream) == L.OXC_INVALID_ARG
    torch.cuda.synchronize()
    assert (ctx.final_attachment == FILL).all() and (tctx.final_attachment == FILL).all()  # nothing was launched
    run_and_check(renderer, ctx, "after the refusals")  # and the context still runs
