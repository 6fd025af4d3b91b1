"""oxc_apply_eye_adaptation on the GPU: every byte of the histogram and of the exposure buffer equal to tests/eye_adaptation_model.py's --
the library's own lit frame in both formats; the tiny extents with both outputs between guard bands and the grid capped to 1 and 3 blocks;
the contention cases at 256 x 256; hand-made texels and exposure buffers no sane frame has; five frames on one exposure buffer; all seven
passes in one captured graph replayed three times; invalid arguments."""
import dataclasses

import numpy as np
import pytest
import torch

from gpu_passes import ALL_FLAGS, DrawnFrame, Guard, ONE_ONE, lights_tensor, same, words_tensor
from gpu_passes import EYE_COMPONENT as COMPONENT
from gpu_passes import EYE_DEFAULTS as DEFAULTS
from gpu_passes import eye_context as make_context
from gpu_passes import eye_want_of as want_of
from pbr_apply_model import TRANSPARENT_BACKGROUND
from pixel_rules import pack_b10g11r11
from scenes import NAN16, NAN32

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = pytest.mark.parametrize("fmt", [0, 1], ids=["b10g11r11", "rgba16f"])
POISON = 0xFFFFFFFB  # what the histogram and the exposure buffer hold before a call: no count of these images and no stored float


def pack_image(r, g, b, fmt) -> np.ndarray:
    """Three binary32 planes [H, W] as the image oxc_apply_pbr would write: uint32 [H, W] or uint16 [H, W, 4] with alpha 1."""
    if fmt == 0:
        return pack_b10g11r11(r.reshape(-1), g.reshape(-1), b.reshape(-1)).astype(np.uint32).reshape(r.shape)
    with np.errstate(over="ignore"):
        return np.stack([r, g, b, np.ones_like(r)], axis=-1).astype(np.float16).view(np.uint16)


def random_image(W, H, fmt, seed, lo=-13.0, hi=14.0) -> np.ndarray:
    """Finite texels whose channels are log-uniform over 2^lo .. 2^hi, a twentieth of them black."""
    rng = np.random.default_rng(seed)
    planes = [np.where(rng.random((H, W)) < 0.05, 0.0, np.exp2(rng.uniform(lo, hi, (H, W)))).astype(np.float32) for _ in range(3)]
    return pack_image(*planes, fmt)


def grey_image(values, fmt) -> np.ndarray:
    v = np.asarray(values, dtype=np.float32)
    return pack_image(v, v, v, fmt)


def upload(image: np.ndarray) -> torch.Tensor:
    view = np.int32 if image.dtype == np.uint32 else np.int16
    return torch.from_numpy(np.ascontiguousarray(image).view(view).copy()).cuda()


def got_of(ctx):
    torch.cuda.synchronize()
    return ctx.histogram_buffer.cpu().numpy().view(np.uint32).copy(), ctx.exposure_buffer.cpu().numpy().view(np.uint32).copy()


def run_and_check(r, image: np.ndarray, label, exposure_words=ONE_ONE, time_coeff=1.0, settings=DEFAULTS):
    """One call on a fresh context; returns the checker's (histogram, exposure words)."""
    ctx = make_context(upload(image), words_tensor(exposure_words), time_coeff, settings)
    want = want_of(ctx, exposure_words)
    r.apply_eye_adaptation(ctx)
    same(got_of(ctx), want, label)
    return want


# ---- 1. the drawn frame ---------------------------------------------------------------------------------------------------------------------------
@FORMATS
def test_drawn_frame(renderer, fmt):
    """The 192 x 192 frame drawn, decoded, resolved, occluded and lit by the library's own passes: the histogram and the exposure equal the
    checker's, the frame spreads over several bins, and the source image is unchanged."""
    frame = DrawnFrame(renderer)
    frame.passes()
    pbr = frame.pbr(ALL_FLAGS | (TRANSPARENT_BACKGROUND if fmt else 0), lights_tensor(frame.four_lights()))
    renderer.apply_pbr(pbr)
    torch.cuda.synchronize()
    before = pbr.final_attachment.clone()
    ctx = make_context(pbr.final_attachment, words_tensor(ONE_ONE), time_coeff=0.25, settings=COMPONENT)
    assert ctx.source_format == fmt and (ctx.width, ctx.height) == (192, 192)
    want = want_of(ctx, ONE_ONE)
    renderer.apply_eye_adaptation(ctx)
    same(got_of(ctx), want, "drawn frame")
    assert int(want[0].sum()) == 192 * 192 and (want[0] > 0).sum() >= 4, want[0]
    assert torch.equal(pbr.final_attachment, before)


# ---- 2. extents between guard bands -----------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1), (1, 2), (3, 1), (2, 3), (5, 7), (63, 1), (64, 64), (65, 63), (129, 65)]


@pytest.mark.parametrize("extent", EXTENTS, ids=[f"{w}x{h}" for w, h in EXTENTS])
@FORMATS
def test_extent_between_guard_bands(renderer, extent, fmt):
    """The image, the histogram and the exposure buffer each a window in a larger poisoned buffer, the image at the least alignment the ABI
    demands (so the texels before the first 16-byte boundary are there): a load outside the image is one count too many, a store outside an
    output changes a band.  Again with the grid capped to 1 and to 3 blocks: every block walks its stride loop several times."""
    from oxylus_amd import lib as L

    W, H = extent
    image = random_image(W, H, fmt, seed=23 + W)
    if fmt == 0:
        src = Guard("final_attachment", (H, W), torch.int32, W, NAN32, 4, data=image)
    else:
        src = Guard("final_attachment", (H, W, 4), torch.int16, 4 * W, NAN16, 8, data=image)
    hist = Guard("histogram_buffer", (256,), torch.int32, 256, 0xFFFFFFF7, 4, fill=POISON)
    start = np.array([0.5, 2.0], dtype=np.float32).view(np.uint32)
    exposure = Guard("exposure_buffer", (2,), torch.float32, 2, 0xFFFFFFF7, 4, data=start.view(np.float32))
    ctx = dataclasses.replace(make_context(src.tensor, exposure.tensor, time_coeff=0.5), histogram_buffer=hist.tensor)
    want = want_of(ctx, start)
    assert int(want[0].sum()) == W * H
    try:
        for cap in (0, 1, 3):
            renderer.debug_set_tuning(L.TUNE_EYE_ADAPTATION_GRID, cap)
            hist.refill()
            exposure.tensor.copy_(words_tensor(start))
            renderer.apply_eye_adaptation(ctx)
            label = f"{W} x {H}, cap {cap}"
            same(got_of(ctx), want, label)
            for guard in (src, hist, exposure):
                guard.check(label)
    finally:
        renderer.debug_set_tuning(L.TUNE_EYE_ADAPTATION_GRID, 0)


@FORMATS
def test_every_alignment_of_the_image(renderer, fmt):
    """The image at every texel offset from a 16-byte boundary -- addresses 0, 4, 8 and 12 mod 16 (B10G11R11), 0 and 8 mod 16 (RGBA16F) --
    and with 1 to 11 and 35 texels: every count of texels before the first vector (0 to 3, 0 to 1) meets every count behind the last one,
    with and without whole vectors in between.  The buffer around the image holds poison texels; one read outside is one count too many."""
    per_texel, dtype, poison = ((1, torch.int32, NAN32), (4, torch.int16, NAN16))[fmt]
    for offset in range(16 // (8 if fmt else 4)):
        for shape in [(1, n) for n in range(1, 12)] + [(7, 5)]:
            H, W = shape
            image = random_image(W, H, fmt, seed=101 + 16 * offset + W * H)
            n = W * H * per_texel
            buf = torch.full((64 + n + 64,), poison, dtype=dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            lo = (16 + offset) * per_texel  # 16 texels are a multiple of 16 bytes in both formats
            window = buf[lo:lo + n]
            window.copy_(upload(image).reshape(-1))
            tensor = window.view((H, W) if fmt == 0 else (H, W, 4))
            assert tensor.data_ptr() % 16 == offset * (8 if fmt else 4)
            ctx = make_context(tensor, words_tensor(ONE_ONE), time_coeff=1.0)
            want = want_of(ctx, ONE_ONE)
            assert int(want[0].sum()) == W * H
            renderer.apply_eye_adaptation(ctx)
            same(got_of(ctx), want, f"{W} x {H} at {offset} texels behind a 16-byte boundary")


# ---- 3. contention and coverage ---------------------------------------------------------------------------------------------------------------------
# every bin within both formats' range and bin 1 wholly above the dark threshold (2^-9.5 = 0.00138): bin k holds log2 in -9.5 + (k - 1 .. k) * 20 / 254
WIDE = dict(min_exposure=-9.5, max_exposure=10.5, ev100_bias=1.0)


def bin_centre(k):
    return np.exp2((np.asarray(k, dtype=np.float64) - 0.5) / 254.0 * 20.0 - 9.5)


@FORMATS
def test_constant_image(renderer, fmt):
    """Every pixel in one bin: the worst case of the counting."""
    want = run_and_check(renderer, grey_image(np.full((256, 256), 0.18), fmt), "constant")
    assert sorted(want[0].tolist())[-2:] == [0, 65536]


@FORMATS
def test_every_bin(renderer, fmt):
    """Texel i aims at the middle of bin i mod 256 (0: black, 255: beyond the range)."""
    k = (np.arange(256 * 256) % 256).reshape(256, 256)
    v = np.where(k == 0, 0.0, np.where(k == 255, 1500.0, bin_centre(k)))
    want = run_and_check(renderer, grey_image(v, fmt), "every bin", settings=WIDE)
    assert (want[0] == 256).all(), want[0]


@FORMATS
def test_two_adjacent_bins(renderer, fmt):
    """Neighbouring lanes alternate between bins 100 and 101."""
    i = np.arange(256 * 256).reshape(256, 256)
    want = run_and_check(renderer, grey_image(np.where(i % 2 == 0, bin_centre(100), bin_centre(101)), fmt), "two bins", settings=WIDE)
    assert want[0][100] == 32768 and want[0][101] == 32768


# ---- 4. hand-made texels ----------------------------------------------------------------------------------------------------------------------------
def test_handmade_b10g11r11(renderer):
    """Every exponent class of the three fields -- zero, denormal, the smallest and largest normal, +Inf, NaN -- in every combination."""
    uf11 = [0, 1, 63, 1 << 6, (15 << 6) | 17, (30 << 6) | 63, 31 << 6, (31 << 6) | 1, (31 << 6) | 63]
    uf10 = [0, 1, 31, 1 << 5, (15 << 5) | 9, (30 << 5) | 31, 31 << 5, (31 << 5) | 1, (31 << 5) | 31]
    w = np.array([r | (g << 11) | (b << 22) for r in uf11 for g in uf11 for b in uf10], dtype=np.uint32)
    want = run_and_check(renderer, w.reshape(27, 27), "exponent classes", settings=COMPONENT)
    assert want[0][0] > 0 and want[0][255] > 0


def test_handmade_rgba16f(renderer):
    """Half denormals, -0, negatives, Inf and NaN in every channel, alpha poisoned."""
    h = [0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0xBC00, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFFFF, 0x1418]
    texels = np.array([(r, g, b, 0x7E00) for r in h for g in h for b in h], dtype=np.uint16)
    want = run_and_check(renderer, texels.reshape(14, 196, 4), "half classes", settings=COMPONENT)
    assert want[0][0] > 0 and want[0][255] > 0


@FORMATS
def test_threshold_and_integer_edges(renderer, fmt):
    """Luminances around 0.001f and around the powers of two on which `mapped` is an integer, as near as the format's grid comes: a window of
    consecutive bit patterns of the format around each."""
    if fmt == 1:
        centres = [int(np.float16(v).view(np.uint16)) for v in (0.001 / 1.0001, 2.0 ** -6, 1.0, 64.0, 2.0 ** 15)]
        texels = np.array([(c + d, c + d, c + d, 0x3C00) for c in centres for d in range(-8, 9)], dtype=np.uint16).reshape(1, -1, 4)
        run_and_check(renderer, texels, "edges", settings=COMPONENT)
        run_and_check(renderer, texels, "edges, engine range")
    else:
        # one channel at a time: luminance = channel * weight, the other two zero
        fields = [(e << 6) | m for e in (5, 6, 9, 15, 21, 30) for m in (0, 1, 31, 62, 63)]
        w = np.array([f for f in fields] + [f << 11 for f in fields] + [(f >> 1) << 22 for f in fields], dtype=np.uint32).reshape(1, -1)
        run_and_check(renderer, w, "edges", settings=COMPONENT)
        run_and_check(renderer, w, "edges, engine range")


def test_exact_luminance_edges_through_one_channel(renderer):
    """RGBA16F green = v, the others zero: luminance = v * 0.7152f.  The halves around 0.001f / 0.7152f straddle the dark threshold; the
    checker says which side each falls on, both sides occur."""
    c = int(np.float16(0.001 / 0.7152).view(np.uint16))
    texels = np.array([(0, c + d, 0, 0) for d in range(-4, 5)], dtype=np.uint16).reshape(1, -1, 4)
    want = run_and_check(renderer, texels, "green threshold", settings=COMPONENT)
    assert 0 < want[0][0] < 9


# ---- 5. hand-made exposure buffers ------------------------------------------------------------------------------------------------------------------
EXPOSURE_WORDS = [0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0xBF800000, 0x00000001, 0x007FFFFF,
                  0x807FFFFF, 0x7F7FFFFF, 0x3E99999A]


@pytest.mark.parametrize("time_coeff", [0.0, 0.3, 1.0])
def test_handmade_exposure_buffers(renderer, time_coeff):
    """NaN, Inf, 0, negative and denormal adapted_luminance (and a poisoned exposure word, which is not read)."""
    image_t = upload(random_image(33, 17, 0, seed=5))
    for word in EXPOSURE_WORDS:
        start = np.array([word, POISON], dtype=np.uint32)
        ctx = make_context(image_t, words_tensor(start), time_coeff)
        want = want_of(ctx, start)
        renderer.apply_eye_adaptation(ctx)
        same(got_of(ctx), want, f"adapted_luminance 0x{word:08X}, time_coeff {time_coeff}")
        assert want[1][0] != POISON and want[1][1] != POISON


# ---- 6. five frames on one exposure buffer ----------------------------------------------------------------------------------------------------------
@FORMATS
def test_five_frames_on_one_exposure_buffer(renderer, fmt):
    """The images change and time_coeff varies (0 and 1 among them); after every call the buffer equals the checker's chain.  The last frame
    goes through the renderer's own time_coeff (adaptation_speed, delta_time), taken as given by the checker."""
    from oxylus_amd.renderer import exposure_buffer, eye_adaptation_time_coeff

    exposure = exposure_buffer()
    assert exposure.cpu().numpy().view(np.uint32).tolist() == ONE_ONE.tolist()
    words = ONE_ONE
    for k, tc in enumerate([0.018, 0.0, 0.5, 1.0, None]):
        image_t = upload(random_image(65, 63, fmt, seed=40 + k, lo=-13.0 + 2 * k, hi=4.0 + 2 * k))
        ctx = make_context(image_t, exposure, tc)
        if tc is None:
            given = eye_adaptation_time_coeff(ctx.adaptation_speed, 1.0 / 60.0)
            assert 0.018 < given < 0.0185  # 1 - exp(-1.1 / 60)
            want = want_of(dataclasses.replace(ctx, time_coeff=given), words)
        else:
            want = want_of(ctx, words)
        renderer.apply_eye_adaptation(ctx, delta_time=1.0 / 60.0)
        same(got_of(ctx), want, f"frame {k}")
        if tc == 0.0:
            assert want[1][0] == words[0]
        words = want[1]


# ---- 7. all seven passes in one captured graph ------------------------------------------------------------------------------------------------------
def test_seven_passes_in_one_graph(renderer):
    """Draw -> decode -> resolve -> contact shadows -> ambient occlusion -> apply -> eye adaptation captured into one graph and replayed three
    times with the lights changed between the replays: after each replay the histogram and the exposure equal the checker's chain from the
    image that replay wrote.  Captured with the default queue settings."""
    frame = DrawnFrame(renderer)
    frame.passes()
    sets = [lights_tensor(frame.four_lights(shift)) for shift in (0.0, 0.3, -0.2)]
    lights = sets[0].clone()
    pbr = frame.pbr(ALL_FLAGS, lights)
    renderer.apply_pbr(pbr)
    exposure = words_tensor(ONE_ONE)
    ctx = make_context(pbr.final_attachment, exposure, time_coeff=0.4, settings=COMPONENT)
    renderer.apply_eye_adaptation(ctx)  # eager once
    same(got_of(ctx), want_of(ctx, ONE_ONE), "eager")
    exposure.copy_(words_tensor(ONE_ONE))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        frame.passes(stream)
        renderer.apply_pbr(pbr, stream=stream)
        renderer.apply_eye_adaptation(ctx, stream=stream)
    words, histograms = ONE_ONE, []
    for replay, s in enumerate(sets):
        pbr.final_attachment.fill_(-5)
        ctx.histogram_buffer.fill_(-5)
        lights.copy_(s)
        torch.cuda.synchronize()
        g.replay()
        want = want_of(ctx, words)  # from the image this replay wrote
        same(got_of(ctx), want, f"replay {replay}")
        words = want[1]
        histograms.append(want[0])
    assert (histograms[0] != histograms[1]).any() and (histograms[1] != histograms[2]).any()  # the lights show


# ---- 8. invalid arguments ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L

    W, H = 24, 16
    images = {0: upload(random_image(W, H, 0, seed=3)), 1: upload(random_image(W, H, 1, seed=3))}
    start = np.array([0x3F000000, POISON], dtype=np.uint32)
    exposure = words_tensor(start)
    base = {fmt: make_context(images[fmt], exposure, 0.5) for fmt in (0, 1)}
    hist = base[0].histogram_buffer
    for c in base.values():
        c.histogram_buffer = hist

    def untouched():
        torch.cuda.synchronize()
        assert (hist == -5).all() and exposure.cpu().numpy().view(np.uint32).tolist() == start.tolist()

    def bad(word, fmt=0, **kw):
        with pytest.raises(L.OxcError) as e:
            renderer.apply_eye_adaptation(dataclasses.replace(base[fmt], **kw))
        assert e.value.status == L.OXC_INVALID_ARG, kw
        assert "apply_eye_adaptation: " in str(e.value) and word in str(e.value), (word, str(e.value))
        untouched()

    i32 = lambda n: torch.full((n,), -5, dtype=torch.int32, device="cuda")  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad("zero", width=0)
    bad("zero", height=0)
    bad("beyond 65536", width=65537, height=1, final_attachment=i32(65537))
    bad("beyond 65536", width=1, height=65537, final_attachment=i32(65537))
    bad("2^32 - 1", width=65536, height=65536)
    bad("source_format", source_format=2)
    bad("final_attachment", final_attachment=i32(W * H - 1))
    bad("final_attachment", final_attachment=None)
    bad("final_attachment", final_attachment=i32(W * H + 1).view(torch.int16)[1:])          # 2-byte aligned
    bad("final_attachment", fmt=1, final_attachment=i32(2 * W * H - 1).view(torch.int16))   # one half-texel short
    bad("final_attachment", fmt=1, final_attachment=i32(2 * W * H + 1)[1:])                 # 4-byte aligned u16x4
    bad("final_attachment", fmt=1, final_attachment=images[0])                              # a u32 image under format 1
    bad("histogram_buffer", histogram_buffer=i32(255))
    bad("histogram_buffer", histogram_buffer=None)
    bad("histogram_buffer", histogram_buffer=i32(257).view(torch.int16)[1:])
    bad("exposure_buffer", exposure_buffer=torch.ones(1, dtype=torch.float32, device="cuda"))
    bad("exposure_buffer", exposure_buffer=None)
    bad("exposure_buffer", exposure_buffer=i32(3).view(torch.int16)[1:])
    for name in ("min_exposure", "max_exposure", "ev100_bias", "time_coeff"):
        for v in (nan, inf, -inf):
            bad("finite", **{name: v})
    bad("finite", min_exposure=-3.0e38, max_exposure=3.0e38)  # the difference overflows
    bad("above", min_exposure=18.0, max_exposure=18.0)
    bad("above", min_exposure=18.0, max_exposure=-6.0)
    lib, raw, stream = renderer._lib, renderer._ctx, renderer._stream(None)
    c = base[0].c()
    c.struct_size = 4
    assert lib.oxc_apply_eye_adaptation(raw, c, stream) == L.OXC_INVALID_ARG
    assert lib.oxc_apply_eye_adaptation(raw, None, stream) == L.OXC_INVALID_ARG
    untouched()
    # 65536 x 1 is accepted, and the contexts still run
    run_and_check(renderer, random_image(65536, 1, 0, seed=9), "65536 x 1")
    for fmt in (0, 1):
        exposure.copy_(words_tensor(start))
        want = want_of(base[fmt], start)
        renderer.apply_eye_adaptation(base[fmt])
        same(got_of(base[fmt]), want, f"after the refusals, format {fmt}")
