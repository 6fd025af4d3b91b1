"""oxc_apply_bloom on the GPU: every byte of both pyramids equal to tests/bloom_model.py's -- the library's own lit frame in both formats with
and without the exposure of oxc_apply_eye_adaptation; an extent sweep with both pyramids between guard bands and guard gaps between the
levels, each with the tail kernel off, at its default and from level 1; hand-made texels, parameters and exposure words; every texel
alignment; all eight passes in one captured graph replayed three times; invalid arguments."""
import dataclasses

import numpy as np
import pytest
import torch

import bloom_model as BM
from gpu_passes import ALL_FLAGS, EYE_COMPONENT, ONE_ONE, DrawnFrame, eye_context, eye_want_of, lights_tensor, words_tensor
from pbr_apply_model import TRANSPARENT_BACKGROUND
from pixel_rules import pack_b10g11r11

pytestmark = pytest.mark.gpu

F = np.float32
FORMATS = pytest.mark.parametrize("fmt", [0, 1], ids=["b10g11r11", "rgba16f"])
POISON = 0xFFFFFFF7     # what the pyramids' buffers hold before a call (every UF11 / UF10 / binary16 field a NaN with a payload no store writes)
SOURCE_POISON = 0xFFFFFFFF  # around the source: NaN in every field of both formats, so one texel read outside shows in the result
BAND = 64               # texels of poison before and behind a window
TAIL_OFF, TAIL_DEFAULT, TAIL_FROM_ONE = 13, 0, 1  # OXC_TUNE_BLOOM_TAIL_LEVEL: a value >= L, the library's choice, level 1
ALL_TAILS = (TAIL_OFF, TAIL_DEFAULT, TAIL_FROM_ONE)
DEFAULTS = dict(threshold=1.0, soft_threshold=0.125, clamp_value=4.0, radius=0.75)
HAS_EYE_ADAPTATION = 1 << 2


def _i32(pattern):
    return int(np.array([pattern], dtype=np.uint32).view(np.int32)[0])


class Source:
    """The source image as a window `shift` texels behind a 16-byte boundary inside a buffer of NaN texels."""

    def __init__(self, image: np.ndarray, fmt: int, shift: int = 1):
        self.words_per_texel = 2 if fmt else 1
        H, W = image.shape[:2]
        n = W * H * self.words_per_texel
        self.buf = torch.full(((2 * BAND + shift) * self.words_per_texel + n,), _i32(SOURCE_POISON), dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo = (BAND + shift) * self.words_per_texel
        self.hi = self.lo + n
        self.host = np.ascontiguousarray(image).view(np.uint32).reshape(-1).copy()
        self.buf[self.lo:self.hi].copy_(torch.from_numpy(self.host.view(np.int32)).cuda())
        window = self.buf[self.lo:self.hi]
        self.tensor = window.view(torch.int16).view(H, W, 4) if fmt else window.view(H, W)

    def check(self, label):
        a = self.buf.cpu().numpy().view(np.uint32)
        assert (a[:self.lo] == SOURCE_POISON).all() and (a[self.hi:] == SOURCE_POISON).all() and np.array_equal(a[self.lo:self.hi], self.host), f"{label}: the source changed"


class Pyramid:
    """A pyramid whose levels lie `gap` poisoned texels apart in one buffer, `shift` texels behind a 16-byte boundary, between two bands."""

    def __init__(self, W, H, fmt, gap=3, shift=1):
        from oxylus_amd.renderer import BloomPyramid, bloom_layout

        w2, h2, levels, offsets, total = bloom_layout(W, H, fmt, gap_texels=gap)
        texel = 8 if fmt else 4
        base = (BAND + shift) * texel
        self.buf = torch.full((((2 * BAND + shift) * texel + total) // 4,), _i32(POISON), dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.offsets = [base + o for o in offsets]
        self.attachment = BloomPyramid(self.buf, w2, h2, levels, self.offsets, fmt)

    def refill(self):
        self.buf.fill_(_i32(POISON))

    def check(self, label, want_levels):
        """The whole buffer: the checker's levels where the levels lie, the poison everywhere else."""
        got = self.buf.cpu().numpy().view(np.uint32)
        want = np.full(got.size, POISON, dtype=np.uint32)
        for off, level in zip(self.offsets, want_levels):
            w = np.ascontiguousarray(level).view(np.uint32).reshape(-1)
            want[off // 4:off // 4 + w.size] = w
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{label}: {bad.size} words differ, the first at byte {4 * int(bad[0])} (levels at {self.offsets}): 0x{int(got[bad[0]]):08X} != 0x{int(want[bad[0]]):08X}"


def run_and_check(r, image: np.ndarray, fmt: int, label, exposure_words=None, tails=(TAIL_DEFAULT,), shift=1, gap=3, **params):
    """The call on `image` for every tail setting, both pyramids and the source between guard bands; `exposure_words` switches HasEyeAdaptation
    on.  Returns the checker's (D, U)."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import BloomContext

    p = {**DEFAULTS, **params}
    H, W = image.shape[:2]
    src, D, U = Source(image, fmt, shift), Pyramid(W, H, fmt, gap, shift), Pyramid(W, H, fmt, gap + 1, shift)
    exposure = words_tensor(exposure_words) if exposure_words is not None else None
    ctx = BloomContext(src.tensor, exposure, D.attachment, U.attachment, W, H, fmt, HAS_EYE_ADAPTATION if exposure_words is not None else 0, **p)
    want = BM.apply_bloom(image, fmt, exposure_words, **p)
    try:
        for tail in tails:
            r.debug_set_tuning(L.TUNE_BLOOM_TAIL_LEVEL, tail)
            D.refill()
            U.refill()
            r.apply_bloom(ctx)
            torch.cuda.synchronize()
            D.check(f"{label}, tail {tail}: bloom_downsampled", want[0])
            U.check(f"{label}, tail {tail}: bloom_upsampled", want[1])
            src.check(label)
    finally:
        r.debug_set_tuning(L.TUNE_BLOOM_TAIL_LEVEL, 0)
    if exposure is not None:
        assert exposure.cpu().numpy().view(np.uint32).tolist() == [int(w) for w in exposure_words], f"{label}: the exposure buffer changed"
    return want


def pack_image(r, g, b, fmt) -> np.ndarray:
    if fmt == 0:
        return pack_b10g11r11(r.reshape(-1), g.reshape(-1), b.reshape(-1)).astype(np.uint32).reshape(r.shape)
    with np.errstate(over="ignore"):
        return np.stack([r, g, b, np.full_like(r, 0.25)], axis=-1).astype(np.float16).view(np.uint16)


def random_image(W, H, fmt, seed, lo=-6.0, hi=4.0) -> np.ndarray:
    """Finite texels whose channels are log-uniform over 2^lo .. 2^hi (around the threshold 1 and the clamp 4), a tenth of them black."""
    rng = np.random.default_rng(seed)
    planes = [np.where(rng.random((H, W)) < 0.1, 0.0, np.exp2(rng.uniform(lo, hi, (H, W)))).astype(np.float32) for _ in range(3)]
    return pack_image(*planes, fmt)


# ---- 1. the drawn frame ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eye", [False, True], ids=["unit-exposure", "eye-adaptation"])
@FORMATS
def test_drawn_frame(renderer, fmt, eye):
    """The 192 x 192 frame drawn, decoded, resolved, occluded and lit by the library's own passes under four lights; with HasEyeAdaptation the
    exposure is what oxc_apply_eye_adaptation left in its buffer."""
    frame = DrawnFrame(renderer)
    frame.passes()
    pbr = frame.pbr(ALL_FLAGS | (TRANSPARENT_BACKGROUND if fmt else 0), lights_tensor(frame.four_lights()))
    renderer.apply_pbr(pbr)
    words = None
    if eye:
        ectx = eye_context(pbr.final_attachment, words_tensor(ONE_ONE), time_coeff=0.25, settings=EYE_COMPONENT)
        renderer.apply_eye_adaptation(ectx)
        torch.cuda.synchronize()
        words = ectx.exposure_buffer.cpu().numpy().view(np.uint32).copy()
        assert words.tolist() == eye_want_of(ectx, ONE_ONE)[1].tolist() and words[1] != 0x3F800000
    torch.cuda.synchronize()
    image = pbr.final_attachment.cpu().numpy()
    image = image.view(np.uint16) if fmt else image.view(np.uint32)
    assert image.shape[:2] == (192, 192)
    D, U = run_and_check(renderer, image, fmt, "drawn frame", words, tails=ALL_TAILS)
    assert len(D) == 7 and D[0].shape[:2] == (96, 96)
    assert np.count_nonzero(D[0][..., :3] if fmt else D[0]) > 0 and np.count_nonzero(U[0][..., :3] if fmt else U[0]) > 0  # the frame blooms


def test_the_renderer_allocates_the_pyramids(renderer):
    """BloomContext.create and BloomPyramid.level: the twin's own allocation, without guard bands."""
    from oxylus_amd.renderer import BloomContext

    for fmt in (0, 1):
        image = random_image(37, 21, fmt, seed=77)
        t = torch.from_numpy(image.view(np.int16 if fmt else np.int32).copy()).cuda()
        ctx = BloomContext.create(t, radius=0.5)
        assert (ctx.width, ctx.height, ctx.source_format, ctx.bloom_upsampled_attachment.levels) == (37, 21, fmt, 5)
        renderer.apply_bloom(ctx)
        torch.cuda.synchronize()
        D, U = BM.apply_bloom(image, fmt, None, radius=0.5)
        for k in range(5):
            view = np.uint16 if fmt else np.uint32
            assert np.array_equal(ctx.bloom_downsampled_attachment.level(k).cpu().numpy().view(view), D[k]), (fmt, k)
            assert np.array_equal(ctx.bloom_upsampled_attachment.level(k).cpu().numpy().view(view), U[k]), (fmt, k)


# ---- 2. the extent sweep --------------------------------------------------------------------------------------------------------------------------
# the smallest shapes with: L = 1 (no upsample, U is only the clear); an odd side (the half truncates, the tapped column drifts by a whole
# texel); one side reaching 1 levels before the other; outputs of 15, 16, 17 and 33 texels across a 16-wide tile
EXTENTS = [(2, 2), (3, 3), (2, 9), (9, 2), (4, 4), (5, 7), (31, 33), (32, 32), (34, 30), (66, 66), (67, 35), (129, 65), (130, 2), (258, 6)]


@pytest.mark.parametrize("extent", EXTENTS, ids=[f"{w}x{h}" for w, h in EXTENTS])
@FORMATS
def test_extent_between_guard_bands(renderer, extent, fmt):
    W, H = extent
    image = random_image(W, H, fmt, seed=11 + 3 * W + H)
    words = np.array([0x7FC00000, F(1.5).view(np.uint32)], dtype=np.uint32)
    D, U = run_and_check(renderer, image, fmt, f"{W} x {H}", words, tails=ALL_TAILS)
    assert [d.shape[:2][::-1] for d in D] == BM.geometry(W, H)[3]
    if len(U) == 1:
        assert not np.any(U[0][..., :3] if fmt else U[0])  # L = 1: the bloom is black


# ---- 3. hand-made sources -------------------------------------------------------------------------------------------------------------------------
UF11_CLASSES = [0, 1, 63, 1 << 6, (15 << 6) | 17, (30 << 6) | 63, 31 << 6, (31 << 6) | 1, (31 << 6) | 63]
UF10_CLASSES = [0, 1, 31, 1 << 5, (15 << 5) | 9, (30 << 5) | 31, 31 << 5, (31 << 5) | 1, (31 << 5) | 31]
HALF_CLASSES = [0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0xBC00, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFFFF, 0x8001, 0xC400]


@FORMATS
def test_every_number_class(renderer, fmt):
    """A finite random image with one texel in sixteen drawn from every class of the format -- zero, denormal, smallest and largest normal,
    Inf, NaN, and with RGBA16F the negatives of each -- and alpha poisoned: NaN and Inf go through the taps, the clamp, the levels and both
    chains exactly as the checker says."""
    W, H = 45, 27
    rng = np.random.default_rng(5 + fmt)
    image = random_image(W, H, fmt, seed=31)
    special = rng.random((H, W)) < 1.0 / 16.0
    if fmt == 0:
        pick = lambda classes: rng.choice(np.array(classes, dtype=np.uint32), (H, W))  # noqa: E731
        image = np.where(special, pick(UF11_CLASSES) | (pick(UF11_CLASSES) << 11) | (pick(UF10_CLASSES) << 22), image).astype(np.uint32)
    else:
        image = np.where(special[..., None], rng.choice(np.array(HALF_CLASSES, dtype=np.uint16), (H, W, 4)), image).astype(np.uint16)
        image[..., 3] = 0x7E00
    D, _ = run_and_check(renderer, image, fmt, "number classes", tails=ALL_TAILS)
    if fmt == 0:
        # min(group, clamp_value) takes every NaN and Inf to 4, and nothing in B10G11R11 is negative: the weights lie in (0, 1] and D holds no
        # NaN and no Inf whatever the source holds (RGBA16F has -Inf, which passes the min)
        assert not ((D[0] & 0x7C0) == 0x7C0).any() and not (((D[0] >> 11) & 0x7C0) == 0x7C0).any() and not ((D[0] >> 27) == 31).any()
    # the same image of pure random bits: nearly everything is NaN or Inf
    bits = rng.integers(0, 1 << 32, (H, W * (2 if fmt else 1)), dtype=np.uint64).astype(np.uint32)
    run_and_check(renderer, bits.view(np.uint16).reshape(H, W, 4) if fmt else bits, fmt, "random bits", tails=(TAIL_OFF, TAIL_DEFAULT))


@FORMATS
def test_channels_on_the_thresholds(renderer, fmt):
    """Constant patches whose groups land exactly on threshold, threshold +- knee and clamp_value, and one step of the format to either side
    (1, 0.875, 1.125 and 4 are exact in UF11, UF10 and binary16; a constant patch gives the group its own value)."""
    values = []
    for centre in (1.0, 0.875, 1.125, 4.0):
        h = int(np.float16(centre).view(np.uint16))
        step = 32  # one UF10 step of the mantissa in binary16 bits, 2^(10 - 5): exact in all three formats
        values += [float(np.array([h + d * step], dtype=np.uint16).view(np.float16)[0]) for d in (-1, 0, 1)]
    patch = 12  # wider than the 10 texels a pixel's taps reach: the middle of every patch sees the constant alone
    row = np.repeat(np.array(values, dtype=np.float32), patch)
    plane = np.tile(row, (patch, 1))
    for rgb in ((plane, plane, plane), (plane, plane * 0, plane * 0), (plane * 0, plane * F(0.5), plane)):
        run_and_check(renderer, pack_image(*[np.ascontiguousarray(c, dtype=np.float32) for c in rgb], fmt), fmt, "thresholds", tails=(TAIL_OFF, TAIL_DEFAULT))


PARAMETERS = [dict(threshold=0.0), dict(soft_threshold=0.0), dict(threshold=0.0, soft_threshold=0.0), dict(radius=0.0), dict(radius=1.0), dict(clamp_value=0.5),
              dict(clamp_value=0.0), dict(threshold=-1.0, soft_threshold=0.5), dict(radius=-0.5, clamp_value=65504.0), dict(threshold=1.0e-3, soft_threshold=1.0, radius=2.0)]


@FORMATS
def test_parameters(renderer, fmt):
    """threshold 0, knee 0, radius 0 and 1, a clamp below the threshold, and values no editor slider reaches."""
    image = random_image(41, 23, fmt, seed=8)
    blooms = []
    for params in PARAMETERS:
        _, U = run_and_check(renderer, image, fmt, f"{params}", tails=(TAIL_OFF, TAIL_DEFAULT), **params)
        blooms.append(U[0])
    assert not np.any(blooms[5][..., :3] if fmt else blooms[5])  # clamp_value 0.5 under threshold 1: nothing passes
    assert not np.array_equal(blooms[3], blooms[4])


EXPOSURE_WORDS = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x7F800001, 0xBF800000, 0xC1200000, 0x3E99999A,
                  0x7F7FFFFF, 0x3F800000]


@FORMATS
def test_handmade_exposure_words(renderer, fmt):
    """0, denormal, Inf, NaN and negative exposures (the adapted luminance beside it poisoned: it is not read), then a poisoned and a null
    exposure buffer with the flag clear: the result of exposure 1."""
    from oxylus_amd.renderer import BloomContext

    image = random_image(26, 19, fmt, seed=13)
    for word in EXPOSURE_WORDS:
        want = run_and_check(renderer, image, fmt, f"exposure 0x{word:08X}", np.array([0xFFFFFFFB, word], dtype=np.uint32), tails=(TAIL_OFF, TAIL_DEFAULT))
    unit = BM.apply_bloom(image, fmt, None, **DEFAULTS)
    assert all(np.array_equal(a, b) for a, b in zip(want[0] + want[1], unit[0] + unit[1]))  # the last word is 1.0
    H, W = image.shape[:2]
    for exposure in (words_tensor([0x7FC00000, 0x7FC00000]), None, torch.zeros(1, dtype=torch.int16, device="cuda")[1:]):
        src, D, U = Source(image, fmt), Pyramid(W, H, fmt), Pyramid(W, H, fmt)
        renderer.apply_bloom(BloomContext(src.tensor, exposure, D.attachment, U.attachment, W, H, fmt, 0xFFFFFFFF & ~HAS_EYE_ADAPTATION, **DEFAULTS))
        torch.cuda.synchronize()
        D.check("flag clear: bloom_downsampled", unit[0])
        U.check("flag clear: bloom_upsampled", unit[1])


@FORMATS
def test_every_texel_alignment(renderer, fmt):
    """The source and every level at every texel offset from a 16-byte boundary: 0, 4, 8, 12 bytes (B10G11R11), 0 and 8 (RGBA16F); the gap
    between the levels varies too, so the levels of one pyramid differ in alignment."""
    for shift in range(16 // (8 if fmt else 4)):
        for gap in (0, 1, 2):
            image = random_image(19, 11, fmt, seed=50 + shift)
            run_and_check(renderer, image, fmt, f"shift {shift}, gap {gap}", tails=(TAIL_OFF, TAIL_DEFAULT), shift=shift, gap=gap)


@FORMATS
def test_interleaved_pyramids_in_one_allocation(renderer, fmt):
    """D level 0, U level 0, D level 1, U level 1, ... one poisoned texel apart in one buffer: no level shares a byte with another, so the
    call is accepted although the two pyramids' spans overlap, and every byte outside the levels stays poison."""
    from oxylus_amd.renderer import BloomContext, BloomPyramid

    W, H = 37, 21
    image = random_image(W, H, fmt, seed=91)
    w2, h2, levels, extents = BM.geometry(W, H)
    texel = 8 if fmt else 4
    offsets, at = ([], []), BAND * texel
    for w, h in extents:
        for which in (0, 1):
            at += texel
            offsets[which].append(at)
            at += w * h * texel
    buf = torch.full(((at + BAND * texel) // 4,), _i32(POISON), dtype=torch.int32, device="cuda")
    src = Source(image, fmt)
    D, U = (BloomPyramid(buf, w2, h2, levels, offsets[which], fmt) for which in (0, 1))
    renderer.apply_bloom(BloomContext(src.tensor, None, D, U, W, H, fmt, 0, **DEFAULTS))
    torch.cuda.synchronize()
    want = BM.apply_bloom(image, fmt, None, **DEFAULTS)
    expect = np.full(buf.numel(), POISON, dtype=np.uint32)
    for which in (0, 1):
        for off, level in zip(offsets[which], want[which]):
            w = np.ascontiguousarray(level).view(np.uint32).reshape(-1)
            expect[off // 4:off // 4 + w.size] = w
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), expect)
    src.check("interleaved")


# ---- 4. all eight passes in one captured graph ------------------------------------------------------------------------------------------------------
def test_eight_passes_in_one_graph(renderer):
    """Draw -> decode -> resolve -> contact shadows -> ambient occlusion -> apply -> eye adaptation -> bloom captured into one graph on one
    stream and replayed three times with the lights changed between the replays: each replay's pyramids equal the checker's on the image that
    replay lit and on the exposure that replay's eye adaptation stored.  Captured with the default queue settings."""
    from oxylus_amd.renderer import BloomContext

    frame = DrawnFrame(renderer)
    frame.passes()
    sets = [lights_tensor(frame.four_lights(shift)) for shift in (0.0, 0.3, -0.2)]
    lights = sets[0].clone()
    pbr = frame.pbr(ALL_FLAGS, lights)
    renderer.apply_pbr(pbr)
    exposure = words_tensor(ONE_ONE)
    ectx = eye_context(pbr.final_attachment, exposure, time_coeff=0.4, settings=EYE_COMPONENT)
    D, U = Pyramid(192, 192, 0), Pyramid(192, 192, 0)
    bctx = BloomContext(pbr.final_attachment, exposure, D.attachment, U.attachment, 192, 192, 0, HAS_EYE_ADAPTATION, **DEFAULTS)
    renderer.apply_eye_adaptation(ectx)  # eager once
    renderer.apply_bloom(bctx)
    exposure.copy_(words_tensor(ONE_ONE))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        frame.passes(stream)
        renderer.apply_pbr(pbr, stream=stream)
        renderer.apply_eye_adaptation(ectx, stream=stream)
        renderer.apply_bloom(bctx, stream=stream)
    words, blooms = ONE_ONE, []
    for replay, s in enumerate(sets):
        pbr.final_attachment.fill_(-5)
        D.refill()
        U.refill()
        lights.copy_(s)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        words = eye_want_of(ectx, words)[1]  # the chain of exposures, from the image this replay wrote
        assert exposure.cpu().numpy().view(np.uint32).tolist() == words.tolist(), f"replay {replay}: exposure"
        want = BM.apply_bloom(pbr.final_attachment.cpu().numpy().view(np.uint32), 0, words, **DEFAULTS)
        D.check(f"replay {replay}: bloom_downsampled", want[0])
        U.check(f"replay {replay}: bloom_upsampled", want[1])
        blooms.append(want[1][0])
    assert (blooms[0] != blooms[1]).any() and (blooms[1] != blooms[2]).any()  # the lights show


# ---- 5. invalid arguments ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import BloomContext, BloomPyramid

    W, H = 24, 18  # (12, 9): 4 levels
    images = {fmt: random_image(W, H, fmt, seed=3) for fmt in (0, 1)}
    sources = {fmt: Source(images[fmt], fmt) for fmt in (0, 1)}
    pyramids = {fmt: (Pyramid(W, H, fmt), Pyramid(W, H, fmt)) for fmt in (0, 1)}
    start = np.array([0x3F000000, 0x3FC00000], dtype=np.uint32)
    exposure = words_tensor(start)
    base = {fmt: BloomContext(sources[fmt].tensor, exposure, pyramids[fmt][0].attachment, pyramids[fmt][1].attachment, W, H, fmt, HAS_EYE_ADAPTATION, **DEFAULTS)
            for fmt in (0, 1)}

    def untouched():
        torch.cuda.synchronize()
        for fmt in (0, 1):
            for p in pyramids[fmt]:
                p.check("refused call", [])
            sources[fmt].check("refused call")
        assert exposure.cpu().numpy().view(np.uint32).tolist() == start.tolist()

    def bad(word, fmt=0, **kw):
        with pytest.raises(L.OxcError) as e:
            renderer.apply_bloom(dataclasses.replace(base[fmt], **kw))
        assert e.value.status == L.OXC_INVALID_ARG, kw
        assert "apply_bloom: " in str(e.value) and word in str(e.value), (word, str(e.value))
        untouched()

    def pyramid(fmt=0, which=0, **kw):
        return dataclasses.replace(pyramids[fmt][which].attachment, **kw)

    i32 = lambda n: torch.full((n,), -5, dtype=torch.int32, device="cuda")  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad("at least 2", width=1)
    bad("at least 2", height=1)
    bad("at least 2", width=0, height=0)
    bad("below 8192", width=16384)
    bad("below 8192", height=16385)
    bad("source_format", source_format=2)
    bad("final_attachment", final_attachment=i32(W * H - 1))
    bad("final_attachment", final_attachment=None)
    bad("final_attachment", final_attachment=i32(W * H + 1).view(torch.int16)[1:])         # 2-byte aligned
    bad("final_attachment", fmt=1, final_attachment=i32(2 * W * H + 1)[1:])                # a 4-byte aligned u16x4
    bad("final_attachment", fmt=1, final_attachment=sources[0].tensor)                     # a u32 image under format 1
    offs = pyramids[0][0].offsets
    for name, which in (("bloom_downsampled_attachment", 0), ("bloom_upsampled_attachment", 1)):
        o = pyramids[0][which].offsets
        bad(name, **{name: pyramid(0, which, width=W // 2 + 1)})
        bad(name, **{name: pyramid(0, which, height=H // 2 - 1)})
        bad(name, **{name: pyramid(0, which, levels=3)})
        bad(name, **{name: pyramid(0, which, levels=5, level_offset=o + [o[-1] + 8])})
        bad(name + ": every level", **{name: pyramid(0, which, data=None)})
        bad(name + ": every level", **{name: pyramid(0, which, level_offset=[o[0] + 2] + o[1:])})             # level 0 two bytes off
        bad(name + ": every level", **{name: pyramid(0, which, level_offset=o[:3] + [4 * pyramids[0][which].buf.numel()])})  # level 3 behind the end
        bad(name + ": every level", **{name: pyramid(0, which, level_offset=o[:3] + [1 << 62])})
        bad(name + ": every level", **{name: pyramid(0, which, data=pyramids[0][which].buf[:o[0] // 4 + 12 * 9 - 1])})  # level 0 one texel short
        bad(name + ": two levels overlap", **{name: pyramid(0, which, level_offset=[o[0], o[0] + 4 * (12 * 9 - 1)] + o[2:])})
        bad(name + ": two levels overlap", **{name: pyramid(0, which, level_offset=o[:3] + [o[0]])})
    o1 = pyramids[1][0].offsets
    bad("bloom_downsampled_attachment: every level", fmt=1, bloom_downsampled_attachment=pyramid(1, 0, level_offset=[o1[0] + 4] + o1[1:]))  # 4-byte aligned u16x4
    bad("must not overlap", bloom_upsampled_attachment=pyramid(0, 0))
    bad("must not overlap", bloom_downsampled_attachment=BloomPyramid(sources[0].buf, W // 2, H // 2, 4, offs, 0))
    big = i32(2048)
    bad("must not overlap", bloom_upsampled_attachment=BloomPyramid(big, W // 2, H // 2, 4, [0, 432, 528, 552], 0), final_attachment=big[138:138 + W * H].view(H, W))  # the source's first texel is U's last
    bad("must not overlap", bloom_downsampled_attachment=BloomPyramid(big, W // 2, H // 2, 4, [0, 432, 528, 552], 0),
        bloom_upsampled_attachment=BloomPyramid(big, W // 2, H // 2, 4, [1000, 552, 1600, 1700], 0))  # U's level 1 on D's level 3
    bad("exposure_buffer", exposure_buffer=None)
    bad("exposure_buffer", exposure_buffer=torch.ones(1, dtype=torch.float32, device="cuda"))
    bad("exposure_buffer", exposure_buffer=i32(3).view(torch.int16)[1:])
    for name in ("threshold", "soft_threshold", "clamp_value", "radius"):
        for v in (nan, inf, -inf):
            bad("finite", **{name: v})
    # two broken rules report the first of the list
    bad("at least 2", width=1, source_format=2)
    bad("source_format", source_format=2, final_attachment=None)
    bad("final_attachment", final_attachment=None, bloom_downsampled_attachment=pyramid(0, 0, levels=3))
    bad("bloom_downsampled_attachment", bloom_downsampled_attachment=pyramid(0, 0, levels=3), bloom_upsampled_attachment=pyramid(0, 1, levels=3))
    bad("bloom_upsampled_attachment", bloom_upsampled_attachment=pyramid(0, 1, levels=3), exposure_buffer=None)
    bad("exposure_buffer", exposure_buffer=None, radius=nan)
    lib, raw, stream = renderer._lib, renderer._ctx, renderer._stream(None)
    c = base[0].c()
    c.struct_size = 4
    assert lib.oxc_apply_bloom(raw, c, stream) == L.OXC_INVALID_ARG
    assert lib.oxc_apply_bloom(raw, None, stream) == L.OXC_INVALID_ARG
    untouched()
    # the contexts still run
    for fmt in (0, 1):
        renderer.apply_bloom(base[fmt])
        torch.cuda.synchronize()
        want = BM.apply_bloom(images[fmt], fmt, start, **DEFAULTS)
        pyramids[fmt][0].check(f"after the refusals, format {fmt}: bloom_downsampled", want[0])
        pyramids[fmt][1].check(f"after the refusals, format {fmt}: bloom_upsampled", want[1])
