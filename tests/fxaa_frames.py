"""What the FXAA tests share: the hand-made images of tests/test_fxaa_model.py and tests/test_gpu_fxaa.py (plateaus, step edges, polygons,
the long-search strips, the tie cases, the exact-threshold pixel, the list-size stripes) and the GPU call between guard bands.  Numpy only
until `run_fxaa` is called; the numeric rules come from pixel_rules, the guard bands from gpu_passes."""
import numpy as np

import fxaa_model as XM
from pixel_rules import pack_b10g11r11

F = np.float32
POISON = 0xFFFFFFFF  # NaN in every UF11 / UF10 / binary16 field: one read outside a window shows in the result
DARK, BRIGHT = (0.125, 0.25, 0.0625), (1.0, 0.75, 0.5)  # exact in UF11 / UF10 and binary16


def pack_image(r, g, b, a, fmt) -> np.ndarray:
    r, g, b, a = (np.asarray(c, dtype=np.float32) for c in (r, g, b, a))
    if fmt == 0:
        return pack_b10g11r11(r.reshape(-1), g.reshape(-1), b.reshape(-1)).astype(np.uint32).reshape(r.shape)
    with np.errstate(over="ignore"):
        return np.stack([r, g, b, a], axis=-1).astype(np.float16).view(np.uint16)


def two_colours(mask, fmt, lo=DARK, hi=BRIGHT, alpha=(0.25, 0.75)) -> np.ndarray:
    """`hi` where the mask is set, `lo` elsewhere; with RGBA16F the two alphas likewise."""
    planes = [np.where(mask, h, l).astype(np.float32) for l, h in zip(lo + (alpha[0],), hi + (alpha[1],))]
    return pack_image(*planes, fmt)


def constant_image(W, H, fmt, colour=(0.5, 0.25, 2.0), alpha=0.5) -> np.ndarray:
    return two_colours(np.zeros((H, W), dtype=bool), fmt, lo=colour, alpha=(alpha, alpha))


def step_edge(W, H, fmt, at, vertical=True) -> np.ndarray:
    """Two plateaus: DARK before column (vertical) or row `at`, BRIGHT from it on."""
    ys, xs = np.mgrid[0:H, 0:W]
    return two_colours((xs if vertical else ys) >= at, fmt)


def plateaus(W, H, fmt, seed, count=6) -> np.ndarray:
    """Random rectangles of random colours over a random background: hard edges in both orientations and of both signs."""
    rng = np.random.default_rng(seed)
    planes = [np.full((H, W), v, dtype=np.float32) for v in rng.uniform(0.05, 1.0, 4)]
    for _ in range(count):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        x1, y1 = x0 + int(rng.integers(1, max(2, W // 2 + 1))), y0 + int(rng.integers(1, max(2, H // 2 + 1)))
        for p, v in zip(planes, np.exp2(rng.uniform(-4.0, 2.0, 4))):
            p[y0:y1, x0:x1] = v
    return pack_image(*planes, fmt)


def polygons(W=64, H=48, fmt=0) -> np.ndarray:
    """Hard-edged polygons with distinct plateau colours over a mild gradient: sixteen axis-aligned rectangles with even sides of 4 .. 10
    texels on a 16 x 12 grid, the gradient running through them.  Even, short sides keep the two search distances of a pixel apart (an odd
    side has a middle pixel whose distances tie, and beyond five texels the step table merges neighbouring distances); the gradient keeps
    the corner pixels' horizontal and vertical estimates apart."""
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = xs + 0.5, ys + 0.5
    planes = [(base + sx * px / W + sy * py / H).astype(np.float32) for base, sx, sy in ((0.10, 0.30, 0.12), (0.12, 0.18, 0.36), (0.08, 0.24, 0.18), (0.5, 0.2, 0.1))]
    rng = np.random.default_rng(20)
    for gy in range(4):
        for gx in range(4):
            w, h = 4 + 2 * int(rng.integers(0, 4)), 4 + 2 * int(rng.integers(0, 3))
            x0, y0 = 16 * gx + 2 + int(rng.integers(0, 13 - w)), 12 * gy + 2 + int(rng.integers(0, 9 - h))
            for p, v in zip(planes, np.exp2(rng.uniform(-1.0, 1.5, 4))):
                p[y0:y0 + h, x0:x0 + w] += np.float32(v)
    return pack_image(*planes, fmt)


def long_search(fmt, along_x=True, length=96, across=8, stops=(0, 13, 38, 95)) -> np.ndarray:
    """A one-texel step edge along a `length` x `across` strip, between the rows across / 2 - 1 and across / 2, with terminators: at each
    column of `stops` the whole column is BRIGHT, so the edge ends there.  The edge's three pieces are 12, 24 and 56 texels long, so a pixel at it lies 1 .. 56 texels
    from the terminator on either side: every end step of both sides occurs (the taps lie 1, 2, 3, 4, 5, 6.5, 8.5, 10.5, 12.5, 14.5 and 18.5
    texels out), and the pixels of the long piece more than 18.5 texels from a terminator run all 12 steps without reaching it."""
    ys, xs = np.mgrid[0:across, 0:length]
    mask = (ys >= across // 2) | np.isin(xs, stops)
    return two_colours(mask if along_x else mask.T, fmt)


def isolated_texel(W, H, fmt) -> np.ndarray:
    ys, xs = np.mgrid[0:H, 0:W]
    return two_colours((xs == W // 2) & (ys == H // 2), fmt)


def checkerboard(W, H, fmt) -> np.ndarray:
    ys, xs = np.mgrid[0:H, 0:W]
    return two_colours((xs + ys) % 2 == 1, fmt)


def ridge(W, H, fmt, vertical=True) -> np.ndarray:
    """A one-texel bright line: at its pixels |gradient1| == |gradient2|."""
    ys, xs = np.mgrid[0:H, 0:W]
    return two_colours((xs == W // 2) if vertical else (ys == H // 2), fmt)


def stripe(W, H, fmt, extra=False) -> np.ndarray:
    """A two-texel bright stripe down the columns 4 and 5: the columns 3 .. 6 search, 64 pixels of a 16-row tile; `extra` lights the texel
    (16, 8) of the next tile, whose left neighbour (15, 8) is then the 65th searching pixel of the first."""
    ys, xs = np.mgrid[0:H, 0:W]
    return two_colours((xs == 4) | (xs == 5) | (extra & (xs == 16) & (ys == 8)), fmt)


def searched_per_tile(early) -> list:
    """The number of searching pixels of every 16 x 16 tile, row-major: the lengths of the kernel's per-block lists."""
    H, W = early.shape
    return [int((~early[y:y + 16, x:x + 16]).sum()) for y in range(0, H, 16) for x in range(0, W, 16)]


def texel_lumas(codes, fmt) -> np.ndarray:
    """The luma of each texel of a [n] (B10G11R11) or [n, 4] (RGBA16F) array of codes."""
    r, g, b, _ = XM.decode(codes.reshape((1,) + codes.shape), fmt)
    return XM.luma_of(r, g, b)[0]


def threshold_pair(fmt):
    """Two texels (hi, lo) whose lumas give luma_range == max(0.0312f, luma_max * 0.125f) exactly: a pixel of `lo` among `hi` neighbours
    (or the reverse) sits on the threshold, which the rule's `<` sends into the search.  Found by a search over green and red codes."""
    if fmt == 0:
        g, r = np.meshgrid(np.arange(1 << 6, 31 << 6, dtype=np.uint32), np.arange(0, 31 << 6, 61, dtype=np.uint32))
        codes = (r.reshape(-1) | (g.reshape(-1) << np.uint32(11))).astype(np.uint32)
    else:
        g, r = np.meshgrid(np.arange(0x0400, 0x7C00, dtype=np.uint16), np.arange(0x2C00, 0x4400, 0x155, dtype=np.uint16))
        codes = np.stack([r.reshape(-1), g.reshape(-1), np.zeros(g.size, np.uint16), np.full(g.size, 0x3800, np.uint16)], axis=-1).astype(np.uint16)
    lum = texel_lumas(codes, fmt)
    order = np.argsort(lum, kind="stable")
    lum, codes = lum[order], codes[order]
    threshold = np.fmax(XM.EDGE_THRESHOLD_MIN, lum * XM.EDGE_THRESHOLD_MAX)
    at = np.searchsorted(lum, lum - threshold)
    for k in (0, -1, 1):
        j = np.clip(at + k, 0, lum.size - 1)
        hit = np.flatnonzero((lum - lum[j]).astype(np.float32) == threshold)
        if hit.size:
            return codes[hit[0]], codes[j[hit[0]]]
    raise AssertionError("no texel pair on the threshold")


def on_the_threshold(W, H, fmt) -> np.ndarray:
    """A `hi` image with one `lo` texel in the middle."""
    hi, lo = threshold_pair(fmt)
    image = np.empty((H, W) + hi.shape, dtype=hi.dtype)
    image[...] = hi
    image[H // 2, W // 2] = lo
    return image


# ---- the GPU call -------------------------------------------------------------------------------------------------------------------------------
def run_fxaa(r, image, fmt, label, align_src=None, align_dst=None, counters=True):
    """One oxc_apply_fxaa with the source and the destination between poisoned guard bands (gpu_passes.Guard): every output word equal to the
    checker's, both bands of both images untouched, the source unchanged and, with `counters`, every counter equal to the checker's counts.
    Returns (the checker's image, its counters, its detail)."""
    import torch

    from gpu_passes import Guard, same
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import FxaaContext

    image = np.ascontiguousarray(image)
    H, W = image.shape[:2]
    texel, dtype, fill = (8, torch.int16, 0xFFFB) if fmt else (4, torch.int32, 0xFFFFFFFB)
    poison = POISON & (0xFFFF if fmt else 0xFFFFFFFF)
    src = Guard("final_attachment", image.shape, dtype, W * (4 if fmt else 1), poison, align_src or texel, data=image)
    dst = Guard("fxaa_attachment", image.shape, dtype, W * (4 if fmt else 1), poison, align_dst or texel, fill=fill)
    detail = {}
    want, stats = XM.apply_fxaa(image, fmt, detail)
    ctx = FxaaContext(src.tensor, dst.tensor, W, H, fmt)
    if counters:
        r.debug_set_tuning(L.TUNE_FXAA_STATS, 1)
    try:
        out = r.apply_fxaa(ctx)
        torch.cuda.synchronize()
        if counters:
            got_stats = r.debug_fxaa_stats()
    finally:
        if counters:
            r.debug_set_tuning(L.TUNE_FXAA_STATS, 0)
    assert out is dst.tensor
    dst.check(f"{label}: dst", want)
    src.check(f"{label}: src")
    same(dst.bits()[1].reshape(want.shape), want, f"{label}: fxaa_attachment")
    same(src.bits()[1].reshape(image.shape), image.view(want.dtype), f"{label}: final_attachment")
    if counters:
        assert list(got_stats.values()) == stats, f"{label}: counters {got_stats} != {stats}"
    return want, stats, detail
