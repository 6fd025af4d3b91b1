"""The numpy checker of oxc_apply_bloom: the geometry, the manual bilinear and steps 1-5 of its header block in include/oxcull.h, vectorised
over a level.  Every binary32 operation is one numpy float32 operation in the order the header states.  A level is uint32 [h, w]
(B10G11R11) or uint16 [h, w, 4] (R16G16B16A16 Sfloat); a decoded level is three float32 planes [h, w]."""
from __future__ import annotations

import numpy as np

from pixel_rules import channel_half, cvt_i32_sat, f32a, from_half_bits, lerp, pack_b10g11r11, unpack_b10g11r11
from pixel_rules import pack_ufloat  # noqa: F401  (the pack the B10G11R11 store goes through; the tests name it)

F = np.float32
FORMAT_B10G11R11, FORMAT_R16G16B16A16 = 0, 1
BORDER, CLAMP = 0, 1
HALF_ONE = 0x3C00
# bloom_prefilter.slang:51-63 and bloom_downsample.slang:21-33
TAPS13 = dict(a=(-2, 2), b=(0, 2), c=(2, 2), d=(-2, 0), e=(0, 0), f=(2, 0), g=(-2, -2), h=(0, -2), i=(2, -2), j=(-1, 1), k=(1, 1), l=(-1, -1), m=(1, -1))
# bloom_upsample.slang:31-39
TAPS9 = dict(a=(-1, 1), b=(0, 1), c=(1, 1), d=(-1, 0), e=(0, 0), f=(1, 0), g=(-1, -1), h=(0, -1), i=(1, -1))


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------
def geometry(W: int, H: int):
    """(w2, h2, L, [(w, h) of every level])."""
    w2, h2 = W // 2, H // 2
    L = max(w2, h2).bit_length()  # floor(log2(m)) + 1 in integers
    return w2, h2, L, [(max(1, w2 >> k), max(1, h2 >> k)) for k in range(L)]


# ---- formats (step 5) ----------------------------------------------------------------------------------------------------------------------------
def decode(level, fmt: int):
    level = np.ascontiguousarray(level)
    if fmt == FORMAT_B10G11R11:
        w = level.view(np.uint32)
        return tuple(c.reshape(w.shape) for c in unpack_b10g11r11(w.reshape(-1)))
    halves = level.view(np.uint16)
    return tuple(from_half_bits(halves[..., c]) for c in range(3))


def encode(rgb, fmt: int) -> np.ndarray:
    r, g, b = (f32a(c) for c in rgb)
    if fmt == FORMAT_B10G11R11:
        return pack_b10g11r11(r.reshape(-1), g.reshape(-1), b.reshape(-1)).astype(np.uint32).reshape(r.shape)
    return np.stack([channel_half(r), channel_half(g), channel_half(b), np.full(r.shape, HALF_ONE, dtype=np.uint16)], axis=-1).astype(np.uint16)


# ---- the manual bilinear -------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def axis_tap(n_out: int, n_src: int, k: int):
    """One axis of a tap for every output coordinate: (i int64 [n_out], f float32 [n_out])."""
    x = np.arange(n_out, dtype=np.float32)
    uv = (x + F(0.5)) / F(n_out)
    ts = F(1.0) / F(n_out)
    p = uv + F(ts * F(k))
    g = (p * F(n_src) - F(0.5)).astype(np.float32)
    i = np.floor(g)
    return cvt_i32_sat(i).astype(np.int64), (g - i).astype(np.float32)


def fetch(plane, yy, xx, mode: int) -> np.ndarray:
    """The texels (yy[r], xx[c]) of one plane under an address mode."""
    sh, sw = plane.shape
    t = plane[np.clip(yy, 0, sh - 1)[:, None], np.clip(xx, 0, sw - 1)[None, :]]
    if mode == CLAMP:
        return t
    inside = ((yy >= 0) & (yy <= sh - 1))[:, None] & ((xx >= 0) & (xx <= sw - 1))[None, :]
    return np.where(inside, t, F(0.0)).astype(np.float32)


def bilinear(rgb, ow: int, oh: int, kx: int, ky: int, mode: int):
    """The tap (kx, ky) of an ow x oh output on a decoded level: three planes [oh, ow]."""
    sh, sw = rgb[0].shape
    ix, fx = axis_tap(ow, sw, kx)
    iy, fy = axis_tap(oh, sh, ky)
    fx, fy = fx[None, :], fy[:, None]
    out = []
    for plane in rgb:
        top = lerp(fetch(plane, iy, ix, mode), fetch(plane, iy, ix + 1, mode), fx)
        bottom = lerp(fetch(plane, iy + 1, ix, mode), fetch(plane, iy + 1, ix + 1, mode), fx)
        out.append(lerp(top, bottom, fy))
    return tuple(out)


def taps(rgb, ow, oh, table, mode):
    return {name: bilinear(rgb, ow, oh, kx, ky, mode) for name, (kx, ky) in table.items()}


@np.errstate(all="ignore")
def sum4(t, names):
    a, b, c, d = (t[n] for n in names)
    return tuple(((a[ch] + b[ch]) + c[ch]) + d[ch] for ch in range(3))


# ---- the steps -----------------------------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def prefilter_curve(group, threshold, soft_threshold):
    """prefilter() of bloom_prefilter.slang:29-39 on three planes."""
    r, g, b = group
    threshold = F(threshold)
    brightness = np.fmax(r, np.fmax(g, b))
    knee = F(threshold * F(soft_threshold))
    soft = np.fmin(np.fmax((brightness - threshold) + knee, F(0.0)), F(F(2.0) * knee))
    soft = ((soft * soft) * F(0.25)) / F(knee + F(1.0e-5))
    contribution = np.fmax(soft, brightness - threshold) / np.fmax(brightness, F(1.0e-5))
    return tuple((c * contribution).astype(np.float32) for c in group)


@np.errstate(all="ignore")
def prefilter(image, fmt: int, exposure, threshold, soft_threshold, clamp_value):
    """Step 2: D level 0 (encoded) of a W x H image.  `exposure` is the binary32 the groups are multiplied by."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    ow, oh = W // 2, H // 2
    t = taps(decode(image, fmt), ow, oh, TAPS13, BORDER)
    exposure, clamp_value = F(exposure), F(clamp_value)
    color_sum = [np.zeros((oh, ow), dtype=np.float32) for _ in range(3)]
    weight_sum = np.zeros((oh, ow), dtype=np.float32)
    for names in ("abde", "bcef", "degh", "efhi", "jklm"):
        group = tuple(np.fmin((c * F(0.25)) * exposure, clamp_value) for c in sum4(t, names))
        r, g, b = group
        weight = F(1.0) / (F(1.0) + ((r * F(0.299) + g * F(0.587)) + b * F(0.114)))
        curve = prefilter_curve(group, threshold, soft_threshold)
        color_sum = [color_sum[ch] + curve[ch] * weight for ch in range(3)]
        weight_sum = weight_sum + weight
    denominator = weight_sum + F(1.0e-5)
    return encode([c / denominator for c in color_sum], fmt)


@np.errstate(all="ignore")
def downsample(level, fmt: int, ow: int, oh: int):
    """Step 3: D level k (encoded, ow x oh) from D level k - 1 (encoded)."""
    t = taps(decode(level, fmt), ow, oh, TAPS13, BORDER)
    corners, edges, inner = sum4(t, "acgi"), sum4(t, "bdfh"), sum4(t, "ejkl")
    return encode([(corners[ch] * F(0.03125) + edges[ch] * F(0.0625)) + (inner[ch] + t["m"][ch]) * F(0.125) for ch in range(3)], fmt)


@np.errstate(all="ignore")
def upsample(source, down, fmt: int, radius):
    """Step 4: U level k - 1 (encoded) from the 9-tap source (U level k, or D level L - 1) and D level k - 1, both encoded."""
    down = np.asarray(down)
    oh, ow = down.shape[:2]
    t = taps(decode(source, fmt), ow, oh, TAPS9, CLAMP)
    edges, corners = sum4(t, "bdfh"), sum4(t, "acgi")
    source_color = decode(down, fmt)
    radius = F(radius)
    return encode([lerp(source_color[ch], (t["e"][ch] * F(0.25) + edges[ch] * F(0.125)) + corners[ch] * F(0.0625), radius) for ch in range(3)], fmt)


def exposure_of(exposure_words) -> np.float32:
    """The exposure the prefilter multiplies by: the second word of the buffer, or 1.0 without the flag (None)."""
    if exposure_words is None:
        return F(1.0)
    return np.asarray(exposure_words, dtype=np.uint32).view(np.float32)[1]


def apply_bloom(image, fmt: int, exposure_words=None, threshold=1.0, soft_threshold=0.125, clamp_value=4.0, radius=0.75):
    """The whole call: (D, U), each a list of L encoded levels.  `exposure_words`: the exposure buffer's two uint32 with
    HasEyeAdaptation, None without."""
    image = np.asarray(image)
    _, _, L, extents = geometry(image.shape[1], image.shape[0])
    D = [prefilter(image, fmt, exposure_of(exposure_words), threshold, soft_threshold, clamp_value)]
    for k in range(1, L):
        D.append(downsample(D[k - 1], fmt, *extents[k]))
    U = [None] * L
    zero = np.zeros((1, 1), dtype=np.float32)
    U[L - 1] = encode([zero, zero, zero], fmt)  # step 1
    for k in range(L - 1, 0, -1):
        U[k - 1] = upsample(D[L - 1] if k == L - 1 else U[k], D[k - 1], fmt, radius)
    return D, U
