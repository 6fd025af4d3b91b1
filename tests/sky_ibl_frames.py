"""What the sky-cubemap tests share: the LUT contents (the LUT checker's for the realistic frames, random halves with hand-placed NaN / Inf /
HALF_MAX texels for the small ones), the history patterns, the cameras and suns, and one GPU call between guard bands.  Numpy only until
`run` is called; the rules come from sky_ibl_model, the LUTs from atmosphere_frames / atmosphere_model, the guard bands from gpu_passes."""
import numpy as np

import atmosphere_frames as AF
import atmosphere_model as AM
import sky_ibl_model as SM
from pixel_rules import to_half_bits

F = np.float32
POISON, FILL = AF.POISON, AF.FILL
STRENGTH = 0.15
CAMERAS = {"ground": (3.0, 0.0, -2.0), "below ground": (3.0, -500.0, -2.0), "50 km": (3.0, 5000.0, -2.0), "above the atmosphere": (3.0, 15000.0, -2.0)}
SUNS = dict(AF.SUNS, zero=(0.0, 0.0, 0.0))
HALF_NAN, HALF_INF, HALF_NEG_INF, HALF_MAX_BITS, HALF_ONE, HALF_NEG_ZERO, HALF_DENORMAL = 0x7E00, 0x7C00, 0xFC00, 0x7BFF, 0x3C00, 0x8000, 0x0001

_kept = {}


def atmosphere(sky_view=(17, 9), transmittance=(17, 9)):
    """The engine's record with these two LUT extents (the call reads no other extent)."""
    return AF.small_atmosphere(sky_view=sky_view, transmittance=transmittance)


def realistic_luts(A, camera="ground", sun="30 deg", sun_intensity=AF.SUN_INTENSITY):
    """(sky_view_lut, sky_transmittance_lut) of the LUT checker for this record, camera and sun; computed once and kept, read-only."""
    key = (repr(A), camera, sun, float(sun_intensity))
    if key not in _kept:
        t = AF.want_transmittance(A)
        v = AM.sky_view_lut(A, t, CAMERAS[camera], SUNS[sun], sun_intensity)
        v.setflags(write=False)
        _kept[key] = (v, t)
    return _kept[key]


def random_lut(width, height, seed, alpha_scale=4.0, special=True) -> np.ndarray:
    """uint16 [height, width, 4]: random finite halves (colours in [-0.25, 1), alpha in [0, alpha_scale)), and with `special` one texel each of
    a NaN colour, an Inf alpha, a -Inf colour and HALF_MAX in every channel, at fixed places."""
    rng = np.random.default_rng(seed)
    values = rng.random((height, width, 4), dtype=np.float32) * F(1.25) - F(0.25)
    values[..., 3] = rng.random((height, width), dtype=np.float32) * F(alpha_scale)
    lut = to_half_bits(values).astype(np.uint16)
    if special:
        flat = lut.reshape(-1, 4)
        n = flat.shape[0]
        flat[0 % n, 1] = HALF_NAN
        flat[(n // 3) % n, 3] = HALF_INF
        flat[(n // 2) % n, 2] = HALF_NEG_INF
        flat[n - 1] = HALF_MAX_BITS
    return lut


def history_patterns(cube_size: int, seed: int = 5) -> np.ndarray:
    """A cube whose texels run through the history cases in turn: zero, alpha 0 with finite colours, a negative alpha, -0.0, a NaN alpha, a
    positive denormal alpha, alpha 1 with a NaN / Inf / -Inf in exactly one colour channel, colours at HALF_MAX, and an ordinary history."""
    rng = np.random.default_rng(seed)
    n = 6 * cube_size * cube_size
    cube = to_half_bits(rng.random((n, 4), dtype=np.float32) * F(2.0)).astype(np.uint16)
    cube[:, 3] = HALF_ONE
    kind = np.arange(n) % 11
    cube[kind == 0] = 0
    cube[kind == 1, 3] = 0
    cube[kind == 2, 3] = 0xBC00  # -1.0
    cube[kind == 3, 3] = HALF_NEG_ZERO
    cube[kind == 4, 3] = HALF_NAN
    cube[kind == 5, 3] = HALF_DENORMAL
    cube[kind == 6, 0] = HALF_NAN
    cube[kind == 7, 1] = HALF_INF
    cube[kind == 8, 2] = HALF_NEG_INF
    cube[kind == 9, :3] = HALF_MAX_BITS
    return cube.reshape(6, cube_size, cube_size, 4)


def want(A, view, transmittance, cube, camera_position, sun_dir, sun_intensity=AF.SUN_INTENSITY, strength=STRENGTH, frame_index=0, counts=None):
    return SM.sky_ibl(A.planet_radius, A.atmos_radius, view, transmittance, cube, camera_position, sun_dir, sun_intensity, strength, frame_index, counts)


def guard(name, data):
    """`data` (uint16 [..., W, 4]) between guard bands of at least one row."""
    import torch

    from gpu_passes import Guard

    return Guard(name, data.shape, torch.int16, data.shape[-2] * 4, POISON, 8, data=data)


def guards(view, transmittance, cube):
    return guard("sky_view_lut", view), guard("sky_transmittance_lut", transmittance), guard("sky_cubemap", cube)


def context(A, gs, camera_position, sun_dir, sun_intensity=AF.SUN_INTENSITY, strength=STRENGTH, frame_index=0):
    from oxylus_amd.renderer import SkyIblContext

    v, t, c = gs
    return SkyIblContext(AF.renderer_atmosphere(A), v.tensor, t.tensor, c.tensor, int(c.tensor.shape[1]), tuple(sun_dir), float(sun_intensity),
                         tuple(camera_position), float(strength), int(frame_index))


def run(r, A, view, transmittance, cube, camera_position, sun_dir, label, sun_intensity=AF.SUN_INTENSITY, strength=STRENGTH, frame_index=0, counts=None):
    """One oxc_generate_sky_ibl between guard bands: every word of the cube equal to the checker's, the bands and both LUTs untouched.
    Returns the cube after the call."""
    import torch

    from gpu_passes import same

    gs = guards(view, transmittance, cube)
    r.generate_sky_ibl(context(A, gs, camera_position, sun_dir, sun_intensity, strength, frame_index))
    torch.cuda.synchronize()
    expected = want(A, view, transmittance, cube, camera_position, sun_dir, sun_intensity, strength, frame_index, counts)
    for g in gs:
        g.check(label)
    same(gs[0].bits()[1].reshape(view.shape), view, f"{label}: sky_view_lut (input)")
    same(gs[1].bits()[1].reshape(transmittance.shape), transmittance, f"{label}: sky_transmittance_lut (input)")
    got = gs[2].bits()[1].reshape(expected.shape)
    same(got, expected, f"{label}: sky_cubemap")
    return got
