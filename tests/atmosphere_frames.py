"""What the atmosphere tests share: the Atmosphere records, the rule that makes the 64 hemisphere directions, the cameras and suns, the
checker's LUTs (computed once per record and kept) and the GPU calls between guard bands.  Numpy only until a `run_*` helper is called; the
numeric rules come from pixel_rules and atmosphere_model, the guard bands from gpu_passes."""
import dataclasses
import math

import numpy as np

import atmosphere_model as AM

F = np.float32
POISON, FILL = 0xFFFF, 0xFFFB  # NaN halves: one read outside a window shows in the result; no pass writes 0xFFFB (a NaN is stored as 0x7E00)
SUN_INTENSITY = 10.0


# ---- records ------------------------------------------------------------------------------------------------------------------------------------
def engine_atmosphere(**overrides) -> AM.Atmosphere:
    """What RendererInstance.cpp:1445-1455 makes of the AtmosphereComponent defaults: the coefficients scaled by 1e-3 in binary32; the engine's
    four extents."""
    s = lambda v: tuple(float(F(x) * F(1e-3)) for x in v)  # noqa: E731
    a = AM.Atmosphere(rayleigh_scatter=s((5.802, 13.558, 33.100)), mie_scatter=s((3.996, 3.996, 3.996)), mie_extinction=s((4.44,))[0],
                      ozone_absorption=s((0.650, 1.881, 0.085)))
    return dataclasses.replace(a, **overrides)


def small_atmosphere(transmittance=(17, 9), multiscatter=(5, 3), sky_view=(17, 9), aerial=(5, 3, 2), **overrides) -> AM.Atmosphere:
    """The engine's record at small extents."""
    return engine_atmosphere(transmittance_lut_size=tuple(transmittance) + (1,), multiscattering_lut_size=tuple(multiscatter) + (1,),
                             sky_view_lut_size=tuple(sky_view) + (1,), aerial_perspective_lut_size=tuple(aerial), **overrides)


def hemisphere() -> np.ndarray:
    """The tests' 64 unit directions: a spherical Fibonacci set over the whole sphere, z = 1 - (2 i + 1) / 64, longitude 2 pi i / golden ratio,
    evaluated in binary64 and rounded to binary32.  float32 [64, 3]."""
    i = np.arange(64, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / 64.0
    lon = 2.0 * math.pi * i / ((1.0 + math.sqrt(5.0)) / 2.0)
    rad = np.sqrt(1.0 - z * z)
    return np.stack([rad * np.cos(lon), z, rad * np.sin(lon)], axis=-1).astype(np.float32)


# ---- cameras and suns ---------------------------------------------------------------------------------------------------------------------------
def camera(y_metres: float, look=(0.0, 0.0, -1.0), fov_y=60.0, aspect=1.0, near=0.1, far=2000.0):
    """(position, inverse projection-view, column-major float32 [16]) of a perspective camera at (3, y, -2) looking along `look`, built in
    binary64 and rounded once."""
    eye = np.array([3.0, y_metres, -2.0])
    f = np.array(look, dtype=np.float64)
    f /= np.linalg.norm(f)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.99 else np.array([0.0, 0.0, 1.0])
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -view[:3, :3] @ eye
    t = 1.0 / math.tan(math.radians(fov_y) / 2.0)
    proj = np.array([[t / aspect, 0, 0, 0], [0, -t, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]])
    inv = np.linalg.inv(proj @ view)
    return tuple(float(F(v)) for v in eye), inv.T.reshape(16).astype(np.float32)  # column-major: element (r, c) at c * 4 + r


CAMERAS = {
    "ground": camera(0.0, look=(0.3, 0.1, -1.0)),
    "below ground": camera(-500.0, look=(0.0, 0.2, -1.0)),
    "50 km": camera(5000.0, look=(0.2, -0.3, -1.0)),  # eye altitude = y * 0.01 km above min_altitude
    "100.5 km down": camera(10050.0, look=(0.05, -1.0, 0.02), fov_y=40.0),  # just above the atmosphere: aerial texels move to its top and go on
    "150 km down": camera(15000.0, look=(0.05, -1.0, 0.02), fov_y=40.0),
    "150 km away": camera(15000.0, look=(0.0, 1.0, 0.05), fov_y=40.0),
    "150 km limb": camera(15000.0, look=(0.0, -0.13, -1.0), fov_y=60.0),  # part of the frame hits the atmosphere, part misses
}


def sun(elevation_deg: float, azimuth_deg: float = 20.0, scale: float = 1.0):
    e, a = math.radians(elevation_deg), math.radians(azimuth_deg)
    return tuple(float(F(scale * v)) for v in (math.cos(e) * math.cos(a), math.sin(e), math.cos(e) * math.sin(a)))


SUNS = {"30 deg": sun(30.0), "zenith": (0.0, 1.0, 0.0), "horizon": sun(0.0), "below": sun(-12.0), "not normalised": sun(40.0, 70.0, 2.5)}


# ---- the checker's LUTs, kept ---------------------------------------------------------------------------------------------------------------------
_kept = {}


def _key(A, names):
    return tuple(repr(getattr(A, n)) for n in names)


_MEDIUM = ("rayleigh_scatter", "rayleigh_density", "mie_scatter", "mie_density", "mie_extinction", "mie_asymmetry", "ozone_absorption", "ozone_height",
           "ozone_thickness", "terrain_albedo", "planet_radius", "atmos_radius")


def want_transmittance(A) -> np.ndarray:
    k = ("t",) + _key(A, _MEDIUM + ("transmittance_lut_size",))
    if k not in _kept:
        _kept[k] = AM.transmittance_lut(A)
        _kept[k].setflags(write=False)
    return _kept[k]


def want_multiscatter(A, directions=None, counts=None) -> np.ndarray:
    directions = hemisphere() if directions is None else directions
    k = ("m", directions.tobytes()) + _key(A, _MEDIUM + ("transmittance_lut_size", "multiscattering_lut_size"))
    if k not in _kept or counts is not None:
        _kept[k] = AM.multiscatter_lut(A, want_transmittance(A), directions, counts)
        _kept[k].setflags(write=False)
    return _kept[k]


def want_draw(A, cam, sun_dir, sun_intensity=SUN_INTENSITY, counts=None):
    """(sky_view_lut, sky_aerial_perspective_lut) of the checker, from the checker's own transmittance LUT."""
    position, inv = cam
    t = want_transmittance(A)
    return (AM.sky_view_lut(A, t, position, sun_dir, sun_intensity, counts), AM.aerial_lut(A, t, position, inv, sun_dir, sun_intensity, counts))


# ---- the GPU calls ------------------------------------------------------------------------------------------------------------------------------
def renderer_atmosphere(A):
    from oxylus_amd.renderer import Atmosphere

    return Atmosphere(**dataclasses.asdict(A))


def _guard(name, shape, data=None, align=8):
    import torch

    from gpu_passes import Guard

    return Guard(name, tuple(shape) + (4,), torch.int16, shape[-1] * 4, POISON, align, data=data, fill=None if data is not None else FILL)


def lut_guards(A, transmittance=None, multiscatter=None):
    """The four LUTs between guard bands: the first two hold the given bits (inputs) or the pre-fill (outputs)."""
    t, m, v, a = A.transmittance_lut_size, A.multiscattering_lut_size, A.sky_view_lut_size, A.aerial_perspective_lut_size
    return (_guard("sky_transmittance_lut", (t[1], t[0]), transmittance), _guard("sky_multiscatter_lut", (m[1], m[0]), multiscatter),
            _guard("sky_view_lut", (v[1], v[0])), _guard("sky_aerial_perspective_lut", (a[2], a[1], a[0])))


def run_sky_luts(r, A, label, directions=None):
    """One oxc_generate_sky_luts between guard bands: every word of both LUTs equal to the checker's, the bands and the table untouched."""
    import torch

    from gpu_passes import Guard, same
    from oxylus_amd.renderer import SkyLutContext

    directions = hemisphere() if directions is None else directions
    table = Guard("hemisphere_directions", (64, 3), torch.float32, 3, 0xFFFFFFFF, 8, data=directions)
    t, m, _, _ = lut_guards(A)
    r.generate_sky_luts(SkyLutContext(renderer_atmosphere(A), table.tensor, t.tensor, m.tensor))
    torch.cuda.synchronize()
    want_t, want_m = want_transmittance(A), want_multiscatter(A, directions)
    t.check(f"{label}: transmittance", want_t)
    m.check(f"{label}: multiscatter", want_m)
    table.check(f"{label}: table")
    same(t.bits()[1].reshape(want_t.shape), want_t, f"{label}: sky_transmittance_lut")
    same(m.bits()[1].reshape(want_m.shape), want_m, f"{label}: sky_multiscatter_lut")
    same(table.bits()[1], directions.view(np.uint32).reshape(-1), f"{label}: hemisphere_directions")
    return want_t, want_m


def draw_context(A, guards, cam, sun_dir, sun_intensity=SUN_INTENSITY):
    from oxylus_amd.renderer import AtmosphereContext

    t, m, v, a = guards
    position, inv = cam
    return AtmosphereContext(renderer_atmosphere(A), t.tensor, m.tensor, v.tensor, a.tensor, tuple(sun_dir), float(sun_intensity), tuple(position),
                             tuple(float(x) for x in inv))


def run_draw(r, A, cam, sun_dir, label, sun_intensity=SUN_INTENSITY, counts=None):
    """One oxc_draw_atmosphere on the checker's transmittance and multiscatter LUTs, between guard bands: every word of both outputs equal to
    the checker's, every band and both inputs untouched."""
    import torch

    from gpu_passes import same

    want_t, want_m = want_transmittance(A), want_multiscatter(A)
    guards = lut_guards(A, want_t, want_m)
    r.draw_atmosphere(draw_context(A, guards, cam, sun_dir, sun_intensity))
    torch.cuda.synchronize()
    want_v, want_a = want_draw(A, cam, sun_dir, sun_intensity, counts)
    for g, want, name in zip(guards, (None, None, want_v, want_a), ("transmittance", "multiscatter", "sky view", "aerial")):
        g.check(f"{label}: {name}", want)
    same(guards[0].bits()[1].reshape(want_t.shape), want_t, f"{label}: sky_transmittance_lut (input)")
    same(guards[1].bits()[1].reshape(want_m.shape), want_m, f"{label}: sky_multiscatter_lut (input)")
    same(guards[2].bits()[1].reshape(want_v.shape), want_v, f"{label}: sky_view_lut")
    same(guards[3].bits()[1].reshape(want_a.shape), want_a, f"{label}: sky_aerial_perspective_lut")
    return want_v, want_a
