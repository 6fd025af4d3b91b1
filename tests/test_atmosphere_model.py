"""tests/atmosphere_model.py, the checker of oxc_generate_sky_luts and oxc_draw_atmosphere, on the CPU: the library's exports and struct sizes,
the one exp rule, a comparison with a second, scalar transcription of the four Slang passes (written from the Slang, run in binary64 and in
binary32), physical sanity, and the branch classes the GPU test relies on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import atmosphere_frames as AF
import atmosphere_model as AM
import tonemap_model as TM
from pixel_rules import from_half_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- exports ------------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_struct_sizes():
    """Both symbols are exported and the ctypes structs have the header's sizes (computed from the header's own field lists)."""
    from oxylus_amd import lib as L

    lib = L.load()
    for name in ("oxc_generate_sky_luts", "oxc_draw_atmosphere"):
        assert name in L.EXPORTS and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "oxcull.h")) as f:
        header = f.read()

    def words(struct):  # 4-byte words of a typedef whose members are float / uint32_t (arrays too), oxc_atmosphere and oxc_buffer
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        total = 0
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            kind, names = decl.split(None, 1)
            each = {"float": 1, "uint32_t": 1, "oxc_buffer": 4, "oxc_atmosphere": 34}[kind]
            for n in names.split(","):
                dims = re.findall(r"\[(\d+)\]", n)
                total += each * (int(dims[0]) if dims else 1)
        return total

    assert words("oxc_atmosphere") == 34 and C.sizeof(L.Atmosphere) == 136
    assert C.sizeof(L.SkyLutContext) == 4 * words("oxc_sky_lut_context")
    assert C.sizeof(L.AtmosphereContext) == 4 * words("oxc_atmosphere_context")


def test_one_exp_rule():
    x = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 88.0, -88.0, 88.72, 89.0, -87.4, -104.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, 3.62489], dtype=np.float32)
    x = np.concatenate([x, np.linspace(-90.0, 90.0, 4001).astype(np.float32)])
    a, b = AM.exp_rule(x), TM.exp_rule(x)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c, d = AM.cos_turn_rule(x), TM.cos_turn_rule(x)
    assert np.array_equal(c.view(np.uint32), d.view(np.uint32))


# ---- a scalar transcription of the Slang, in the number type T ------------------------------------------------------------------------------------
class Transcription:
    """sky.slang and the four passes statement by statement on numpy scalars of type T (float64 or float32) with numpy's own exp, pow, cos and
    acos; LUTs are stored as binary16 and sampled with a clamp-mode bilinear, as the images are."""

    def __init__(self, A, T):
        self.T, self.A = T, A
        for name in ("rayleigh_density", "mie_density", "mie_extinction", "mie_asymmetry", "ozone_height", "ozone_thickness", "planet_radius", "atmos_radius"):
            setattr(self, name, T(np.float32(getattr(A, name))))
        for name in ("rayleigh_scatter", "mie_scatter", "ozone_absorption", "terrain_albedo"):
            setattr(self, name, np.array([np.float32(v) for v in getattr(A, name)], dtype=T))
        self.PI = T(math.pi)

    def v(self, *c):
        return np.array(c, dtype=self.T)

    def nearest(self, o, d, radius):
        T = self.T
        a, b, c = d @ d, T(2) * (d @ o), o @ o - radius * radius
        delta = b * b - T(4) * a * c
        if delta < 0:
            return None
        s0, s1 = (-b - np.sqrt(delta)) / (T(2) * a), (-b + np.sqrt(delta)) / (T(2) * a)
        if s0 < 0 and s1 < 0:
            return None
        if s0 < 0:
            return max(T(0), s1)
        if s1 < 0:
            return max(T(0), s0)
        return max(T(0), min(s0, s1))

    def medium(self, altitude):
        T = self.T
        rd, md = np.exp(-altitude / self.rayleigh_density), np.exp(-altitude / self.mie_density)
        od = max(T(0), T(1) - abs(altitude - self.ozone_height) / self.ozone_thickness)
        rayleigh, mie = self.rayleigh_scatter * rd, self.mie_scatter * md
        return rayleigh, mie, rayleigh + mie, rayleigh + self.mie_extinction * md + self.ozone_absorption * od

    def sample(self, lut, u, v):
        T = self.T
        H, W = lut.shape[:2]
        gx, gy = u * T(W) - T(0.5), v * T(H) - T(0.5)
        ix, iy = int(math.floor(gx)), int(math.floor(gy))
        fx, fy = gx - T(ix), gy - T(iy)
        cl = lambda i, n: min(max(i, 0), n - 1)  # noqa: E731
        t = lambda x, y: lut[cl(y, H), cl(x, W), :3].astype(T)  # noqa: E731
        top = t(ix, iy) + (t(ix + 1, iy) - t(ix, iy)) * fx
        bottom = t(ix, iy + 1) + (t(ix + 1, iy + 1) - t(ix, iy + 1)) * fx
        return top + (bottom - top) * fy

    def transmittance_uv(self, h, mu):
        T, ar, pr = self.T, self.atmos_radius, self.planet_radius
        H = np.sqrt(max(T(0), ar * ar - pr * pr))
        rho = np.sqrt(max(T(0), h * h - pr * pr))
        d = max(T(0), -h * mu + np.sqrt(max(T(0), h * h * (mu * mu - T(1)) + ar * ar)))
        d_min, d_max = ar - h, rho + H
        return (d - d_min) / (d_max - d_min), rho / H

    def draine(self, alpha, g, c):
        T = self.T
        return (T(1) / (T(4) * self.PI)) * ((T(1) - g * g) / np.power(T(1) + g * g - T(2) * g * c, T(1.5))) * ((T(1) + alpha * c * c) / (T(1) + alpha * (T(1) / T(3)) * (T(1) + T(2) * g * g)))

    def integrate(self, lut, eye, d, sun, sun_intensity, step_count, t_max=None, planet=False):
        T, pr = self.T, self.planet_radius
        lum, as1, tr = self.v(0, 0, 0), self.v(0, 0, 0), self.v(1, 1, 1)
        if eye @ eye <= pr * pr:
            return lum, as1, tr
        hit = self.nearest(eye, d, pr)
        if t_max is None:
            top = self.nearest(eye, d, self.atmos_radius)
            if top is None:
                return lum, as1, tr
            span = top if hit is None else max(T(0), hit)
        else:
            span = t_max
        c = sun @ d
        rayleigh_phase = T(3) / (T(16) * self.PI) * (T(1) + c * c)
        g = self.mie_asymmetry
        g_hg = np.exp(-(T(0.0990567) / (g - T(1.67154))))
        g_d = np.exp(-(T(2.20679) / (g + T(3.91029))) - T(0.428934))
        alpha = np.exp(T(3.62489) - (T(8.29288) / (g + T(5.52825))))
        w_d = np.exp(-(T(0.599085) / (g - T(0.641583))) - T(0.665888))
        a, b = self.draine(T(0), g_hg, c), self.draine(alpha, g_d, c)
        mie_phase = a + (b - a) * w_d
        old, step = T(0), T(0)
        while step < step_count:
            shift = span * (step + T(0.3)) / step_count
            step_length, old = shift - old, shift
            pos = eye + shift * d
            h = np.sqrt(pos @ pos)
            rayleigh, mie, scattering, extinction = self.medium(h - pr)
            up = pos / h
            t_sun = self.sample(lut, *self.transmittance_uv(h, sun @ up))
            shadow = T(0) if self.nearest(pos - T(0.001) * up, sun, pr) is not None else T(1)
            sun_luminance = shadow * t_sun * (mie * mie_phase + rayleigh * rayleigh_phase)
            t = np.exp(-step_length * extinction)
            lum = lum + sun_intensity * ((sun_luminance - sun_luminance * t) / extinction * tr)
            as1 = as1 + (scattering - scattering * t) / extinction * tr
            tr = tr * t
            step += T(1)
        if planet and hit is not None and span == hit:
            pos = eye + span * d
            h = np.sqrt(pos @ pos)
            up = pos / h
            nol = min(max((sun / np.sqrt(sun @ sun)) @ (up / np.sqrt(up @ up)), T(0)), T(1))
            t_sun = self.sample(lut, *self.transmittance_uv(h, sun @ up))
            lum = lum + sun_intensity * (t_sun * tr * nol * self.terrain_albedo / self.PI)
        return lum, as1, tr

    @staticmethod
    def store(rows):
        with np.errstate(over="ignore"):
            return np.array(rows, dtype=np.float64).astype(np.float32).astype(np.float16)

    def transmittance(self):
        T, ar, pr = self.T, self.atmos_radius, self.planet_radius
        W, Hh = self.A.transmittance_lut_size[:2]
        H = np.sqrt(max(T(0), ar * ar - pr * pr))
        out = np.zeros((Hh, W, 4))
        for y in range(Hh):
            for x in range(W):
                u, v = (T(x) + T(0.5)) / T(W), (T(y) + T(0.5)) / T(Hh)
                rho = H * v
                lut_x = np.sqrt(rho * rho + pr * pr)
                d_min, d_max = ar - lut_x, rho + H
                d = d_min + u * (d_max - d_min)
                lut_y = T(1) if d == 0 else (H * H - rho * rho - d * d) / (T(2) * lut_x * d)
                lut_y = min(max(lut_y, T(-1)), T(1))
                sun, pos = self.v(0, np.sqrt(T(1) - lut_y * lut_y), lut_y), self.v(0, 0, lut_x)
                per_step = self.nearest(pos, sun, ar) / T(1000)
                depth = self.v(0, 0, 0)
                for _ in range(1000):
                    pos = pos + sun * per_step
                    depth = depth + self.medium(np.sqrt(pos @ pos) - pr)[3] * per_step
                out[y, x] = [*np.exp(-depth), 1.0]
        return self.store(out)

    def multiscatter(self, lut, directions):
        T, ar, pr = self.T, self.atmos_radius, self.planet_radius
        W, H = self.A.multiscattering_lut_size[:2]
        out = np.zeros((H, W, 4))
        for y in range(H):
            for x in range(W):
                u, v = (T(x) + T(0.5)) / T(W), (T(y) + T(0.5)) / T(H)
                altitude = pr + v * (ar - pr) + T(0.001)
                c = u * T(2) - T(1)
                sun = self.v(0, c, np.sqrt(max(T(0), T(1) - c * c)))
                lum, as1 = self.v(0, 0, 0), self.v(0, 0, 0)
                for d in directions:
                    l, m, _ = self.integrate(lut, self.v(0, altitude, 0), d.astype(T), sun, T(10), T(32), None, True)
                    as1, lum = as1 + m, lum + l
                sphere = T(4) * self.PI
                lum = lum * (sphere * (T(1) / T(64)))
                as1 = as1 * (T(1) / T(64))
                out[y, x] = [*(lum * (T(1) / sphere) * (T(1) / (T(1) - as1))), 1.0]
        return self.store(out)

    def eye_altitude(self, camera_y):
        T = self.T
        low = self.planet_radius + T(0.001)
        return max(T(np.float32(camera_y)) * T(0.01) + low, low)

    def move_to_top(self, pos, d):
        T = self.T
        h = np.sqrt(pos @ pos)
        if h > self.atmos_radius:
            top = self.nearest(pos, d, self.atmos_radius)
            if top is None:
                return None
            return pos + d * top + pos / h * -T(0.001)
        return pos

    def sky_view(self, lut, camera_position, sun_dir, sun_intensity):
        T, pr = self.T, self.planet_radius
        W, H = self.A.sky_view_lut_size[:2]
        out = np.zeros((H, W, 4))
        sun_dir = np.array([np.float32(s) for s in sun_dir], dtype=T)
        for y in range(H):
            for x in range(W):
                eye = self.v(0, self.eye_altitude(camera_position[1]), 0)
                h = np.sqrt(eye @ eye)
                u, v = (T(x) + T(0.5)) / T(W), (T(y) + T(0.5)) / T(H)
                u, v = (u - T(0.5) / T(W)) * (T(W) / (T(W) - T(1))), (v - T(0.5) / T(H)) * (T(H) / (T(H) - T(1)))
                horizon = np.sqrt(max(T(0), h * h - pr * pr))
                beta = np.arccos(horizon / h)
                zha = self.PI - beta
                if v < T(0.5):
                    coord = T(1) - v * T(2)
                    angle = zha * (T(1) - coord * coord)
                else:
                    coord = v * T(2) - T(1)
                    angle = zha + beta * coord * coord
                lon = u * T(2) * self.PI
                cz, cl = np.cos(angle), np.cos(lon)
                sz = np.sqrt(max(T(0), T(1) - cz * cz)) * (T(1) if angle > 0 else T(-1))
                sl = np.sqrt(max(T(0), T(1) - cl * cl)) * (T(1) if lon <= self.PI else T(-1))
                d = self.v(sz * cl, cz, sz * sl)
                eye = self.move_to_top(eye, d)
                if eye is None:
                    continue
                c = sun_dir @ (eye / h)
                sun = self.v(np.sqrt(max(T(0), T(1) - c * c)), c, 0)
                sun = sun / np.sqrt(sun @ sun)
                lum, _, _ = self.integrate(lut, eye, d, sun, T(np.float32(sun_intensity)), T(48))
                lum = np.where(np.isfinite(np.maximum(lum, 0)), np.maximum(lum, 0), 0)
                mult = min(max(lum.max(), T(6.103515625e-5)), T(65504))
                out[y, x] = [*(lum / mult), mult]
        return self.store(out)

    def aerial(self, lut, camera_position, inv, sun_dir, sun_intensity):
        T = self.T
        W, H, D = self.A.aerial_perspective_lut_size
        out = np.zeros((D, H, W, 4))
        m = np.asarray(inv, dtype=np.float32).astype(T).reshape(4, 4).T  # row-major
        cam = np.array([np.float32(c) for c in camera_position], dtype=T)
        sun = np.array([np.float32(s) for s in sun_dir], dtype=T)
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    u, v = (T(x) + T(0.5)) / T(W), (T(y) + T(0.5)) / T(H)
                    world = m @ self.v(T(2) * u - T(1), T(2) * v - T(1), 1, 1)
                    d = world[:3] / world[3] - cam
                    d = d / np.sqrt(d @ d)
                    eye = self.v(0, self.eye_altitude(camera_position[1]), 0)
                    slab = (T(z) + T(0.5)) * (T(1) / T(D))
                    slab = slab * slab * T(D)
                    t_max = slab * T(W // D)
                    if np.sqrt(eye @ eye) >= self.atmos_radius:
                        prev, eye = eye, self.move_to_top(eye, d)
                        if eye is None:
                            continue
                        gap = np.sqrt((prev - eye) @ (prev - eye))
                        if t_max < gap:
                            continue
                        t_max = max(T(0), t_max - gap)
                    lum, _, tr = self.integrate(lut, eye, d, sun, T(np.float32(sun_intensity)), max(T(1), (T(z) + T(1)) * T(2)), t_max)
                    out[z, y, x] = [*lum, tr @ self.v(1, 1, 1) / T(3)]
        return self.store(out)


def _difference(a, b):
    """The largest |a - b| / max(|a|, |b|, the LUT's largest magnitude * 2^-10) over two binary16 LUTs."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    floor = max(np.abs(a).max(), np.abs(b).max()) * 2.0 ** -10
    return float((np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), floor)).max())


# Measured on this transcription, binary32 against binary64 (the largest difference per LUT, in _difference's measure): transmittance 2.05e-2 --
# the 1000-step chain at a grazing ray, where a binary32 ray position near 6360 km carries 5e-4 km of rounding into exp(-altitude / 1.2) --
# multiscatter 7.7e-4, sky view 8.0e-4, aerial 8.8e-4, each one step of the binary16 store.  The bound is twice the measured figure, rounded up.
TRANSCRIPTION_BOUND = {"transmittance": 4.2e-2, "multiscatter": 2.0 ** -9, "sky view": 2.0 ** -9, "aerial": 2.0 ** -9}


@pytest.fixture(scope="module")
def transcribed():
    A = AF.small_atmosphere(transmittance=(5, 3), multiscatter=(2, 2), sky_view=(5, 4), aerial=(4, 2, 2))
    cam, sun = AF.CAMERAS["ground"], AF.SUNS["30 deg"]
    out = {}
    with np.errstate(all="ignore"):
        for T in (np.float64, np.float32):
            s = Transcription(A, T)
            t = s.transmittance()
            out[T] = (t, s.multiscatter(t, AF.hemisphere()), s.sky_view(t, cam[0], sun, AF.SUN_INTENSITY), s.aerial(t, cam[0], cam[1], sun, AF.SUN_INTENSITY))
    return A, cam, sun, out


def test_checker_against_the_transcription(transcribed):
    """The checker's four LUTs against the binary64 transcription, within TRANSCRIPTION_BOUND of the larger magnitude (texels under 2^-10 of the
    LUT's largest value: of that value).  Measured: the transcription in binary32 differs from itself in binary64 by 2.05e-2 (transmittance),
    7.7e-4 (multiscatter), 8.0e-4 (sky view) and 8.8e-4 (aerial); the bounds are twice that, 4.2e-2 and 2^-9.  The checker measured 2.05e-2,
    7.7e-4, 8.0e-4 and 8.8e-4 against the binary64 run."""
    A, cam, sun, out = transcribed
    t = AF.want_transmittance(A)
    v, a = AF.want_draw(A, cam, sun)
    got = (t, AF.want_multiscatter(A), v, a)
    for name, g, w64, w32 in zip(("transmittance", "multiscatter", "sky view", "aerial"), got, out[np.float64], out[np.float32]):
        own = _difference(w32, w64)
        diff = _difference(from_half_bits(g), w64)
        print(f"{name}: transcription binary32 vs binary64 {own:.3e}, checker vs binary64 {diff:.3e}")
        assert own <= TRANSCRIPTION_BOUND[name] and diff <= TRANSCRIPTION_BOUND[name], name


# ---- physical sanity ------------------------------------------------------------------------------------------------------------------------------
def test_physical_sanity():
    A = AF.small_atmosphere(transmittance=(17, 9), multiscatter=(5, 3), sky_view=(17, 9), aerial=(16, 16, 3))
    t = from_half_bits(AF.want_transmittance(A))
    assert (t >= 0).all() and (t <= 1).all() and (t[..., 3] == 1).all()
    # column 0 is the ray closest to the zenith (d near d_min): a higher row is a higher altitude, and more light gets through in every channel.
    # (The other columns change their zenith angle with the row, so they need not be monotone.)
    assert (np.diff(t[:, 0, :3], axis=0) >= 0).all()
    m = from_half_bits(AF.want_multiscatter(A))
    assert np.isfinite(m).all() and (m[..., :3] >= 0).all()
    for cam in ("ground", "50 km", "150 km limb"):
        v, a = (from_half_bits(x) for x in AF.want_draw(A, AF.CAMERAS[cam], AF.SUNS["30 deg"]))
        written = v.any(axis=-1)
        assert (v[written][:, 3] >= AM.HALF_MIN_NORMAL).all() and (v[written][:, 3] <= AM.HALF_MAX).all()
        assert (a[..., 3] >= 0).all() and (a[..., 3] <= 1).all() and np.isfinite(a).all()


def test_atmosphere_assert_not_degenerate():
    """The cameras and suns of the GPU test leave no branch class empty."""
    A = AF.small_atmosphere(sky_view=(17, 9), aerial=(16, 16, 3))
    counts = {}
    AF.want_multiscatter(A, counts=counts)
    for cam in AF.CAMERAS.values():
        AF.want_draw(A, cam, AF.SUNS["30 deg"], counts=counts)
    for sun in AF.SUNS.values():
        AF.want_draw(A, AF.CAMERAS["ground"], sun, counts=counts)
    for name in ("sky_view_above_horizon", "sky_view_below_horizon", "rays_hit_planet", "rays_miss_planet", "steps_earth_shadow_0", "steps_earth_shadow_1",
                 "ground_bounce_taken", "ground_bounce_not_taken", "sky_view_moved_to_top", "sky_view_missed_atmosphere", "aerial_moved_to_top",
                 "aerial_missed_atmosphere", "aerial_rejected_by_t_max"):
        assert counts.get(name, 0) > 0, f"{name}: no case ({counts})"


def test_integer_division_is_pinned():
    """5 x 3 x 2: per_slice_depth is 5 // 2 = 2; a float division (2.5) would give another LUT."""
    A = AF.small_atmosphere(aerial=(5, 3, 2))
    _, a = AF.want_draw(A, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    B = AF.small_atmosphere(aerial=(4, 3, 2))  # 4 // 2 = 2 as well: the same t_max per slice
    _, b = AF.want_draw(B, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    assert np.array_equal(from_half_bits(a)[:, :, 0, 3] < 1, from_half_bits(b)[:, :, 0, 3] < 1)
    zero = AF.small_atmosphere(aerial=(3, 3, 4))  # 3 // 4 = 0: t_max 0, nothing integrated
    _, c = AF.want_draw(zero, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    c = from_half_bits(c)
    assert (c[..., :3] == 0).all() and (c[..., 3] == 1).all()
