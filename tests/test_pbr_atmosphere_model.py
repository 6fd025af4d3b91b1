"""tests/pbr_atmosphere_model.py, the checker of oxc_apply_pbr_atmosphere, on the CPU: the library's export and the struct's layout against a
compiled probe, the cube rule, known answers worked out by hand, a comparison with a scalar transcription of pbr_apply.slang in binary64 with
libm's acos / atan2 / cos / exp / pow, and the classes and branches the GPU tests rely on."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pbr_apply_model as PM
import pbr_atmosphere_frames as PF
import pbr_atmosphere_model as AP
import sky_ibl_model as SM
from pbr_apply_model import HAS_CONTACT_SHADOWS, HAS_DIRECTIONAL_LIGHT, TRANSPARENT_BACKGROUND
from pixel_rules import from_half_bits, to_half_bits, unpack_b10g11r11, vec3_to_oct
from scenes import CAMERA, INV_PV, PBR_SUN, SUN_INTENSITY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FIELDS = ("struct_size", "width", "height", "scene_flags", "light_count", "inv_projection_view", "camera_position", "sun_dir", "sun_intensity", "atmosphere",
          "cube_size", "_pad", "depth_attachment", "albedo_attachment", "normal_attachment", "emissive_attachment", "metallic_roughness_occlusion_attachment",
          "ambient_occlusion_attachment", "resolved_shadows_attachment", "contact_shadows_attachment", "lights_buffer", "sky_transmittance_lut", "sky_view_lut",
          "sky_aerial_perspective_lut", "sky_cubemap", "final_attachment")


# ---- exports ------------------------------------------------------------------------------------------------------------------------------------
def test_export_and_struct_layout(tmp_path):
    """The symbol is exported, and sizeof / offsetof of every field agree between ctypes and the header as a C compiler lays it out."""
    from oxylus_amd import lib as L

    lib = L.load()
    assert "oxc_apply_pbr_atmosphere" in L.EXPORTS and hasattr(lib, "oxc_apply_pbr_atmosphere")
    assert [n for n, _ in L.PbrAtmosphereContext._fields_] == list(FIELDS)
    compiler = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "probe.c"
    prints = "".join(f'  printf("%zu\\n", offsetof(oxc_pbr_atmosphere_context, {n}));\n' for n in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oxcull.h"\nint main(void) {\n  printf("%zu\\n", sizeof(oxc_pbr_atmosphere_context));\n' + prints
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call([compiler, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    numbers = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert numbers[0] == C.sizeof(L.PbrAtmosphereContext)
    assert numbers[1:] == [getattr(L.PbrAtmosphereContext, n).offset for n in FIELDS]


def test_renderer_context_shares_its_sources():
    """PBRAtmosphereContext.create takes the G-buffer from the PBRContext, the LUTs, sun and camera from the AtmosphereContext, the cube and
    its size from the SkyIblContext, and allocates the output in the format the flags pick."""
    import torch

    from oxylus_amd.renderer import Atmosphere, AtmosphereContext, PBRAtmosphereContext, PBRContext, SkyIblContext

    z = lambda *s, dtype=torch.int32: torch.zeros(s, dtype=dtype)  # noqa: E731
    lights = torch.zeros(128, dtype=torch.uint8)
    p = PBRContext.create(z(4, 6, dtype=torch.float32), z(4, 6), z(4, 6, 4, dtype=torch.int16), z(4, 6), z(4, 6), z(4, 6, dtype=torch.int16), z(4, 6, dtype=torch.float32),
                          z(4, 6, dtype=torch.float32), HAS_DIRECTIONAL_LIGHT | TRANSPARENT_BACKGROUND, INV_PV, (9.0, 9.0, 9.0), (1.0, 0.0, 0.0), 1.0, lights=lights)
    a = AtmosphereContext.create(Atmosphere.engine(), "cpu", sun_dir=(0.0, 0.5, 0.5), sun_intensity=3.0, camera_position=(1.0, 2.0, 3.0))
    i = SkyIblContext.create(a, 5)
    c = PBRAtmosphereContext.create(p, a, i)
    assert c.albedo_attachment is p.albedo_attachment and c.sky_view_lut_attachment is a.sky_view_lut_attachment and c.sky_cubemap_attachment is i.sky_cubemap_attachment
    assert c.sky_aerial_perspective_lut_attachment is a.sky_aerial_perspective_lut_attachment and tuple(c.final_attachment.shape) == (4, 6, 4)
    s = c.c()
    assert s.struct_size == C.sizeof(s) and (s.width, s.height, s.cube_size, s.light_count) == (6, 4, 5, 2) and list(s.sun_dir) == [0.0, 0.5, 0.5]
    assert list(s.camera_position) == [1.0, 2.0, 3.0] and s.sun_intensity == 3.0 and s.atmosphere.planet_radius == 6360.0 and s.sky_cubemap.bytes == 6 * 5 * 5 * 8
    assert s.scene_flags == HAS_DIRECTIONAL_LIGHT | TRANSPARENT_BACKGROUND and s.lights_buffer.bytes == 128


# ---- rule F ---------------------------------------------------------------------------------------------------------------------------------------
def _index_cube(S):
    """A cube whose texel (face, y, x) holds (face, y, x, 1)."""
    face, y, x = np.mgrid[0:6, 0:S, 0:S]
    return to_half_bits(np.stack([face, y, x, np.ones_like(x)], axis=-1).astype(np.float32)).astype(np.uint16)


@pytest.mark.parametrize("S", [1, 3])
def test_axis_directions_hit_the_face_centres(S):
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    r = tuple(np.array([a[c] for a in axes], dtype=np.float32) for c in range(3))
    face, s, t = AP.cube_coords(r)
    assert face.tolist() == [0, 1, 2, 3, 4, 5] and (s == F(0.5)).all() and (t == F(0.5)).all()
    got = AP.cube_sample(_index_cube(S), r)
    assert got[0].tolist() == [0, 1, 2, 3, 4, 5] and (got[1] == S // 2).all() and (got[2] == S // 2).all() and (got[3] == 1).all()


@pytest.mark.parametrize("S", [1, 3])
def test_rule_f_inverts_step_12(S):
    """Sampling at the output_dir of oxc_generate_sky_ibl's step 12 returns that texel.  The face is exact.  (s, t) lands on the texel's
    centre to one rounding of the coordinate (measured: 6.0e-8 texels at size 3, 0 at size 1), so the bilinear weight of a neighbour is at
    most 2^-23 * S: the sample equals the texel's value to 2^-20 of the cube's largest value, and exactly at size 1 and at every face's
    centre texel."""
    dirs, (face, y, x) = SM.output_dirs(S)
    f, s, t = AP.cube_coords(dirs)
    assert (f == face).all()
    assert np.abs(s * F(S) - F(0.5) - x).max() <= 2.0 ** -23 * S and np.abs(t * F(S) - F(0.5) - y).max() <= 2.0 ** -23 * S
    got = AP.cube_sample(_index_cube(S), dirs)
    for plane, want in zip(got, (face, y, x, np.ones_like(x))):
        assert np.abs(plane - want).max() <= 5 * 2.0 ** -20
        centre = (x == S // 2) & (y == S // 2)
        assert (plane[centre] == want[centre]).all()
    if S == 1:
        assert all((plane == want).all() for plane, want in zip(got, (face, y, x, np.ones_like(x))))


def test_ties_zero_and_nan():
    """|x| == |y| picks Y, |y| == |z| and all three equal pick Z; a zero vector is +Z with 0 / 0 coordinates, a NaN vector +X: both read the
    face's texel 0 with a NaN weight -- defined, and the same on the device."""
    r = tuple(np.array(v, dtype=np.float32) for v in ([1, 0, 1, -1, 0, np.nan], [1, 1, 1, -1, 0, np.nan], [0, -1, 1, -1, 0, np.nan]))
    face, s, t = AP.cube_coords(r)
    assert face.tolist() == [2, 5, 4, 5, 4, 0]
    assert np.isnan(s[4:]).all() and np.isnan(t[4:]).all()
    got = AP.cube_sample(_index_cube(3), r)
    assert np.isnan(got[1][4:]).all() and not np.isnan(got[0][:4]).any()
    nz = tuple(np.array([v], dtype=np.float32) for v in (0.5, -0.0, 0.0))
    assert AP.cube_coords(nz)[0].tolist() == [0]
    assert AP.cube_coords(tuple(np.array([v], dtype=np.float32) for v in (0.0, 0.0, -0.0)))[0].tolist() == [4]  # a negative zero counts as positive


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------
def test_draw_sun_known_answers():
    """min_cos = cos(pi / 180) = 0.99984769...  ct = 1 >= min_cos: 1, inside.  ct = min_cos: offset 0 is still the first arm (>=).  Just below,
    offset -> 0+: exp(0) * 0.5 + (1 / 0.02) * 0.01 = 0.5 + 0.5 = 1.0 in the limit.  ct = -1: offset = 1.99984769, exp(-99992) = 0, inv = (1 /
    (0.02 + 599.954)) * 0.01 = 1.6667e-5."""
    K = AP.host_constants(PF.atmosphere(), CAMERA, PBR_SUN)
    mc = K["min_cos"]
    assert abs(float(mc) - math.cos(math.pi / 180.0)) < 6e-8
    v, inside = AP.draw_sun(mc, np.array([1.0, mc, np.nextafter(mc, F(0)), -1.0, np.nan], dtype=np.float32))
    assert inside.tolist() == [True, True, False, False, False]
    assert v[0] == 1 and v[1] == 1 and abs(float(v[2]) - 1.0) < 2e-3 and abs(float(v[3]) - 0.01 / (0.02 + 300.0 * (float(mc) + 1.0))) < 1e-9 and np.isnan(v[4])


def _one_pixel(depth, sky, A, sun_dir=PBR_SUN, flags=TRANSPARENT_BACKGROUND * 0, inv=INV_PV, camera=CAMERA, normal=(0.0, 0.0, 1.0), albedo=0xFFFFFF, mro=0x00FF8000,
               lights=None, detail=None, sun_intensity=SUN_INTENSITY):
    e = vec3_to_oct(tuple(F(v) for v in normal))
    n = np.array([[[to_half_bits(e[0]), to_half_bits(e[1]), to_half_bits(e[0]), to_half_bits(e[1])]]], dtype=np.uint16)
    one = lambda v, dt: np.array([[v]], dtype=dt)  # noqa: E731
    img, _ = AP.apply_pbr_atmosphere(one(depth, np.float32), one(albedo, np.uint32), n, one(0, np.uint32), one(mro, np.uint32), one(0x3C00, np.uint16), None, None,
                                     flags | TRANSPARENT_BACKGROUND * 0, inv, camera, sun_dir, sun_intensity, A, sky["transmittance"], sky["sky_view"], sky["aerial"],
                                     sky["cube"], lights, detail=detail)
    return unpack_b10g11r11(img.reshape(-1))


def _constant(shape, rgba):
    return np.broadcast_to(to_half_bits(np.array(rgba, dtype=np.float32)), tuple(shape) + (4,)).astype(np.uint16).copy()


def _constant_sky(A, transmittance=(1, 1, 1, 1), view=(0.5, 0.25, 0.125, 2.0), aerial=(0.5, 0.5, 0.5, 0.5), cube=(0.5, 0.25, 1.0, 0.5), S=3):
    t, v, a = A.transmittance_lut_size, A.sky_view_lut_size, A.aerial_perspective_lut_size
    return dict(transmittance=_constant((t[1], t[0]), transmittance), sky_view=_constant((v[1], v[0]), view), aerial=_constant((a[2], a[1], a[0]), aerial),
                cube=_constant((6, S, S), cube))


def test_sky_pixel_looking_straight_at_the_sun():
    """One pixel at depth 0 whose view ray is (0, 0.6, -0.8) = L, above the horizon: no planet hit, draw_sun = 1.  With a constant sky-view LUT
    (0.5, 0.25, 0.125, alpha 2), transmittance 1 and Li = 2.5 the colour is ((0.5, 0.25, 0.125) + 1 * 2.5 * 1) * 2 = (6, 5.5, 5.25)."""
    A = PF.atmosphere()
    # inv_projection_view = identity scaled so that the 1 x 1 image's centre unprojects to camera + (0, 0.6, -0.8) * 1
    cam = (0.0, 0.0, 0.0)
    inv = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0.0, 0.6, -0.8, 1.0]  # column-major: world = (nx, ny + 0.6, d - 0.8), nx = ny = 0 at the centre
    d = {}
    rgb = _one_pixel(0.0, _constant_sky(A), A, sun_dir=(0.0, 0.6, -0.8), inv=inv, camera=cam, detail=d)
    assert bool(d["sky_in_disc"][0]) and not bool(d["sky_hit"][0])
    assert [float(c[0]) for c in rgb] == [6.0, 5.5, 5.25]


def test_sky_pixel_below_the_horizon():
    """The view ray (0, -0.6, -0.8) from min_altitude hits the planet: the hit arm of the uv, no disc whatever L.  Colour = view.rgb * view.a
    = (1, 0.5, 0.25), even with the sun along the ray."""
    A = PF.atmosphere()
    inv = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0.0, -0.6, -0.8, 1.0]
    d = {}
    rgb = _one_pixel(0.0, _constant_sky(A), A, sun_dir=(0.0, -0.6, -0.8), inv=inv, camera=(0.0, 0.0, 0.0), detail=d)
    assert bool(d["sky_hit"][0]) and not bool(d["sky_in_disc"][0])
    assert [float(c[0]) for c in rgb] == [1.0, 0.5, 0.25]


def test_lit_pixel_at_relative_depth_zero_has_no_aerial_term():
    """The synthetic camera is 2.6 units = 0.026 km from the pixel; with aerial_perspective_start_km = 8 relative_depth = max(0, 0.026 - 8) = 0,
    the fade-out factor saturate(0 * 1000) = 0, weight = 0: a.rgb = 0 whatever the LUT holds, so aerial = 0 * a.w = 0."""
    A = PF.atmosphere(8.0)
    d, counts = {}, {}
    _one_pixel(0.5, _constant_sky(A, aerial=(100.0, 100.0, 100.0, 0.25)), A, detail=d)
    assert [float(c[0]) for c in d["aerial"]] == [0.0, 0.0, 0.0]
    far = {}
    _one_pixel(0.5, _constant_sky(A, aerial=(100.0, 100.0, 100.0, 0.25)), PF.atmosphere("far"), detail=far)
    assert all(float(c[0]) > 0 for c in far["aerial"])


def test_constant_cube_ties_the_ambient_to_the_no_atmosphere_model():
    """With a constant cube (rgb * a = (0.25, 0.125, 0.5)) both samples are that colour wherever they land (a + (a - a) * f = a), so the ambient
    term equals pbr_apply_model's with env = cube.rgb * cube.a * horizon_darkening, bit for bit.  env is per channel in both; transmittance 0
    and no aerial term leave the rest of the image equal too: every word of the two images is the same."""
    A = PF.atmosphere(8.0)
    inp = PF.frame()
    inp["depth"] = np.where(inp["depth"] == 0, F(0.5), inp["depth"])
    sky = _constant_sky(A, transmittance=(0, 0, 0, 1))
    K = AP.host_constants(A, CAMERA, PBR_SUN)
    env = tuple(float(F(c) * K["horizon_darkening"]) for c in (0.25, 0.125, 0.5))
    assert 0 < float(K["horizon_darkening"]) <= 1
    for flags in (0, TRANSPARENT_BACKGROUND):
        d = {}
        got = PF.want(inp, flags, A, sky, detail=d)
        st = {}
        want = PM.apply_pbr(inp["depth"], inp["albedo"], inp["normal"], inp["emissive"], inp["mro"], inp["ao"], None, None, flags, INV_PV, CAMERA, PBR_SUN, SUN_INTENSITY,
                            base_ambient_color=env, stats=st)
        assert (got == want).all()


# ---- the scalar transcription -------------------------------------------------------------------------------------------------------------------
class Slang:
    """pbr_apply.slang's fs_main with pbr.slang and sky.slang for one pixel, in Python floats (binary64) with libm; images are float64 arrays."""

    def __init__(self, A, sky, inv, camera, L, Li, lights):
        self.A, self.inv, self.cam, self.L, self.Li = A, [float(F(v)) for v in inv], [float(F(v)) for v in camera], [float(F(v)) for v in L], float(F(Li))
        self.sky = {k: from_half_bits(v).astype(np.float64) for k, v in sky.items()}
        self.lights = None if lights is None else PM.unpack_lights(lights)

    @staticmethod
    def bilinear(img, u, v):
        H, W = img.shape[:2]
        gx, gy = u * W - 0.5, v * H - 0.5
        x0, y0 = math.floor(gx), math.floor(gy)
        fx, fy = gx - x0, gy - y0
        cl = lambda i, n: min(max(int(i), 0), n - 1)  # noqa: E731
        a, b = img[cl(y0, H), cl(x0, W)], img[cl(y0, H), cl(x0 + 1, W)]
        c, d = img[cl(y0 + 1, H), cl(x0, W)], img[cl(y0 + 1, H), cl(x0 + 1, W)]
        top, bottom = a + (b - a) * fx, c + (d - c) * fx
        return top + (bottom - top) * fy

    def cube(self, r):
        ax, ay, az = abs(r[0]), abs(r[1]), abs(r[2])
        if az >= ax and az >= ay:
            face, sc, tc, ma = (5, -r[0], -r[1], az) if r[2] < 0 else (4, r[0], -r[1], az)
        elif ay >= ax:
            face, sc, tc, ma = (3, r[0], -r[2], ay) if r[1] < 0 else (2, r[0], r[2], ay)
        else:
            face, sc, tc, ma = (1, r[2], -r[1], ax) if r[0] < 0 else (0, -r[2], -r[1], ax)
        return self.bilinear(self.sky["cube"][face], sc / ma * 0.5 + 0.5, tc / ma * 0.5 + 0.5)

    def intersect(self, o, d, radius):
        a, b, c = np.dot(d, d), 2.0 * np.dot(d, o), np.dot(o, o) - radius * radius
        delta = b * b - 4.0 * a * c
        if delta < 0:
            return False
        s0, s1 = (-b - math.sqrt(delta)) / (2 * a), (-b + math.sqrt(delta)) / (2 * a)
        return not (s0 < 0 and s1 < 0)

    def brdf(self, V, N, l, albedo, roughness, metallic):
        NoV = abs(np.dot(N, V)) + 1e-5
        VL = V + l
        H = VL / np.linalg.norm(VL) if np.dot(VL, VL) > 1e-8 else N
        sat = lambda x: min(max(x, 0.0), 1.0)  # noqa: E731
        NoL, NoH, LoH = sat(np.dot(N, l)), sat(np.dot(N, H)), sat(np.dot(l, H))
        F0 = 0.04 + (albedo - 0.04) * metallic
        alpha = max(roughness * roughness, 0.0025)
        a2 = alpha * alpha
        f = (NoH * a2 - NoH) * NoH + 1.0
        D = a2 / (math.pi * f * f + 1e-7)
        Vis = sat(0.5 / (NoL * math.sqrt(NoV * NoV * (1 - a2) + a2) + NoV * math.sqrt(NoL * NoL * (1 - a2) + a2) + 1e-7))
        Fr = F0 + (1.0 - F0) * sat(1.0 - LoH) ** 5.0
        ABx, ABy = self.albedo_fit(NoV, alpha)
        Ess = sat(ABx + ABy)
        ec = 1.0 + F0 * (1.0 - Ess) / max(Ess, 1e-4)
        return (1.0 - metallic) * (1.0 - Fr) * albedo / math.pi, D * Vis * Fr * ec

    @staticmethod
    def albedo_fit(x, y):
        c = PM.ALBEDO_FIT.astype(np.float64)
        r = c[0] + c[1] * x + c[2] * y + c[3] * x * y + c[4] * x * x + c[5] * y * y + c[6] * x * x * y + c[7] * x * y * y + c[8] * x * x * y * y
        cl = lambda v: min(max(v, 0.0), 1.0)  # noqa: E731
        return cl(r[0] / r[2]), cl(r[1] / r[3])

    def pixel(self, px, py, W, H, g):
        """g: the pixel's decoded G-buffer.  -> (rgb, class)"""
        A, L, Li = self.A, np.array(self.L), self.Li
        sat = lambda x: min(max(x, 0.0), 1.0)  # noqa: E731
        u, v = (px + 0.5) / W, (py + 0.5) / H
        ndc = (u * 2 - 1, v * 2 - 1, g["depth"], 1.0)
        h = [sum(self.inv[c * 4 + r] * ndc[c] for c in range(4)) for r in range(4)]
        world = np.array(h[:3]) / h[3]
        cam = np.array(self.cam)
        V = (cam - world) / np.linalg.norm(cam - world)
        N = g["mapped"] / np.linalg.norm(g["mapped"])
        R = -V - 2.0 * np.dot(N, -V) * N
        NoV, NoL = abs(np.dot(N, V)) + 1e-5, max(np.dot(N, L), 0.0)
        pr, ar = float(F(A.planet_radius)), float(F(A.atmos_radius))
        min_alt = pr + float(F(0.001))
        sun_cos = L[1]
        s = sat((sun_cos + float(F(0.1))) / (float(F(0.3)) + float(F(0.1))))
        hd = s * s * (3 - 2 * s)

        def transmittance(alt, mu):
            hh = math.sqrt(max(0.0, ar * ar - pr * pr))
            rho = math.sqrt(max(0.0, alt * alt - pr * pr))
            disc = alt * alt * (mu * mu - 1.0) + ar * ar
            d = max(0.0, -alt * mu + math.sqrt(max(0.0, disc)))
            d_min, d_max = ar - alt, rho + hh
            return self.bilinear(self.sky["transmittance"], (d - d_min) / (d_max - d_min), rho / hh)[:3]

        sun_t = transmittance(max(world[1] * float(F(0.01)) + min_alt, min_alt), sun_cos)
        direct = sun_t * Li * hd
        if g["depth"] == 0.0:
            alt = max(cam[1] * float(F(0.01)) + min_alt, min_alt)
            eye, up = np.array([0.0, alt, 0.0]), np.array([0.0, 1.0, 0.0])
            right = np.cross(up, -V)
            right /= np.linalg.norm(right)
            forward = np.cross(right, up)
            forward /= np.linalg.norm(forward)
            lop = np.array([np.dot(L, forward), np.dot(L, right)])
            lop /= np.linalg.norm(lop)
            hit = self.intersect(eye, -V, pr)
            horizon = math.sqrt(max(0.0, alt * alt - pr * pr))
            beta = math.acos(horizon / alt)
            zha = math.pi - beta
            angle = math.acos(min(max(np.dot(-V, up), -1.0), 1.0))
            if not hit:
                uy = (1.0 - math.sqrt(max(0.0, 1.0 - angle / zha))) * 0.5
            else:
                uy = math.sqrt(max(0.0, (angle - zha) / beta)) * 0.5 + 0.5
            ux = (math.atan2(-lop[1], -lop[0]) + math.pi) / (2 * math.pi)
            vh, vw = self.sky["sky_view"].shape[:2]
            view = self.bilinear(self.sky["sky_view"], (ux + 0.5 / vw) * (vw / (vw + 1.0)), (uy + 0.5 / vh) * (vh / (vh + 1.0))).copy()
            in_disc = False
            if not hit:
                min_cos = math.cos(1.0 * math.pi / 180.0)
                ct = np.dot(-V, L)
                in_disc = ct >= min_cos
                offset = min_cos - ct
                sun = 1.0 if in_disc else math.exp(-offset * 50000.0) * 0.5 + 1.0 / (0.02 + offset * 300.0) * 0.01
                view[:3] += sun * Li * sun_t
            return view[:3] * view[3], ("sky", hit, in_disc, ux > 0.5)
        # aerial perspective
        lut = [float(n) for n in A.aerial_perspective_lut_size]
        rel = (world - cam) * float(F(0.01))
        depth = max(0.0, np.linalg.norm(rel) - float(F(A.aerial_perspective_start_km)))
        w = math.sqrt(depth / (lut[0] / lut[2]) / lut[2])
        slice_ = w * lut[2]
        weight = sat(slice_ * slice_ * 2.0) if slice_ < math.sqrt(0.5) else 1.0
        weight *= sat(depth * (1.0 / float(F(0.001))))
        D = self.sky["aerial"].shape[0]
        gz = w * D - 0.5
        z0 = math.floor(gz)
        cl = lambda i: min(max(int(i), 0), D - 1)  # noqa: E731
        a0, a1 = self.bilinear(self.sky["aerial"][cl(z0)], u, v), self.bilinear(self.sky["aerial"][cl(z0 + 1)], u, v)
        a = a0 + (a1 - a0) * (gz - z0)
        rgb = a[:3] * weight * float(F(A.aerial_perspective_exposure))
        aerial = rgb * (1.0 - weight * (1.0 - a[3]))
        # the sky ambient
        rd = N + (R - N) * (1.0 - g["roughness"])
        rd /= np.linalg.norm(rd)
        spec, diff = self.cube(rd), self.cube(N)
        specular_sky, diffuse_sky = spec[:3] * spec[3] * hd, diff[:3] * diff[3] * hd
        albedo, metallic, roughness, occlusion = g["albedo"], g["metallic"], g["roughness"], g["occlusion"]
        F0 = 0.04 + (albedo - 0.04) * metallic
        alpha = max(roughness * roughness, 0.0025)
        ABx, ABy = self.albedo_fit(NoV, alpha)
        kS = F0 * ABx + ABy
        kD = (1.0 - metallic) * (1.0 - kS)
        so = sat((NoV + occlusion) ** (2.0 ** (-16.0 * roughness - 1.0)) - 1.0 + occlusion) if NoV + occlusion > 0 else sat(-1.0 + occlusion)
        indirect = kD * diffuse_sky * albedo / math.pi * occlusion + kS * specular_sky * so
        total = np.zeros(3)
        lt = self.lights
        for i in range(0 if lt is None else len(lt["kind"])):
            kind = int(lt["kind"][i])
            if kind not in (1, 2):
                continue
            lv = lt["position"][i].astype(np.float64) - world
            dist = np.linalg.norm(lv)
            Ll = lv / dist
            rng = float(lt["range"][i])
            att = 1.0 / (dist * dist + float(F(0.1))) if rng <= 0 else max(0.0, 1.0 - (dist / rng) ** 4) ** 2 / (dist * dist + float(F(0.1)))
            if kind == 2:
                sd = lt["direction"][i].astype(np.float64)
                sd /= np.linalg.norm(sd)
                e0, e1 = math.cos(float(lt["outer_cone_angle"][i])), math.cos(float(lt["inner_cone_angle"][i]))
                t = sat((np.dot(-Ll, sd) - e0) / (e1 - e0))
                att *= t * t * (3 - 2 * t)
            intensity = float(lt["intensity"][i])
            NdotL = sat(np.dot(N, Ll))
            if att <= 0 or intensity <= 0 or NdotL <= 0:
                continue
            dif, spc = self.brdf(V, N, Ll, albedo, roughness, metallic)
            total += (dif + spc) * lt["color"][i].astype(np.float64) * att * intensity * NdotL
        hz = sat(1.0 + float(F(1.3)) * np.dot(R, g["smooth"])) ** 2
        surface = np.zeros(3)
        if NoL > 0:
            dif, spc = self.brdf(V, N, L, albedo, roughness, metallic)
            surface = (dif + spc * hz) * direct * NoL * g["visibility"]
        return surface + total + indirect + g["emission"] + aerial, ("lit", NoL > 0, False, False)


def _decoded(inp, flags):
    """The G-buffer of every pixel as the Slang's samplers and loads deliver it (exact decodes; the sRGB curve by libm's pow)."""
    H, W = inp["depth"].shape
    nh = from_half_bits(inp["normal"]).astype(np.float64)

    def oct(ex, ey):
        z = 1.0 - abs(ex) - abs(ey)
        if z < 0:
            ex, ey = (1.0 - abs(ey)) * (1.0 if ex >= 0 else -1.0), (1.0 - abs(ex)) * (1.0 if ey >= 0 else -1.0)
        v = np.array([ex, ey, z])
        return v / np.linalg.norm(v)

    em = [c.astype(np.float64).reshape(H, W) for c in unpack_b10g11r11(inp["emissive"].reshape(-1))]
    ao = from_half_bits(inp["ao"]).astype(np.float64)
    out = {}
    for y in range(H):
        for x in range(W):
            c = np.array([(int(inp["albedo"][y, x]) >> (8 * k)) & 0xFF for k in range(3)]) / 255.0
            m = [((int(inp["mro"][y, x]) >> (8 * k)) & 0xFF) / 255.0 for k in range(3)]
            vis = (float(inp["resolved"][y, x]) if flags & HAS_DIRECTIONAL_LIGHT else 1.0) * (float(inp["contact"][y, x]) if flags & HAS_CONTACT_SHADOWS else 1.0)
            out[y, x] = dict(depth=float(inp["depth"][y, x]), albedo=np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4), mapped=oct(*nh[y, x, :2]),
                             smooth=oct(*nh[y, x, 2:]), emission=np.array([e[y, x] for e in em]), metallic=min(max(m[0], 0.0), 1.0),
                             roughness=min(max(m[1], float(F(0.045))), 1.0), occlusion=m[2] * ao[y, x], visibility=vis)
    return out


# Measured on the frames below: the checker's binary32 colours against the binary64 transcription differ by at most 1.9e-4 of the larger
# magnitude (values under 2^-10: of 2^-10), in the sky arm, where acos and atan2 feed a random sky-view LUT.  The bound is four times that.
TRANSCRIPTION_BOUND = 8.0e-4
EXCLUDED_SHARE = 0.01


@pytest.mark.parametrize("start", ["near", "far"])
def test_checker_against_the_transcription(start):
    """The checker's binary32 colours of the 33 x 17 synthetic frame, before the store (sun at one empty pixel, two lights), against the
    transcription, within TRANSCRIPTION_BOUND of the larger magnitude (values under 2^-10: of 2^-10).  Pixels whose class -- planet hit, inside
    the disc, the side of the atan2 seam of the sky-view uv, NoL > 0 -- differs between the two evaluations are left out: there one rounding
    moves the tap across a discontinuity of the mapping, not of the arithmetic.  At most 1 % of the frame.  Measured, "near" and "far" alike:
    1.9e-4, with 2 of 561 pixels (0.36 %) left out, both in the sun's own column, on the seam."""
    from oxylus_amd.synth import pack_lights

    inp = PF.frame()
    H, W = inp["depth"].shape
    sun, _ = PF.sun_at_empty_pixel(inp)
    A = PF.atmosphere(start)
    sky = PF.sky_images(A)
    lights = pack_lights(PF.TWO_LIGHTS).numpy()
    flags = PF.ALL_READ
    detail = {}
    PF.want(inp, PF.ALL_READ, A, sky, lights, sun_dir=sun, detail=detail)
    # the checker's binary32 colours before the store (detail), so that the measure is the arithmetic's deviation and not the format's
    got = np.zeros((H, W, 3))
    cls = {}
    sky_at, lit_at = np.cumsum(detail["sky"]) - 1, np.cumsum(detail["lit"]) - 1
    for k, (y, x) in enumerate(zip(detail["ys"], detail["xs"])):
        if detail["sky"][k]:
            cls[int(y), int(x)] = ("sky", bool(detail["sky_hit"][sky_at[k]]), bool(detail["sky_in_disc"][sky_at[k]]), bool(detail["sky_uv"][0][sky_at[k]] > 0.5))
            got[y, x] = [float(c[sky_at[k]]) for c in detail["sky_rgb"]]
        else:
            cls[int(y), int(x)] = ("lit", bool(detail["NoL"][k] > 0), False, False)
            got[y, x] = [float(c[lit_at[k]]) for c in detail["lit_rgb"]]
    t = Slang(A, sky, INV_PV, CAMERA, sun, SUN_INTENSITY, lights)
    g = _decoded(inp, flags)
    want = np.zeros((H, W, 3))
    keep = np.ones((H, W), bool)
    with np.errstate(all="ignore"):
        for (y, x), px in g.items():
            want[y, x], c = t.pixel(x, y, W, H, px)
            keep[y, x] = (c[0], bool(c[1]), bool(c[2]), bool(c[3])) == cls[y, x]
    share = 1.0 - float(keep.mean())
    a, b = got[keep], want[keep]
    assert (np.isnan(a) == np.isnan(b)).all()  # a NaN emissive channel of the inputs is a NaN in both
    a, b = a[~np.isnan(a)], b[~np.isnan(b)]
    finite = np.isfinite(a) & np.isfinite(b)
    assert (a[~finite] == b[~finite]).all()
    a, b = a[finite], b[finite]
    floor = 2.0 ** -10  # the colours of the frame are of order 1; a few emissive pixels reach 4e4 and must not set the scale
    diff = float((np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), floor)).max())
    print(f"{start}: left out {share:.4f}, checker vs binary64 {diff:.3e}")
    assert share <= EXCLUDED_SHARE
    assert diff <= TRANSCRIPTION_BOUND


# ---- the classes ------------------------------------------------------------------------------------------------------------------------------------
def test_synthetic_inputs_reach_every_class():
    """Every class and branch the checker counts occurs on the inputs the GPU tests use: the 33 x 17 frame with the sun at one empty pixel
    under both aerial starts and both formats, and the 16 x 16 frame under 257 lights."""
    from oxylus_amd.synth import pack_lights
    from test_gpu_pbr_apply import many_lights

    inp = PF.frame()
    assert (inp["depth"] == 0).sum() > 20
    sun, (y, x) = PF.sun_at_empty_pixel(inp)
    assert inp["depth"][y, x] == 0
    lights = pack_lights(PF.TWO_LIGHTS).numpy()
    counts = {}
    for start in ("near", "far"):
        A = PF.atmosphere(start)
        for flags in (PF.ALL_READ, PF.ALL_READ | TRANSPARENT_BACKGROUND):
            PF.want(inp, flags, A, PF.sky_images(A), lights, sun_dir=sun, counts=counts)
    A = PF.atmosphere("far")
    from scenes import synthetic_inputs

    PF.want(synthetic_inputs(16, 16, seed=5), PF.ALL_READ, A, PF.sky_images(A), pack_lights(many_lights(257)).numpy(), counts=counts)
    print(counts)
    for name in AP.COUNT_NAMES:
        assert counts.get(name, 0) > 0, f"{name}: no case ({counts})"
