"""tests/visbuffer_decode_model.py against answers worked out on paper (no GPU): the normal of a triangle whose three vertex normals are equal,
lambda at a vertex, the sRGB / unorm8 / UF11 / UF10 encoders, the explicit half flush -- and, on a frame drawn by the CPU oracle's rasteriser,
that the barycentrics interpolate the depth the rasteriser stored.  Also the scene builders and the main frame tests/test_gpu_visbuffer_decode.py
uses, with the proof that the frame is not degenerate."""
import numpy as np
import pytest
import torch

import visbuffer_decode_model as VD
import vsm_draw_model as DM
from pixel_rules import srgb_unorm_encode, to_half_bits, unorm8
from scenes import DECODE_MAIN_SIZE as MAIN_SIZE
from scenes import build_scene
from scenes import decode_assert_not_degenerate as assert_not_degenerate
from scenes import main_scene

F = np.float32


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------


def oracle_frame(scene, indices, W, H):
    """(vis uint32 [H, W], depth float32 [H, W]) of the CPU oracle's rasteriser, resolved as oxc_draw_visbuffer resolves them."""
    import oracle

    vd = torch.zeros((H, W), dtype=torch.int64)
    oracle.draw_visbuffer(scene, scene.meshlet_instances, indices, scene.camera["projection_view"], W, H, vd)
    depth, vis = oracle.resolve_visbuffer(vd)
    return vis.numpy().view(np.uint32), depth.numpy()


def decode_scene(scene, vis, depth, stats=None, **kw):
    m = scene.materials
    return VD.decode(scene, scene.meshlet_instances, vis, depth, scene.camera["projection_view"], None if m is None else m.numpy(),
                     0 if m is None else m.numel() // 56, stats=stats, **kw)


# ---- answers worked out on paper ---------------------------------------------------------------------------------------------------------------
def _screen_triangle(normal):
    """One triangle that fills the screen of the identity-view camera, its three vertex normals equal."""
    pos = np.array([[-64.0, -64.0, -8.0], [64.0, -64.0, -8.0], [0.0, 96.0, -8.0]], dtype=np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 1]])
    return build_scene([(pos, tris, np.tile(np.asarray(normal, dtype=np.float32), (3, 1)))], [(0, np.eye(4), 0)])


def test_equal_vertex_normals_give_that_normal_everywhere(oracle_lib):
    """n = (0, 0, 1): 10:10:10 holds it as (511, 511, 1022) -> (0, 0, 1) exactly; the cofactor matrix of the identity is the identity;
    lambda's sum is not exactly 1, but normalize divides (0, 0, s) by s: (0, 0, 1) exactly; oct = (0 * 1, 0 * 1) = (0, 0): halves 0, 0."""
    s, idx = _screen_triangle((0.0, 0.0, 1.0))
    vis, depth = oracle_frame(s, idx, 33, 17)
    st = {}
    img = decode_scene(s, vis, depth, st)
    assert st["decoded"] == 33 * 17 and (img["normal"] == 0).all()
    # n = (1, 0, 0) decodes to (1022 / 511 - 1, 0, 0) = (1, 0, 0): z <= 0 folds: ((1 - |0|) * 1, (1 - |1|) * 1) = (1, 0): halves 0x3C00, 0
    s, idx = _screen_triangle((1.0, 0.0, 0.0))
    img = decode_scene(s, *oracle_frame(s, idx, 33, 17))
    assert (img["normal"] == np.array([0x3C00, 0, 0x3C00, 0], dtype=np.uint16)).all()


def test_pixel_centre_on_a_vertex_gives_lambda_1_0_0():
    """pv = identity, w = 1: inv_w = 1, ndc = the vertex.  Vertex 0 at the centre of pixel (2, 1) of a 4 x 4 image: uv = ((2.5 / 4) * 2 - 1,
    (1.5 / 4) * 2 - 1) = (0.25, -0.25) exactly, so d = (0, 0) exactly: interp_inv_w = (1 + 0 * a) + 0 * b = 1, lambda = (1 * ((1 + 0) + 0),
    1 * (0 + 0), 1 * (0 + 0)) = (1, 0, 0) to the last bit, whatever ddx and ddy are."""
    wp = np.array([[[0.25, -0.25, 0.5], [0.75, -0.5, 0.5], [0.5, 0.875, 0.5]]], dtype=np.float32)
    u, v = VD.pixel_ndc(np.array([2]), np.array([1]), 4, 4)
    assert (u[0], v[0]) == (F(0.25), F(-0.25))
    lam, _ = VD.barycentrics(wp, np.eye(4, dtype=np.float32).reshape(-1), u, v)
    assert lam.view(np.uint32).tolist() == [[0x3F800000, 0, 0]]


def test_srgb_bytes():
    """0 -> 0; 0.0031308f is on the linear branch: 12.92 * 0.0031308 = 0.04045 -> floor(0.04045 * 255 + 0.5) = floor(10.81) = 10;
    0.5 -> 1.055 * 0.5^(1 / 2.4) - 0.055 = 0.73536 -> floor(188.02) = 188; 1 -> pow = 1 exactly, 1.055f - 0.055f rounds to at least
    0.99999994: floor(255.49998) = 255; above 1 saturates: 255; negative and NaN: 0."""
    got = unorm8(srgb_unorm_encode(np.array([0.0, 0.0031308, 0.5, 1.0, np.nextafter(F(1.0), F(2.0)), 1.5, -0.5, np.nan, np.inf], dtype=np.float32)))
    assert got.tolist() == [0, 10, 188, 255, 255, 255, 0, 0, 255]


def test_srgb_encoder_inverts_the_binary64_decoder_on_every_byte():
    b = np.arange(256, dtype=np.float64) / 255.0
    linear = np.where(b <= 0.04045, b / 12.92, ((b + 0.055) / 1.055) ** 2.4)
    assert unorm8(srgb_unorm_encode(linear.astype(np.float32))).tolist() == list(range(256))


def test_ufloat_words():
    """UF11 = 5 exponent bits (bias 15), 6 mantissa bits; UF10 has 5.  1.0 = exponent 15; 65504 = 2^15 * 1.1111111111b truncates to exponent 30,
    mantissa all ones (65024 / 64512, the largest finite); 2^-15 is the small format's denormal with the top mantissa bit; 2^-14 * (1 + 2^-6 +
    2^-7) truncates to mantissa 1 (UF11) and 0 (UF10)."""
    v = np.array([0.0, -1.0, 1.0, 65504.0, np.inf, np.nan, 2.0 ** -15, -0.0, -np.inf, 70000.0, 2.0 ** -14 * (1 + 2.0 ** -6 + 2.0 ** -7), 2.0 ** -21, 1e-30], dtype=np.float32)
    assert VD.pack_ufloat(v, 6).tolist() == [0, 0, 15 << 6, (30 << 6) | 63, 31 << 6, (31 << 6) | 63, 32, 0, 0, (30 << 6) | 63, (1 << 6) | 1, 0, 0]
    assert VD.pack_ufloat(v, 5).tolist() == [0, 0, 15 << 5, (30 << 5) | 31, 31 << 5, (31 << 5) | 31, 16, 0, 0, (30 << 5) | 31, 1 << 5, 0, 0]
    assert VD.pack_ufloat(np.array([2.0 ** -20], dtype=np.float32), 6).tolist() == [1] and VD.pack_ufloat(np.array([2.0 ** -19], dtype=np.float32), 5).tolist() == [1]


def test_unorm8_at_the_half_way_value():
    """v * 255 + 0.5 lands on an integer for v = (k + 0.5) / 255 only up to rounding; 0.5f gives 127.5 + 0.5 = 128 exactly: floor 128."""
    assert unorm8(np.array([0.5, 0.0, 1.0, 0.5 / 255.0, np.nan, -1.0, 2.0], dtype=np.float32)).tolist() == [128, 0, 255, 1, 0, 0, 255]


def test_explicit_flush_equals_dequantize_half_on_every_half():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    a, b = VD.dequantize_half_flush(h), DM.dequantize_half(h)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])
    assert a.view(np.uint32)[0x8001] == 0x80000000 and a.view(np.uint32)[0x03FF] == 0 and a[0x0400] == F(2.0 ** -14)


def test_nan_normal_is_one_pattern():
    assert VD.normal_half(np.array([np.nan, -np.nan, 1.0, 2.0 ** -20], dtype=np.float32)).tolist() == [0x7E00, 0x7E00, 0x3C00, int(to_half_bits(F(2.0 ** -20)))]


# ---- the main frame ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_frame(oracle_lib):
    s, idx = main_scene()
    vis, depth = oracle_frame(s, idx, MAIN_SIZE, MAIN_SIZE)
    st = {}
    img = decode_scene(s, vis, depth, st)
    return s, vis, depth, img, st


def test_the_main_gpu_frame_is_not_degenerate(main_frame):
    """main_scene() drawn by the oracle's rasteriser at the GPU test's extent meets the floors the GPU test asserts on the device-drawn frame."""
    s, vis, depth, img, st = main_frame
    print(assert_not_degenerate(st, img, vis.size))
    assert st["default_material"] > 0 and (img["emissive"] != 0).any() and st["zero_vertex_index"] == 0


def _deviations(scene, depth, st, W, H):
    """(|sum(lambda) - 1|, |z/w - depth|) in binary32, the binary32-vs-binary64 deviation of both, and |z/w - depth| in binary64: the largest
    over the decoded pixels.  z/w = (sum lambda_i z_i) / (sum lambda_i w_i): lambda is perspective correct, clip z and w are linear in it."""
    t, ys, xs = st["triangle_slot"], st["ys"], st["xs"]
    lam32, clip32 = st["lam"], st["clip"]
    u, v = VD.pixel_ndc(xs, ys, W, H, np.float64)
    lam64, clip64 = VD.barycentrics(st["fetched"]["world_pos"][t].astype(np.float64), np.asarray(scene.camera["projection_view"], dtype=np.float64), u, v)

    def zw(lam, clip):
        return ((lam[:, 0] * clip[:, 0, 2] + lam[:, 1] * clip[:, 1, 2]) + lam[:, 2] * clip[:, 2, 2]) / ((lam[:, 0] * clip[:, 0, 3] + lam[:, 1] * clip[:, 1, 3]) + lam[:, 2] * clip[:, 2, 3])

    sum32, sum64 = (lam32[:, 0] + lam32[:, 1]) + lam32[:, 2], (lam64[:, 0] + lam64[:, 1]) + lam64[:, 2]
    d = depth[ys, xs].astype(np.float64)
    big = lambda a: float(np.abs(a).max())  # noqa: E731
    return dict(err_sum=big(sum32.astype(np.float64) - 1.0), err_zw=big(zw(lam32, clip32).astype(np.float64) - d), dev_sum=big(sum32.astype(np.float64) - sum64),
                dev_zw=big(zw(lam32, clip32).astype(np.float64) - zw(lam64, clip64)), err_zw_binary64=big(zw(lam64, clip64) - d))


def grid_frame(W=64, H=64, seed=5):
    """A frame whose vertices the rasteriser does not move: a 17 x 17 grid of NDC points k / 8 (pixel corners 4 k + 32 of the 64 x 64 image,
    on its 1 / 256 pixel snapping grid) with w in {1, 2, 4} per point, under the matrix of tests/test_raster.py::_persp_scene, clip = (x, y,
    0.25, w): every vertex depth 0.25 / w is exact, so the depth texel is the screen-space interpolation of z / w in binary64, rounded once."""
    rng = np.random.default_rng(seed)
    k = np.arange(-8, 9)
    gx, gy = np.meshgrid(k, k, indexing="xy")
    w = rng.choice([1.0, 2.0, 4.0], size=gx.shape)
    pos = np.stack([gx / 8.0 * w, gy / 8.0 * w, w], axis=-1).reshape(-1, 3).astype(np.float32)
    tris = []
    for r in range(16):
        for c in range(16):
            a, b, d, e = r * 17 + c, r * 17 + c + 1, (r + 1) * 17 + c, (r + 1) * 17 + c + 1
            tris += [[a, d, b], [b, d, e], [a, b, d], [b, e, d]]
    s, idx = build_scene([(pos, np.array(tris), None)], [(0, np.eye(4), 0)])
    pv = torch.zeros(4, 4)  # [col][row]
    pv[0, 0] = pv[1, 1] = 1.0
    pv[3, 2], pv[2, 3] = 0.25, 1.0
    s.camera["projection_view"] = pv.flatten().tolist()
    vis, depth = oracle_frame(s, idx, W, H)
    return s, vis, depth


def test_lambda_interpolates_the_depth_the_rasteriser_stored(oracle_lib, main_frame):
    """For every decoded pixel sum(lambda) agrees with 1 and the lambda-interpolated z / w with the depth texel, within 4 x the largest
    binary32-vs-binary64 deviation of the same formulas from the same inputs over the frame.
    Frame: grid_frame(), whose vertices lie on the rasteriser's 1 / 256 pixel grid, so that the depth texel IS the interpolated z / w.
    Measured on it: |sum - 1| <= 1.19e-07 against a deviation of 1.19e-07; |z / w - depth| <= 2.98e-08 against a deviation of 2.98e-08
    (the binary64 evaluation is within 2.8e-17 of the texel).
    On main_scene() at 256 x 256 the rasteriser snaps every vertex to 1 / 256 pixel before it interpolates, and the depth texel differs from
    the interpolation at the unsnapped vertices by up to 5.53e-06 -- in binary64 as in binary32 (deviation between the two: 9.43e-09), so
    that frame checks the sum alone (|sum - 1| <= 1.79e-06, deviation 1.79e-06) and prints the rest."""
    s, vis, depth = grid_frame()
    st = {}
    decode_scene(s, vis, depth, st)
    assert st["decoded"] == vis.size and st["distinct_triangles"] >= 500
    g = _deviations(s, depth, st, 64, 64)
    print("grid frame", {k: f"{v:.3e}" for k, v in g.items()})
    assert g["err_sum"] <= 4 * g["dev_sum"] and g["err_zw"] <= 4 * g["dev_zw"], g
    # the figures recorded above, as constants (one binary32 ulp of 1.0 and of 0.25): the bound above moves with the deviation it measures,
    # these do not, so a change of the binary32 evaluation order that loses accuracy shows here
    assert g["dev_sum"] <= 1.2e-07 and g["dev_zw"] <= 3.0e-08 and g["err_sum"] <= 4 * 1.2e-07 and g["err_zw"] <= 4 * 3.0e-08, g
    ms, mvis, mdepth, _, mst = main_frame
    m = _deviations(ms, mdepth, mst, MAIN_SIZE, MAIN_SIZE)
    print("main frame", {k: f"{v:.3e}" for k, v in m.items()})
    assert m["err_sum"] <= 4 * m["dev_sum"], m
