"""tests/textured_decode_model.py, the checker of oxc_decode_visbuffer_textured, on the CPU: hand-worked taps, LODs, a two-component normal and
the tangent frame of an axis-aligned quad; the untextured decode when no flag is set; the binary32 evaluation against a binary64
transcription of the same lines; the shared repeat axis against the tonemap checker's; the golden frame."""
import dataclasses

import numpy as np

import pixel_rules as PR
import textured_decode_frames as FR
import textured_decode_model as TM
import tonemap_model as TN
import visbuffer_decode_model as VD

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
LIN_REP, LIN_CLAMP, NEAR_REP, NEAR_CLAMP = (FR.PRESET_RECORDS[p] for p in FR.PRESETS[:4])


def image(levels, fmt=TM.UNORM):
    levels = [np.asarray(l, dtype=np.uint8) for l in levels]
    return dict(width=levels[0].shape[1], height=levels[0].shape[0], format=fmt, levels=levels)


def sample(img, sampler, uv, gx=(0.0, 0.0), gy=(0.0, 0.0), stats=None):
    a = lambda v: np.asarray([v], dtype=np.float32)  # noqa: E731
    return TM.sample_grad(img, sampler, a(uv), a(gx), a(gy), stats)[0]


TWO = image([[[[10, 20, 30, 40], [50, 60, 70, 80]], [[90, 100, 110, 120], [130, 140, 150, 160]]]])


# ---- hand-worked answers ------------------------------------------------------------------------------------------------------------------------
def test_a_tap_on_a_texel_centre():
    """2 x 2: uv = (0.25, 0.75) gives g = (0, 1): texel (0, 1) with both weights 0 under every sampler."""
    for s in (LIN_REP, LIN_CLAMP, NEAR_REP, NEAR_CLAMP):
        assert sample(TWO, s, (0.25, 0.75)).tolist() == [F(90) / F(255), F(100) / F(255), F(110) / F(255), F(120) / F(255)]


def test_a_tap_on_a_texel_edge_under_each_address_mode():
    """uv.x = 0: g = -0.5, floor -1, f = 0.5.  Repeat: texels 1 and 0 of the row, half each; clamp: texel 0 twice.  Nearest: floor(0 * 2) = 0."""
    t0, t1 = F(10) / F(255), F(50) / F(255)
    assert sample(TWO, LIN_REP, (0.0, 0.25))[0] == t1 + (t0 - t1) * F(0.5)
    assert sample(TWO, LIN_CLAMP, (0.0, 0.25))[0] == t0
    assert sample(TWO, NEAR_REP, (0.0, 0.25))[0] == t0 and sample(TWO, NEAR_CLAMP, (0.0, 0.25))[0] == t0
    # one texel to the left: repeat wraps to texel 1, clamp stays on texel 0
    assert sample(TWO, NEAR_REP, (-0.25, 0.25))[0] == t1 and sample(TWO, NEAR_CLAMP, (-0.25, 0.25))[0] == t0
    # non-finite and beyond int32: NaN converts to texel 0, +Inf saturates (INT_MAX mod 2 = 1; clamp: the last texel), -Inf likewise (INT_MIN mod 2 = 0)
    for u, rep, clamp in ((NAN, t0, t0), (INF, t1, t1), (-INF, t0, t0), (F(3e9), t1, t1), (F(-3e9), t0, t0)):
        assert sample(TWO, NEAR_REP, (u, 0.25))[0] == rep and sample(TWO, NEAR_CLAMP, (u, 0.25))[0] == clamp, u


def test_lod_of_exactly_one_and_of_one_and_a_half():
    """16 x 16 with constant levels 0.2 k: gradients of 2 texels a pixel give rho = 2, lambda = 1 exactly and level 1 alone; (2, 2) texels
    give rho = sqrt(8), lambda = 1.5 to a rounding, half of level 1 and half of level 2.  Nearest mips round 1.5 up."""
    img = image([np.full((16 >> k, 16 >> k, 4), 51 * k, np.uint8) for k in range(5)])
    st = {}
    one = sample(img, LIN_REP, (0.3, 0.6), (0.125, 0.0), (0.0, 0.125), st)
    assert st["lambda"].tolist() == [1.0] and one.tolist() == [F(51) / F(255)] * 4
    half = sample(img, LIN_REP, (0.3, 0.6), (0.125, 0.125), (0.0, 0.0625), st)
    assert abs(float(st["lambda"][0]) - 1.5) <= 2.0 ** -23 and np.abs(half - F(0.3)).max() <= 1e-7
    assert sample(img, NEAR_REP, (0.3, 0.6), (0.125, 0.125), (0.0, 0.0625)).tolist() == [F(102) / F(255)] * 4
    # magnified, zero and NaN gradients: level 0; past the last level: level 4
    for g in ((0.001, 0.0), (0.0, 0.0), (NAN, NAN)):
        assert sample(img, LIN_REP, (0.3, 0.6), g, g).tolist() == [0.0] * 4
    assert sample(img, LIN_REP, (0.3, 0.6), (50.0, 0.0), (0.0, INF)).tolist() == [F(204) / F(255)] * 4


def flat_quad():
    pos, tris, _, uv = FR.quad_mesh()
    return pos, tris, np.tile(np.array([0.0, 0.0, 1.0], np.float32), (4, 1)), uv


def test_the_tangent_frame_of_an_axis_aligned_quad_and_a_two_component_normal():
    """The quad of quad_mesh() under the identity: u grows with world x, v with world y, N = (0, 0, 1).  T is the direction of growing u,
    (1, 0, 0).  pos_ddy is the step to the pixel above, +y here, and cross(N, pos_ddx) = (0, 1, 0), so w = +1 and B = -w * cross(N, T) =
    (0, -1, 0): the Slang's bitangent points against growing v.  A two-component map of bytes (255, 128): s = (1,
    0.0039); x^2 + y^2 > 1, so z = sqrt(saturate(negative)) = 0 and the normal is normalize(T + 0.0039 B): it lies in the surface."""
    rg = image([np.full((2, 2, 2), (255, 128), np.uint8)], TM.RG8)
    f = FR.frame(9, 9, [2 | TM.TWO_COMPONENT], images=[rg], meshes=[flat_quad()], worlds=[np.eye(4)], image_indices=[[0, 0, 0, 0, 0]], holes=False)
    st = {}
    got = FR.want(f, st)
    T, B = np.stack(st["tangent"], axis=-1), np.stack(st["bitangent"], axis=-1)
    assert (st["jacobian_sign"] == 1).all() and len(T) == 81
    assert np.abs(T - [1.0, 0.0, 0.0]).max() < 1e-5 and np.abs(B - [0.0, -1.0, 0.0]).max() < 1e-5, (T[0], B[0])
    rgx, rgy = (got["normal"][..., k].view(np.float16).astype(np.float32) for k in (0, 1))
    s = np.array([F(255) / F(255) * F(2.0) - F(1.0), F(128) / F(255) * F(2.0) - F(1.0)])
    n = s / np.linalg.norm(s)  # z = 0: the octahedral fold at z <= 0 maps (x, y, 0) to ((1 - |py|) sx, (1 - |px|) sy) with p = n / (|x| + |y|)
    p = n / np.abs(n).sum()
    assert np.abs(rgx - (1 - abs(p[1]))).max() < 2e-3 and np.abs(rgy + (1 - abs(p[0]))).max() < 2e-3  # y < 0: B points down
    assert (got["normal"][..., 2:] == VD.normal_half(np.array([0.0, 0.0], np.float32))).all()  # .ba: (0, 0, 1) is (0, 0) octahedral


# ---- the untextured decode ------------------------------------------------------------------------------------------------------------------------
def test_no_flag_set_equals_the_untextured_checker():
    """Flags clear (NormalTwoComponent and NormalFlipY alone sample nothing), images and samplers present: visbuffer_decode_model.decode."""
    f = FR.frame(33, 19, [0, TM.TWO_COMPONENT | TM.FLIP_Y, 0x380, 0], mode="pixels", uv_size=[[3.0, 3.0]] * 4)
    st = {}
    got = FR.want(f, st)
    old = VD.decode(f.cpu, f.cpu.meshlet_instances, f.vis, f.depth, f.cpu.camera["projection_view"], f.cpu.materials.numpy(), 4)
    assert st["decoded"] > 500 and st["level_taps"] == 0
    for k in VD.IMAGES:
        assert np.array_equal(got[k], old[k]), k


# ---- binary32 against binary64 ----------------------------------------------------------------------------------------------------------------------
def grid_frame():
    """A 32 x 32 frame whose projected vertices lie on the 1 / 256 pixel grid, as section 15's: a 5 x 5 grid of NDC points k / 2 with w in
    {1, 2, 4}, clip = (x, y, 0.25, w) under a matrix that passes x, y and w through.  Every triangle spans 8 pixels: none is near-degenerate."""
    rng = np.random.default_rng(9)
    k = np.arange(-2, 3)
    gx, gy = np.meshgrid(k, k, indexing="xy")
    w = rng.choice([1.0, 2.0, 4.0], size=gx.shape)
    pos = np.stack([gx / 2.0 * w, gy / 2.0 * w, w], axis=-1).reshape(-1, 3).astype(np.float32)  # half-exact
    uv = np.stack([(gx + 2) / 4.0, (gy + 2) / 4.0], axis=-1).reshape(-1, 2) * 2.0
    quad = lambda i, j: (j * 5 + i, j * 5 + i + 1, (j + 1) * 5 + i + 1, (j + 1) * 5 + i)  # noqa: E731
    tris = np.array([t for j in range(4) for i in range(4) for a, b, c, d in [quad(i, j)] for t in ((a, b, c), (a, c, d))])
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (25, 1))
    f = FR.frame(32, 32, [FR.ALL_IMAGES], meshes=[(pos, tris, nrm, uv)], worlds=[np.eye(4)], holes=False, uv_size=[[4.0, 4.0]])  # minified: 2 - 16 texels a pixel
    pv = np.zeros(16, np.float32)
    pv[0] = pv[5] = 1.0   # x, y
    pv[14] = 0.25         # z = 0.25
    pv[11] = 1.0          # w = world z
    f.cpu.camera = dict(f.cpu.camera, projection_view=[float(v) for v in pv])
    ys, xs = np.mgrid[0:32, 0:32]
    i, j = xs // 8, ys // 8
    tri = ((xs % 8) < (ys % 8)).astype(np.uint32)  # below the cell's diagonal: (a, c, d)
    # one meshlet holds all 32 triangles in list order
    assert f.cpu.meshlets.shape[0] == 1
    f.vis = ((j * 4 + i) * 2 + tri).astype(np.uint32)
    return f


def test_binary32_against_the_binary64_transcription():
    """lambda, uv, the gradients and the filtered colour of the checker against the same lines in binary64 (real log2, real sRGB curve) on
    grid_frame(), and a property the lines must have: the final ddx / ddy are exact differences, uv_ddx = uv(x + 1, y) - uv(x, y) and
    uv_ddy = uv(x, y - 1) - uv(x, y) inside a triangle.  Bound: 4 x the largest binary32-vs-binary64 deviation of the same quantity on the
    frame, the margin of DESIGN.md section 15.  Measured: uv 1.13e-06 (uv reaches 8), gradients 8.5e-07, lambda 1.04e-05, colour 7.4e-06; the difference
    property holds to 1.31e-06.  The constants below are those figures: the relative bound moves with what it measures, they do not."""
    f = grid_frame()
    st = {}
    FR.want(f, st)
    assert st["decoded"] == 1024 and st["distinct_triangles"] == 32
    t, ys, xs = st["triangle_slot"], st["ys"], st["xs"]
    world = st["fetched"]["world_pos"][t].astype(np.float64)
    u, v = VD.pixel_ndc(xs, ys, 32, 32, np.float64)
    lam, bx, by = TM.partials(world, np.asarray(f.cpu.camera["projection_view"], np.float64), u, v, 32, 32)
    tc = TM.fetch_texcoords(f.cpu, f.cpu.meshlet_instances.numpy().reshape(-1, 2), st["fetched"], np.unique(f.vis))[t].astype(np.float64)
    uv, gx, gy = TM.uv_gradient(lam, bx, by, tc, np.full(2, 4.0), np.zeros(2))
    img = f.images[0]
    s64, s32 = {}, {}
    c64 = TM.sample_grad(img, LIN_REP, uv, gx, gy, s64)
    c32 = TM.sample_grad(img, LIN_REP, st["uv"], st["uv_ddx"], st["uv_ddy"], s32)
    big = lambda a: float(np.abs(a).max())  # noqa: E731
    dev = dict(uv=big(st["uv"] - uv), grad=max(big(st["uv_ddx"] - gx), big(st["uv_ddy"] - gy)), lam=big(s32["lambda"] - s64["lambda"]), colour=big(c32 - c64))
    # the difference property, in binary32, between horizontal and vertical neighbours of one triangle
    grid = np.zeros((32, 32, 2), np.float32)
    grid[ys, xs] = st["uv"]
    ddx, ddy = np.zeros_like(grid), np.zeros_like(grid)
    ddx[ys, xs], ddy[ys, xs] = st["uv_ddx"], st["uv_ddy"]
    same_x, same_y = f.vis[:, 1:] == f.vis[:, :-1], f.vis[1:] == f.vis[:-1]
    err = max(big((grid[:, 1:] - grid[:, :-1] - ddx[:, :-1])[same_x]), big((grid[:-1] - grid[1:] - ddy[1:])[same_y]))
    print("deviations", {k: f"{v:.3e}" for k, v in dev.items()}, f"difference property {err:.3e}")
    assert same_x.sum() > 700 and same_y.sum() > 700
    inside = (s64["lambda"] > 0.0) & (s64["lambda"] < 4.0)
    assert inside.mean() > 0.8 and float(s64["lambda"].min()) > 0.25, (inside.mean(), s64["lambda"].min())  # minified: the trilinear path, inside the chain
    assert err <= 4 * max(dev["uv"], dev["grad"]), (err, dev)
    assert dev["uv"] <= 1.2e-06 and dev["grad"] <= 9.0e-07 and dev["lam"] <= 1.1e-05 and dev["colour"] <= 8.0e-06, dev


# ---- the shared repeat axis -------------------------------------------------------------------------------------------------------------------------
def test_the_repeat_axis_is_the_tonemap_checkers():
    """textured_decode_model.axis_repeat is wrap_axis, which oxc_apply_tonemap's taps use: a bilinear built from it equals tonemap_model.bilinear_repeat
    on a sweep of coordinates, NaN and +-Inf and values beyond int32 included, bit for bit; and its indices stay inside the level."""
    rng = np.random.default_rng(3)
    coords = np.concatenate([np.linspace(-3.0, 3.0, 193), [NAN, INF, -INF, 3e9, -3e9, 1e38, -0.0, np.nextafter(F(1.0), F(2.0)), 2.0 ** -149]]).astype(np.float32)
    for w, h in ((1, 1), (2, 3), (5, 3), (16, 16)):
        plane = rng.random((h, w)).astype(np.float32)
        u, v = np.meshgrid(coords, coords)
        u, v = u.reshape(-1), v.reshape(-1)
        (x0, x1, fx), (y0, y1, fy) = TM.axis_repeat(u, w), TM.axis_repeat(v, h)
        assert min(x0.min(), x1.min(), y0.min(), y1.min()) >= 0 and max(x0.max(), x1.max()) < w and max(y0.max(), y1.max()) < h
        with np.errstate(all="ignore"):
            mine = PR.lerp(PR.lerp(plane[y0, x0], plane[y0, x1], fx), PR.lerp(plane[y1, x0], plane[y1, x1], fx), fy)
        assert np.array_equal(mine.view(np.uint32), TN.bilinear_repeat(plane, u, v).view(np.uint32)), (w, h)


# ---- the golden frame -------------------------------------------------------------------------------------------------------------------------------
def test_the_golden_frame():
    """tests/golden/textured_decode_17x9.npz (written by textured_decode_frames.py run as a script): five presets, three formats, flip-y and a
    two-component map under 64-way divergent tiles.  The checker still gives its images and counters."""
    g = np.load(FR.GOLDEN)
    f = FR.golden_frame()
    assert np.array_equal(f.vis, g["vis"])
    st = {}
    got = FR.want(f, st)
    for k in VD.IMAGES:
        assert np.array_equal(got[k], g["want_" + k]), k
    assert [TM.counters(st)[k] for k in TM.COUNTER_NAMES] == g["counters"].tolist()
    assert all(st["sampled_" + k] > 0 for k in TM.KINDS) and st["per_lane_waves"] > 0
    plain = FR.want(dataclasses.replace(f, images=[], samplers=[]))
    assert (got["albedo"] != plain["albedo"]).any() and (got["normal"][..., :2] != plain["normal"][..., :2]).any()
