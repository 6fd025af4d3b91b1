"""oxc_generate_sky_ibl on the GPU against tests/sky_ibl_model.py: every word of the cube equal to the checker's, between poisoned guard bands,
both LUT inputs unchanged (sky_ibl_frames.run).  The realistic frames read the LUT checker's sky-view and transmittance LUTs, the small ones
random halves with hand-placed NaN / Inf / HALF_MAX texels.  cube_size 1, 2, 3 and 5 are less than one block, an odd count of waves and more
than one block; 32 is the engine's."""
import dataclasses

import numpy as np
import pytest
import torch

import atmosphere_frames as AF
import sky_ibl_frames as SF
import sky_ibl_model as SM
from refusals import raises_refusal

pytestmark = pytest.mark.gpu

ENGINE_LUTS, SMALL_LUTS, TINY_LUTS = ((312, 192), (256, 64)), ((17, 9), (2, 2)), ((2, 2), (2, 2))
REACHABLE = tuple(c for c in SM.CLASSES if c != "side_vec_fallback")  # an exactly vertical input_dir: covered in test_sky_ibl_model.py


@pytest.fixture(scope="module")
def r():
    from oxylus_amd.renderer import RendererInstance

    inst = RendererInstance(0)
    yield inst
    inst.close()


def _luts(sizes, camera="ground", sun="30 deg"):
    A = SF.atmosphere(*sizes)
    if sizes == ENGINE_LUTS:
        return (A,) + SF.realistic_luts(A, camera, sun)
    return A, SF.random_lut(*sizes[0], seed=11), SF.random_lut(*sizes[1], seed=12, alpha_scale=1.0, special=sizes[1] != (2, 2))


def _no_nan_or_inf(cube, label):
    assert ((cube & 0x7C00) != 0x7C00).all(), f"{label}: a NaN or Inf half was stored"


@pytest.mark.parametrize("sizes", [ENGINE_LUTS, SMALL_LUTS, TINY_LUTS], ids=["engine", "17x9", "2x2"])
@pytest.mark.parametrize("cube_size", [1, 2, 3, 5, 32])
def test_sizes(r, cube_size, sizes):
    """A zeroed cube, then the same call on its own output: no history, then history in every texel."""
    A, view, trans = _luts(sizes)
    cam, sun = SF.CAMERAS["ground"], SF.SUNS["30 deg"]
    first = SF.run(r, A, view, trans, np.zeros((6, cube_size, cube_size, 4), np.uint16), cam, sun, f"{cube_size} {sizes} first")
    second = SF.run(r, A, view, trans, first, cam, sun, f"{cube_size} {sizes} second", frame_index=1)
    assert (first[..., 3] == SF.HALF_ONE).all() and (second[..., 3] == SF.HALF_ONE).all()
    _no_nan_or_inf(second, "second")


def test_cameras_suns_and_branch_classes(r):
    """Every camera under the 30-degree sun and every sun from the ground, each on the LUT checker's LUTs for that camera and sun, then the
    frames that reach the remaining classes; no reachable class of the checker stays empty."""
    counts = {}
    A = SF.atmosphere((17, 9), (17, 9))
    cube = SF.history_patterns(5)
    for camera in SF.CAMERAS:
        view, trans = SF.realistic_luts(A, camera, "30 deg")
        SF.run(r, A, view, trans, cube, SF.CAMERAS[camera], SF.SUNS["30 deg"], camera, frame_index=3, counts=counts)
    for sun in SF.SUNS:
        view, trans = SF.realistic_luts(A, "ground", sun)
        SF.run(r, A, view, trans, cube, SF.CAMERAS["ground"], SF.SUNS[sun], f"sun {sun}", frame_index=4, counts=counts)
    B, view, trans = _luts(SMALL_LUTS)
    SF.run(r, B, view, trans, cube, SF.CAMERAS["ground"], SF.SUNS["30 deg"], "special texels", counts=counts)
    SF.run(r, B, view, trans, cube, SF.CAMERAS["ground"], SF.SUNS["30 deg"], "the clamp", sun_intensity=3.0e38, strength=1.0e30, counts=counts)
    for name in REACHABLE:
        assert counts.get(name, 0) > 0, f"{name}: no case ({counts})"


@pytest.mark.parametrize("strength", [0.15, float("nan"), float("inf"), -1.0, 3.0e38])
@pytest.mark.parametrize("intensity", [float("nan"), float("inf"), -1.0, 3.0e38])
def test_no_nan_or_inf_is_stored(r, intensity, strength):
    """What sanitize exists for: whatever the sun's factors, and with NaN / Inf texels in the sky-view LUT, no stored half is a NaN or Inf."""
    A, view, trans = _luts(SMALL_LUTS)
    for cube in (np.zeros((6, 3, 3, 4), np.uint16), SF.history_patterns(3)):
        got = SF.run(r, A, view, trans, cube, SF.CAMERAS["ground"], SF.SUNS["30 deg"], f"{intensity} {strength}", sun_intensity=intensity, strength=strength)
        _no_nan_or_inf(got, f"{intensity} {strength}")


def test_history_patterns(r):
    """Zero, alpha 0 / negative / -0.0 / NaN / positive denormal, alpha 1 with one non-finite colour channel, colours at HALF_MAX."""
    A, view, trans = _luts(ENGINE_LUTS)
    counts = {}
    cube = SF.history_patterns(5)
    got = SF.run(r, A, view, trans, cube, SF.CAMERAS["ground"], SF.SUNS["30 deg"], "history", frame_index=7, counts=counts)
    n = cube.size // 4
    kind = np.arange(n) % 11
    assert counts["has_history"] == int(np.isin(kind, (5, 9, 10)).sum()) and counts["no_history"] == n - counts["has_history"]
    _no_nan_or_inf(got, "history")


def test_three_successive_frames(r):
    """frame_index 0, 1, 2 on the call's own output: each cube equals the checker applied to the previous one."""
    A, view, trans = _luts(ENGINE_LUTS)
    cube = np.zeros((6, 5, 5, 4), np.uint16)
    seen = []
    for frame in range(3):
        cube = SF.run(r, A, view, trans, cube, SF.CAMERAS["ground"], SF.SUNS["30 deg"], f"frame {frame}", frame_index=frame)
        seen.append(cube)
    assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any()


@pytest.mark.parametrize("frame_index", [2 ** 24 + 1, 0xFFFFFFFF])
def test_large_frame_index(r, frame_index):
    """2^24 + 1 is the first index f32() rounds; 0xFFFFFFFF rounds up to 2^32."""
    A, view, trans = _luts(SMALL_LUTS)
    a = SF.run(r, A, view, trans, SF.history_patterns(3), SF.CAMERAS["ground"], SF.SUNS["30 deg"], f"frame {frame_index}", frame_index=frame_index)
    b = SF.want(A, view, trans, SF.history_patterns(3), SF.CAMERAS["ground"], SF.SUNS["30 deg"], frame_index=3)
    assert (a != b).any()  # the index shows


def test_captured_graph(r):
    """Draw -> decode -> resolve -> contact shadows -> ambient occlusion (gpu_passes.DrawnFrame.passes) -> generate_sky_luts -> draw_atmosphere
    -> generate_sky_ibl captured into one graph on one stream, pre-sized by one eager run of every call.  frame_index travels by value, so
    every replay runs with the captured index; the cube is memory, so replay k works on the cube replay k - 1 left: after replay k the cube
    equals the checker iterated k times with that index on the LUT checker's LUTs, the guard bands are intact and the decode's normal image
    equals the eager run's."""
    from gpu_passes import DrawnFrame, same
    from oxylus_amd.renderer import SkyLutContext

    A = AF.small_atmosphere(sky_view=(17, 9), aerial=(16, 16, 3))
    cam, sun, frame_index = AF.CAMERAS["ground"], AF.SUNS["30 deg"], 5
    table = torch.from_numpy(AF.hemisphere()).cuda()
    guards = AF.lut_guards(A)
    luts = SkyLutContext(AF.renderer_atmosphere(A), table, guards[0].tensor, guards[1].tensor)
    draw = AF.draw_context(A, guards, cam, sun)
    zero = np.zeros((6, 5, 5, 4), np.uint16)
    cube = SF.guard("sky_cubemap", zero)
    ibl = SF.context(A, (guards[2], guards[0], cube), cam[0], sun, frame_index=frame_index)
    frame = DrawnFrame(r)
    frame.passes()  # eager: every scratch buffer has its size before the capture
    r.generate_sky_luts(luts)
    r.draw_atmosphere(draw)
    r.generate_sky_ibl(ibl)
    torch.cuda.synchronize()
    normals = frame.dctx.normal_attachment.cpu().numpy().copy()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        frame.passes(stream)
        r.generate_sky_luts(luts, stream=stream)
        r.draw_atmosphere(draw, stream=stream)
        r.generate_sky_ibl(ibl, stream=stream)
    cube.tensor.zero_()
    want_t, want_v = AF.want_transmittance(A), AF.want_draw(A, cam, sun)[0]
    expected = zero
    for replay in range(3):
        for g in guards:
            g.refill()
        frame.dctx.normal_attachment.fill_(-5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        expected = SF.want(A, want_v, want_t, expected, cam[0], sun, frame_index=frame_index)
        label = f"graph, replay {replay}"
        cube.check(label)
        same(cube.bits()[1].reshape(expected.shape), expected, f"{label}: sky_cubemap")
        same(guards[2].bits()[1].reshape(want_v.shape), want_v, f"{label}: sky_view_lut")
        same(frame.dctx.normal_attachment.cpu().numpy(), normals, f"{label}: normal_attachment")


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
def _refused(call, message, gs, before):
    raises_refusal(call, message)
    for g, data in zip(gs, before):
        g.check("refused")
        assert (g.bits()[1] == data.reshape(-1)).all(), f"{g.name} was written"


@pytest.fixture(scope="module")
def refusal(r):
    A = SF.atmosphere((17, 9), (5, 3))
    view, trans, cube = SF.random_lut(17, 9, seed=11), SF.random_lut(5, 3, seed=12, alpha_scale=1.0), SF.history_patterns(3)
    gs = SF.guards(view, trans, cube)
    return A, gs, (view, trans, cube), SF.context(A, gs, SF.CAMERAS["ground"], SF.SUNS["30 deg"])


NULL, ALIGNED, SHORT = "must not be null", "must be aligned to 8 bytes", "is smaller than its extent"


def _cases(A, gs):
    """(changes to the context, message) for every limit on its own, in the header's order."""
    atm = AF.renderer_atmosphere(A)
    rep = dataclasses.replace
    v, t, c = (g.tensor for g in gs)
    flat = lambda x: x.view(-1)  # noqa: E731
    return [
        (dict(atmosphere=rep(atm, sky_view_lut_size=(1, 9, 1))), "sky_view_lut_size"),
        (dict(atmosphere=rep(atm, sky_view_lut_size=(17, 4097, 1))), "sky_view_lut_size"),
        (dict(atmosphere=rep(atm, transmittance_lut_size=(2, 1, 1))), "transmittance_lut_size"),
        (dict(atmosphere=rep(atm, transmittance_lut_size=(4097, 2, 1))), "transmittance_lut_size"),
        (dict(cube_size=0), "cube_size must be in 1 .. 1024"),
        (dict(cube_size=1025), "cube_size must be in 1 .. 1024"),
        (dict(atmosphere=rep(atm, planet_radius=float("inf"))), "must be finite"),
        (dict(atmosphere=rep(atm, atmos_radius=float("nan"))), "must be finite"),
        (dict(atmosphere=rep(atm, planet_radius=0.0)), "planet_radius must be above 0"),
        (dict(atmosphere=rep(atm, atmos_radius=6360.0)), "atmos_radius must be above planet_radius"),
        (dict(sky_view_lut_attachment=None), "sky_view_lut " + NULL),
        (dict(sky_view_lut_attachment=flat(v)[2:]), "sky_view_lut " + ALIGNED),
        (dict(sky_view_lut_attachment=flat(v)[:-4]), "sky_view_lut " + SHORT),
        (dict(sky_transmittance_lut_attachment=None), "sky_transmittance_lut " + NULL),
        (dict(sky_transmittance_lut_attachment=flat(t)[2:]), "sky_transmittance_lut " + ALIGNED),
        (dict(sky_transmittance_lut_attachment=flat(t)[:-4]), "sky_transmittance_lut " + SHORT),
        (dict(sky_cubemap_attachment=None), "sky_cubemap " + NULL),
        (dict(sky_cubemap_attachment=flat(c)[2:]), "sky_cubemap " + ALIGNED),
        (dict(sky_cubemap_attachment=flat(c)[:-4]), "sky_cubemap " + SHORT),
        (dict(sky_cubemap_attachment=v, cube_size=1), "sky_cubemap must not overlap sky_view_lut"),
        (dict(sky_cubemap_attachment=t, cube_size=1), "sky_cubemap must not overlap sky_transmittance_lut"),
    ]


def test_every_limit_on_its_own(r, refusal):
    A, gs, before, base = refusal
    for change, message in _cases(A, gs):
        _refused(lambda: r.generate_sky_ibl(dataclasses.replace(base, **change)), message, gs, before)


def test_the_first_broken_rule_gives_the_message(r, refusal):
    """Two rules broken at once, for every neighbouring pair of the header's order: the earlier one is named."""
    A, gs, before, base = refusal
    atm = AF.renderer_atmosphere(A)
    rep = dataclasses.replace
    v, t, c = (g.tensor for g in gs)
    flat = lambda x: x.view(-1)  # noqa: E731
    for change, message in (
            (dict(atmosphere=rep(atm, sky_view_lut_size=(1, 9, 1), transmittance_lut_size=(1, 2, 1))), "sky_view_lut_size"),
            (dict(atmosphere=rep(atm, transmittance_lut_size=(1, 2, 1)), cube_size=0), "transmittance_lut_size"),
            (dict(cube_size=2000, atmosphere=rep(atm, planet_radius=float("nan"))), "cube_size must be in 1 .. 1024"),
            (dict(atmosphere=rep(atm, planet_radius=float("inf"), atmos_radius=1.0)), "must be finite"),
            (dict(atmosphere=rep(atm, planet_radius=-1.0, atmos_radius=-2.0)), "planet_radius must be above 0"),
            (dict(atmosphere=rep(atm, atmos_radius=6000.0), sky_view_lut_attachment=None), "atmos_radius must be above planet_radius"),
            (dict(sky_view_lut_attachment=None, sky_transmittance_lut_attachment=None), "sky_view_lut " + NULL),
            (dict(sky_view_lut_attachment=flat(v)[2:100]), "sky_view_lut " + ALIGNED),
            (dict(sky_view_lut_attachment=flat(v)[:-4], sky_transmittance_lut_attachment=None), "sky_view_lut " + SHORT),
            (dict(sky_transmittance_lut_attachment=None, sky_cubemap_attachment=None), "sky_transmittance_lut " + NULL),
            (dict(sky_transmittance_lut_attachment=flat(t)[2:8]), "sky_transmittance_lut " + ALIGNED),
            (dict(sky_transmittance_lut_attachment=flat(t)[:-4], sky_cubemap_attachment=None), "sky_transmittance_lut " + SHORT),
            (dict(sky_cubemap_attachment=flat(c)[2:8]), "sky_cubemap " + ALIGNED),
            (dict(sky_cubemap_attachment=flat(v)[:-4], cube_size=6), "sky_cubemap " + SHORT)):
        _refused(lambda: r.generate_sky_ibl(rep(base, **change)), message, gs, before)


def test_null_context_and_short_struct_size(r):
    import ctypes as C

    from oxylus_amd import lib as L

    lib = L.load()
    assert lib.oxc_generate_sky_ibl(r._ctx, None, None) == L.OXC_INVALID_ARG
    assert lib.oxc_generate_sky_ibl(None, None, None) == L.OXC_INVALID_ARG
    c = L.SkyIblContext()
    c.struct_size = C.sizeof(L.SkyIblContext) - 8
    assert lib.oxc_generate_sky_ibl(r._ctx, C.byref(c), None) == L.OXC_INVALID_ARG
    assert b"struct_size" in lib.oxc_last_error(r._ctx)
