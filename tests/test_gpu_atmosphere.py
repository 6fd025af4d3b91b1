"""oxc_generate_sky_luts and oxc_draw_atmosphere on the GPU against tests/atmosphere_model.py: every word of every LUT equal to the checker's,
between poisoned guard bands (atmosphere_frames.run_sky_luts / run_draw).  The draw tests feed the checker's own transmittance and multiscatter
LUTs, so each case stands alone; the captured-graph test chains the two calls.  The extents are the smallest at which the indexing can go wrong:
odd sides, sides that are no multiple of the 64-texel block, more than one block, the aerial integer division 5 / 2 and x < z."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import atmosphere_frames as AF
import atmosphere_model as AM
from refusals import raises_refusal

pytestmark = pytest.mark.gpu

CLASSES = ("sky_view_above_horizon", "sky_view_below_horizon", "rays_hit_planet", "rays_miss_planet", "steps_earth_shadow_0", "steps_earth_shadow_1",
           "ground_bounce_taken", "sky_view_moved_to_top", "sky_view_missed_atmosphere", "aerial_moved_to_top", "aerial_missed_atmosphere",
           "aerial_rejected_by_t_max")


@pytest.fixture(scope="module")
def r():
    from oxylus_amd.renderer import RendererInstance

    inst = RendererInstance(0)
    yield inst
    inst.close()


def test_engine_defaults(r):
    """256 x 64, 32 x 32, 312 x 192 and 32^3, the component defaults scaled by 1e-3, the camera at the ground, the sun at 30 degrees."""
    A = AF.engine_atmosphere()
    AF.run_sky_luts(r, A, "engine")
    AF.run_draw(r, A, AF.CAMERAS["ground"], AF.SUNS["30 deg"], "engine")


@pytest.mark.parametrize("transmittance", [(2, 2), (17, 9), (65, 3)])
@pytest.mark.parametrize("multiscatter", [(2, 2), (5, 3)])
def test_sky_luts_small_extents(r, transmittance, multiscatter):
    AF.run_sky_luts(r, AF.small_atmosphere(transmittance=transmittance, multiscatter=multiscatter), f"{transmittance} {multiscatter}")


@pytest.mark.parametrize("sky_view,aerial", [((2, 2), (2, 2, 1)), ((17, 9), (5, 3, 2)), ((65, 33), (3, 3, 4)), ((17, 9), (16, 16, 33))])
def test_draw_small_extents(r, sky_view, aerial):
    """5 x 3 x 2: the integer division 5 / 2 = 2 where a float division would give 2.5; 3 x 3 x 4: x < z, per_slice_depth 0."""
    AF.run_draw(r, AF.small_atmosphere(sky_view=sky_view, aerial=aerial), AF.CAMERAS["ground"], AF.SUNS["30 deg"], f"{sky_view} {aerial}")


def test_cameras_suns_and_branch_classes(r):
    """Every camera under the 30-degree sun and every sun from the ground; over them and one generate call, no class of
    atmosphere_assert_not_degenerate is empty."""
    A = AF.small_atmosphere(sky_view=(17, 9), aerial=(16, 16, 3))
    counts = {}
    AF.want_multiscatter(A, counts=counts)
    AF.run_sky_luts(r, A, "classes")
    for name, cam in AF.CAMERAS.items():
        AF.run_draw(r, A, cam, AF.SUNS["30 deg"], name, counts=counts)
    for name, sun in AF.SUNS.items():
        AF.run_draw(r, A, AF.CAMERAS["ground"], sun, name, counts=counts)
    AF.run_draw(r, A, AF.CAMERAS["50 km"], AF.SUNS["below"], "50 km, sun below", counts=counts)
    for name in CLASSES:
        assert counts.get(name, 0) > 0, f"{name}: no case ({counts})"


def test_all_zero_texels_looking_away(r):
    A = AF.small_atmosphere(aerial=(5, 3, 2))
    _, aerial = AF.run_draw(r, A, AF.CAMERAS["150 km away"], AF.SUNS["30 deg"], "away")
    assert not aerial.any()


@pytest.mark.parametrize("name,overrides", [
    ("zero rayleigh density", dict(rayleigh_density=0.0)),
    ("zero mie density", dict(mie_density=0.0)),
    ("zero ozone thickness", dict(ozone_thickness=0.0)),
    ("asymmetry on the g_hg pole", dict(mie_asymmetry=1.67154)),
    ("asymmetry on the w_d pole", dict(mie_asymmetry=0.641583)),
    ("asymmetry 0.8", dict(mie_asymmetry=0.8)),
])
def test_extreme_atmosphere_fields(r, name, overrides):
    """Division by zero in exp(-altitude / 0), the poles of the Draine constants: the checker's bytes, no special cases."""
    A = AF.small_atmosphere(transmittance=(9, 5), **overrides)
    AF.run_sky_luts(r, A, name)
    AF.run_draw(r, A, AF.CAMERAS["ground"], AF.SUNS["30 deg"], name)


@pytest.mark.parametrize("intensity", [float("nan"), float("inf"), -1.0, 0.0])
def test_non_finite_sun_intensity(r, intensity):
    AF.run_draw(r, AF.small_atmosphere(), AF.CAMERAS["ground"], AF.SUNS["30 deg"], f"intensity {intensity}", sun_intensity=intensity)


def test_hemisphere_tables(r):
    A = AF.small_atmosphere()
    same_direction = np.tile(AF.hemisphere()[5], (64, 1)).astype(np.float32)
    AF.run_sky_luts(r, A, "all equal", same_direction)
    one_down = AF.hemisphere().copy()
    one_down[17] = (0.0, -1.0, 0.0)
    AF.run_sky_luts(r, A, "one straight down", one_down)


def test_captured_graph(r):
    """Draw -> decode -> resolve -> contact shadows -> ambient occlusion (gpu_passes.DrawnFrame.passes, the chain the other graph tests
    capture) -> generate_sky_luts -> draw_atmosphere captured into one graph on one stream, pre-sized by one eager run of every call.  The sun
    travels by value in the context, as the reference's push constants do, so moving it means capturing again: one capture per sun, three
    suns, and EACH captured graph is replayed three times with all four LUTs refilled with the pre-fill pattern between the replays.  After
    every replay every word of the four LUTs equals the checker's for that capture's sun, the guard bands are intact, and the decode's normal
    image equals the eager run's (the chain in front ran)."""
    from gpu_passes import DrawnFrame, same
    from oxylus_amd.renderer import SkyLutContext

    A = AF.small_atmosphere(sky_view=(17, 9), aerial=(16, 16, 3))
    table = torch.from_numpy(AF.hemisphere()).cuda()
    guards = AF.lut_guards(A)
    luts = SkyLutContext(AF.renderer_atmosphere(A), table, guards[0].tensor, guards[1].tensor)
    frame = DrawnFrame(r)
    frame.passes()  # eager: every scratch buffer has its size before the capture
    r.generate_sky_luts(luts)
    r.draw_atmosphere(AF.draw_context(A, guards, AF.CAMERAS["ground"], AF.SUNS["30 deg"]))
    torch.cuda.synchronize()
    normals = frame.dctx.normal_attachment.cpu().numpy().copy()
    want_t, want_m = AF.want_transmittance(A), AF.want_multiscatter(A)
    stream = torch.cuda.Stream()
    views = []
    for sun_name in ("30 deg", "horizon", "zenith"):
        ctx = AF.draw_context(A, guards, AF.CAMERAS["ground"], AF.SUNS[sun_name])
        want_v, want_a = AF.want_draw(A, AF.CAMERAS["ground"], AF.SUNS[sun_name])
        views.append(want_v)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            frame.passes(stream)
            r.generate_sky_luts(luts, stream=stream)
            r.draw_atmosphere(ctx, stream=stream)
        for replay in range(3):
            for g in guards:
                g.refill()
            frame.dctx.normal_attachment.fill_(-5)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            label = f"graph, sun {sun_name}, replay {replay}"
            for g, want in zip(guards, (want_t, want_m, want_v, want_a)):
                g.check(label, want)
                same(g.bits()[1].reshape(want.shape), want, f"{label}: {g.name}")
            same(frame.dctx.normal_attachment.cpu().numpy(), normals, f"{label}: normal_attachment")
    assert (views[0] != views[1]).any() and (views[1] != views[2]).any()  # the sun shows


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
def _refused(call, message, guards):
    raises_refusal(call, message)
    for g in guards:
        g.check("refused")
        if g.fill is not None:
            assert (g.bits()[1] == g.fill).all(), f"{g.name} was written"


SIZE_CASES = [("transmittance_lut_size", (1, 9, 1)), ("transmittance_lut_size", (17, 4097, 1)), ("multiscattering_lut_size", (5, 1, 1)),
              ("multiscattering_lut_size", (4097, 3, 1))]


@pytest.mark.parametrize("field,value", SIZE_CASES + [("planet_radius", float("inf")), ("atmos_radius", float("nan")), ("planet_radius", 0.0),
                                                      ("planet_radius", -1.0), ("atmos_radius", 6360.0), ("atmos_radius", 100.0)])
def test_invalid_record(r, field, value):
    from oxylus_amd.renderer import SkyLutContext

    good = AF.small_atmosphere()
    guards = AF.lut_guards(good)
    bad = dataclasses.replace(AF.renderer_atmosphere(good), **{field: value})
    table = torch.from_numpy(AF.hemisphere()).cuda()
    above = {"planet_radius": "planet_radius must be above 0", "atmos_radius": "atmos_radius must be above planet_radius"}
    message = field if "size" in field else above[field] if math.isfinite(value) else "planet_radius and atmos_radius must be finite"
    _refused(lambda: r.generate_sky_luts(SkyLutContext(bad, table, guards[0].tensor, guards[1].tensor)), message, guards)
    ctx = AF.draw_context(good, guards, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    ctx.atmosphere = bad
    _refused(lambda: r.draw_atmosphere(ctx), message, guards)


@pytest.mark.parametrize("field,value,message", [("sky_view_lut_size", (17, 1, 1), "sky_view_lut_size"), ("sky_view_lut_size", (5000, 9, 1), "sky_view_lut_size"),
                                                 ("aerial_perspective_lut_size", (5, 3, 0), "aerial_perspective_lut_size"),
                                                 ("aerial_perspective_lut_size", (0, 3, 2), "aerial_perspective_lut_size"),
                                                 ("aerial_perspective_lut_size", (4097, 1, 1), "every side must be in 1 .. 4096"),
                                                 ("aerial_perspective_lut_size", (1, 4097, 1), "every side must be in 1 .. 4096"),
                                                 ("aerial_perspective_lut_size", (1, 1, 4097), "every side must be in 1 .. 4096"),
                                                 pytest.param("aerial_perspective_lut_size", (4096, 4096, 8), "more than 2^26 texels",
                                                              id="aerial_perspective_lut_size-value7-2\\^26 texels")])  # the id it has had
def test_invalid_draw_sizes(r, field, value, message):
    good = AF.small_atmosphere()
    guards = AF.lut_guards(good)
    ctx = AF.draw_context(good, guards, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    ctx.atmosphere = dataclasses.replace(AF.renderer_atmosphere(good), **{field: value})
    _refused(lambda: r.draw_atmosphere(ctx), message, guards)


def test_invalid_buffers(r):
    """Missing, short, misaligned and overlapping buffers, each named in its message."""
    from oxylus_amd.renderer import SkyLutContext

    A = AF.small_atmosphere()
    guards = AF.lut_guards(A)
    t, m, v, a = (g.tensor for g in guards)
    table = torch.from_numpy(AF.hemisphere()).cuda()
    atm = AF.renderer_atmosphere(A)
    flat = lambda x: x.view(-1)  # noqa: E731
    null, aligned, short = "must not be null", "must be aligned to 8 bytes", "is smaller than its extent"
    for ctx, message in ((SkyLutContext(atm, None, t, m), "hemisphere_directions " + null), (SkyLutContext(atm, table.view(-1)[:190], t, m), "hemisphere_directions " + short),
                         (SkyLutContext(atm, table.view(-1)[1:], t, m), "hemisphere_directions " + aligned), (SkyLutContext(atm, table, flat(t)[:-4], m), "sky_transmittance_lut " + short),
                         (SkyLutContext(atm, table, flat(t)[2:], m), "sky_transmittance_lut " + aligned), (SkyLutContext(atm, table, t, flat(m)[:-1]), "sky_multiscatter_lut " + short),
                         (SkyLutContext(atm, table, t, None), "sky_multiscatter_lut " + null), (SkyLutContext(atm, table, t, t), "must not overlap"),
                         (SkyLutContext(atm, t.view(torch.float32), t, m), "must not overlap hemisphere_directions")):
        _refused(lambda: r.generate_sky_luts(ctx), message, guards)
    base = AF.draw_context(A, guards, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    for change, message in ((dict(sky_transmittance_lut_attachment=None), "sky_transmittance_lut " + null), (dict(sky_multiscatter_lut_attachment=flat(m)[:-4]), "sky_multiscatter_lut " + short),
                            (dict(sky_view_lut_attachment=flat(v)[2:]), "sky_view_lut " + aligned), (dict(sky_view_lut_attachment=flat(v)[:-4]), "sky_view_lut " + short),
                            (dict(sky_aerial_perspective_lut_attachment=flat(a)[:-4]), "sky_aerial_perspective_lut " + short),
                            (dict(sky_aerial_perspective_lut_attachment=None), "sky_aerial_perspective_lut " + null),
                            (dict(sky_view_lut_attachment=t), "sky_view_lut must not overlap sky_transmittance_lut"),
                            (dict(sky_aerial_perspective_lut_attachment=t), "sky_aerial_perspective_lut must not overlap sky_transmittance_lut")):
        _refused(lambda: r.draw_atmosphere(dataclasses.replace(base, **change)), message, guards)
    big = dataclasses.replace(atm, sky_view_lut_size=(4, 3, 1), aerial_perspective_lut_size=(4, 3, 1))  # both outputs fit one window: they share bytes
    _refused(lambda: r.draw_atmosphere(dataclasses.replace(base, atmosphere=big, sky_aerial_perspective_lut_attachment=v)), "must not overlap", guards)


def test_the_first_broken_rule_gives_the_message(r):
    """Two rules broken at once, for every neighbouring pair of the header's order: the earlier one is named."""
    from oxylus_amd.renderer import SkyLutContext

    A = AF.small_atmosphere()
    guards = AF.lut_guards(A)
    t, m, v, a = (g.tensor for g in guards)
    table = torch.from_numpy(AF.hemisphere()).cuda()
    atm = AF.renderer_atmosphere(A)
    flat = lambda x: x.view(-1)  # noqa: E731
    rep = dataclasses.replace
    for ctx, message in (
            (SkyLutContext(rep(atm, transmittance_lut_size=(1, 9, 1), multiscattering_lut_size=(5, 1, 1)), table, t, m), "transmittance_lut_size"),
            (SkyLutContext(rep(atm, multiscattering_lut_size=(5, 1, 1), planet_radius=float("nan")), table, t, m), "multiscattering_lut_size"),
            (SkyLutContext(rep(atm, planet_radius=float("inf"), atmos_radius=1.0), table, t, m), "must be finite"),
            (SkyLutContext(rep(atm, planet_radius=-1.0, atmos_radius=-2.0), table, t, m), "planet_radius must be above 0"),
            (SkyLutContext(rep(atm, atmos_radius=6000.0), None, t, m), "atmos_radius must be above planet_radius"),
            (SkyLutContext(atm, None, None, m), "hemisphere_directions must not be null"),
            (SkyLutContext(atm, table.view(-1)[1:100], t, m), "hemisphere_directions must be aligned"),
            (SkyLutContext(atm, table.view(-1)[:100], flat(t)[2:], m), "hemisphere_directions is smaller"),
            (SkyLutContext(atm, table, flat(t)[2:-4], m), "sky_transmittance_lut must be aligned"),
            (SkyLutContext(atm, table, flat(t)[:-4], None), "sky_transmittance_lut is smaller"),
            (SkyLutContext(atm, table, t.view(-1), flat(t)[2:]), "sky_multiscatter_lut must be aligned"),
            (SkyLutContext(atm, table, t, flat(t)[:8]), "sky_multiscatter_lut is smaller")):
        _refused(lambda: r.generate_sky_luts(ctx), message, guards)
    base = AF.draw_context(A, guards, AF.CAMERAS["ground"], AF.SUNS["30 deg"])
    for change, message in (
            (dict(atmosphere=rep(atm, multiscattering_lut_size=(1, 3, 1), sky_view_lut_size=(1, 9, 1))), "multiscattering_lut_size"),
            (dict(atmosphere=rep(atm, sky_view_lut_size=(1, 9, 1), aerial_perspective_lut_size=(0, 3, 2))), "sky_view_lut_size"),
            (dict(atmosphere=rep(atm, aerial_perspective_lut_size=(4097, 4096, 4096))), "every side must be in 1 .. 4096"),
            (dict(atmosphere=rep(atm, aerial_perspective_lut_size=(4096, 4096, 8), planet_radius=0.0)), "more than 2^26 texels"),
            (dict(atmosphere=rep(atm, planet_radius=0.0), sky_transmittance_lut_attachment=None), "planet_radius must be above 0"),
            (dict(sky_transmittance_lut_attachment=None, sky_multiscatter_lut_attachment=None), "sky_transmittance_lut must not be null"),
            (dict(sky_multiscatter_lut_attachment=flat(m)[:-4], sky_view_lut_attachment=None), "sky_multiscatter_lut is smaller"),
            (dict(sky_view_lut_attachment=flat(v)[2:], sky_aerial_perspective_lut_attachment=None), "sky_view_lut must be aligned"),
            (dict(sky_view_lut_attachment=flat(v)[:-4], sky_aerial_perspective_lut_attachment=t), "sky_view_lut is smaller"),
            (dict(sky_aerial_perspective_lut_attachment=flat(a)[:-4], sky_view_lut_attachment=t), "sky_aerial_perspective_lut is smaller")):
        _refused(lambda: r.draw_atmosphere(rep(base, **change)), message, guards)
