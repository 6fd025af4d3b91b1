"""oxc_generate_terrain_maps on the GPU against tests/terrain_maps_model.py: every byte of the five images equal to the checker's, between
poisoned guard bands, the edit images unchanged (terrain_maps_frames.run)."""
import dataclasses

import numpy as np
import pytest
import torch

import terrain_maps_frames as TF
import terrain_maps_model as TM
from refusals import ALIGNED, NULL, SHORT, raises_refusal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r(renderer):
    return renderer


def _frame(res, pc, strokes=True, **generate):
    G, D = TF.engine(res, **generate)
    he, se = TF.edits(res, strokes=strokes)
    return G, D, TF.initial(res, pc, he, se)


def test_engine_defaults(r):
    res, pc, G, D, images, out, _ = TF.engine_48x40()
    got = TF.run(r, G, D, res, pc, images, "engine defaults")
    for name in TF.OUTPUTS:
        assert (got[name] == out[name]).all()


@pytest.mark.parametrize("res,pc", [((1, 1), (1, 1)), ((2, 2), (3, 2)), ((17, 16), (1, 1)), ((33, 17), (3, 2)), ((65, 31), (3, 2)), ((6, 5), (7, 7)), ((17, 16), (40, 33))])
def test_extents_and_patch_counts(r, res, pc):
    """Odd extents, more than one block per side, and more patches than texels."""
    G, D, images = _frame(res, pc)
    TF.run(r, G, D, res, pc, images, f"{res} / {pc}")


@pytest.mark.parametrize("height_octaves,erosion_octaves", [(0, 0), (0, 5), (3, 0), (1, 1), (5, 1), (1, 5), (16, 2), (2, 16)])
def test_octave_counts(r, height_octaves, erosion_octaves):
    """0, 1, 5 and 16 octaves of each kind; without noise octaves the slope is zero and normalize_safe takes its zero arm."""
    res, pc = (19, 18), (2, 2)
    G, D, images = _frame(res, pc, height_octaves=height_octaves)
    G = TF.with_erosion(G, octaves=erosion_octaves)
    counts = {}
    TF.run(r, G, D, res, pc, images, f"octaves {height_octaves} / {erosion_octaves}", counts=counts)
    if height_octaves == 0 and erosion_octaves:
        assert counts["normalize_safe_zero"] > 0


@pytest.mark.parametrize("stages", [TM.GENERATE, TM.DERIVE, TM.MINMAX, TM.GENERATE | TM.MINMAX, TM.DERIVE | TM.MINMAX])
def test_each_stage_alone(r, stages):
    """A stage alone works on the maps as they are; what the requested stages do not touch is a null buffer and cannot be read."""
    res, pc = (33, 17), (3, 2)
    G, D, images = _frame(res, pc)
    TF.run(r, G, D, res, pc, images, f"stages {stages}")
    TF.run(r, G, D, res, pc, images, f"stages {stages}, the rest null", stages=stages, only_touched=True)


@pytest.mark.parametrize("region,dispatch_texels,dispatch_patches", [
    ((0, 0, 0, 0), (1, 1), (1, 1)),            # a corner: one work group each
    ((5, 3, 1, 0), (1, 1), (1, 1)),            # 16 x 14 texels from (5, 3) on the 33 x 17 map
    ((27, 9, 2, 1), (20, 20), (9, 9)),         # straddling the far edges
    ((33, 17, 3, 2), (16, 16), (8, 8)),        # the origin past the extent: nothing is written
    ((0xFFFFFFF0, 2, 0xFFFFFFFF, 0), (33, 5), (3, 1)),  # origin + index wraps in u32
])
def test_regional_calls(r, region, dispatch_texels, dispatch_patches):
    res, pc = (33, 17), (3, 2)
    G, D, images = _frame(res, pc)
    got = TF.run(r, G, D, res, pc, images, f"region {region}", region=region, dispatch_texels=dispatch_texels, dispatch_patches=dispatch_patches)
    if region[0] >= res[0] and region[0] < 2 ** 31:
        for name in TF.OUTPUTS:
            assert (got[name] == images[name]).all()


def test_dispatch_rounding_is_the_work_group(r):
    """Origin (5, 3), dispatch (1, 1) on 33 x 17: exactly the 16 x 14 texels from (5, 3) change; one patch dispatched on 3 x 2 patches from
    (1, 0): the two patches (1, 0), (2, 0) and (1, 1), (2, 1) of the 8 x 8 group."""
    res, pc = (33, 17), (3, 2)
    G, D, images = _frame(res, pc)
    got = TF.run(r, G, D, res, pc, images, "rounding", region=(5, 3, 1, 0), dispatch_texels=(1, 1), dispatch_patches=(1, 1))
    changed = got["heightmap"] != images["heightmap"]
    ys, xs = np.nonzero(changed)
    assert xs.min() >= 5 and xs.max() <= 20 and ys.min() >= 3 and ys.max() <= 16
    assert changed[3:17, 5:21].mean() > 0.99  # a random u16 equals the written one by chance at most
    assert (got["patch_minmax"][:, 0] == images["patch_minmax"][:, 0]).all() and (got["patch_minmax"][:, 1:] != images["patch_minmax"][:, 1:]).all()


def test_regional_rebake_after_a_full_bake(r):
    """A full bake, a brush stroke into height_edit, then the regional call: derive reads the older heightmap around the region."""
    res, pc = (48, 40), (5, 3)
    G, D, images = _frame(res, pc)
    baked = TF.run(r, G, D, res, pc, images, "bake")
    stroke = baked["height_edit"].copy()
    stroke[10:30, 12:34] += np.float32(0.25)
    after = dict(baked, height_edit=stroke)
    got = TF.run(r, G, D, res, pc, after, "re-bake", region=(14, 11, 1, 0), dispatch_texels=(17, 17), dispatch_patches=(3, 3))
    assert (got["heightmap"] != baked["heightmap"]).any() and (got["heightmap"][0] == baked["heightmap"][0]).all()


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF])
def test_seeds(r, seed):
    """0xFFFFFFFF + i wraps to i - 1; f32(0xFFFFFFFF) rounds up to 2^32."""
    res, pc = (20, 17), (2, 2)
    G, D, images = _frame(res, pc)
    TF.run(r, TF.with_erosion(G, seed=seed), D, res, pc, images, f"seed {seed}")


SPECIAL = (float("nan"), float("inf"), float("-inf"), 1e-41, -0.0)
GENERATE_FLOATS = ("domain_size", "height_frequency", "height_amplitude", "height_lacunarity", "height_gain")
EROSION_FLOATS = ("scale", "strength", "gully_weight", "cell_scale", "gain", "lacunarity", "normalization")
DERIVE_FLOATS = ("height_range", "slope_rock_begin", "slope_rock_end", "altitude_snow_begin", "altitude_snow_end", "ridge_drainage_scale")


@pytest.mark.parametrize("value", SPECIAL)
def test_special_values_in_the_settings(r, value):
    """NaN, Inf, a denormal and -0 in each float setting in turn (erosion.detail has its own limit): the rules say what comes out."""
    res, pc = (17, 6), (2, 1)
    G0, D0, images = _frame(res, pc)
    rep = dataclasses.replace
    cases = [(rep(G0, **{n: value}), D0, n) for n in GENERATE_FLOATS] + [(TF.with_erosion(G0, **{n: value}), D0, "erosion." + n) for n in EROSION_FLOATS]
    cases += [(G0, rep(D0, **{n: value}), "derive." + n) for n in DERIVE_FLOATS]
    for field, width in (("rounding", 4), ("onset", 4), ("assumed_slope", 2)):
        for k in range(width):
            v = list(getattr(G0.erosion, field))
            v[k] = value
            cases.append((TF.with_erosion(G0, **{field: tuple(v)}), D0, f"erosion.{field}[{k}]"))
    for k in range(2):
        ho, tw = list(G0.height_offset), list(D0.texel_world_size)
        ho[k], tw[k] = value, value
        cases += [(rep(G0, height_offset=tuple(ho)), D0, f"height_offset[{k}]"), (G0, rep(D0, texel_world_size=tuple(tw)), f"texel_world_size[{k}]")]
    for G, D, name in cases:
        TF.run(r, G, D, res, pc, images, f"{name} = {value}")


def test_special_values_in_the_edit_images(r):
    res, pc = (17, 6), (2, 1)
    G, D, images = _frame(res, pc)
    he = images["height_edit"].copy()
    he.reshape(-1)[:6] = [np.nan, np.inf, -np.inf, 1e-41, -0.0, 3e38]
    se = images["splat_edit"].copy()
    se.reshape(-1)[:4] = [0xFFFFFFFF, 0xFF000000, 0x80FF00FF, 0x01010101]
    TF.run(r, G, D, res, pc, dict(images, height_edit=he, splat_edit=se), "special edits")


def test_captured_graph(r):
    """Bake -> regional re-bake captured into one graph on one stream, replayed three times with the region buffer rewritten between the
    replays: the region is read on the device at replay time."""
    from gpu_passes import same

    res, pc = (48, 40), (5, 3)
    G, D, images = _frame(res, pc)
    G2 = TF.with_erosion(G, seed=7)  # the re-bake differs from the bake where it writes
    gs = TF.guards(images)
    region = TF.region_tensor((0, 0, 0, 0))
    bake = TF.context(G, D, res, pc, gs)
    rebake = TF.context(G2, D, res, pc, gs, region=region, dispatch_texels=(10, 10), dispatch_patches=(2, 2))
    r.generate_terrain_maps(bake)
    r.generate_terrain_maps(rebake)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        r.generate_terrain_maps(bake, stream=stream)
        r.generate_terrain_maps(rebake, stream=stream)
    baked = TF.want(G, D, res, pc, images)
    for replay, where in enumerate(((3, 2, 0, 0), (30, 25, 3, 1), (47, 39, 4, 2))):
        region.copy_(TF.region_tensor(where))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        expected = TF.want(G2, D, res, pc, baked, region=where, dispatch_texels=(10, 10), dispatch_patches=(2, 2))
        got = TF.got_of(gs, images)
        for name, g in gs.items():
            g.check(f"replay {replay}")
            same(got[name], expected[name], f"replay {replay}: {name}")
        assert (expected["heightmap"] != baked["heightmap"]).any()


# ---- the chain into the terrain cull -----------------------------------------------------------------------------------------------------------
def test_patch_minmax_feeds_the_terrain_cull(r, oracle_lib):
    """The call's patch_minmax handed straight to oxc_cull_terrain: the result equals the oracle cull fed the checker's min / max."""
    import oracle
    from oxylus_amd import lib as L
    from test_terrain import _camera, _mask

    res, pc = (64, 48), (9, 7)
    G, D, images = _frame(res, pc)
    gs = TF.guards(images)
    r.generate_terrain_maps(TF.context(G, D, res, pc, gs))
    torch.cuda.synchronize()
    mm_want = TF.want(G, D, res, pc, images)["patch_minmax"]
    total = pc[0] * pc[1]
    cam = _camera(eye=(0.0, 150.0, 300.0))
    wmin, wsize, base_h, hscale = [-300.0, -500.0], [600.0, 650.0], 0.0, 400.0
    mask_cpu = _mask(total, 7, 1.0)
    mask_gpu = mask_cpu.clone().cuda()
    want = oracle.cull_terrain(wmin, wsize, pc, base_h, hscale, torch.from_numpy(mm_want.copy()), cam, L.CULL_TEST_FRUSTUM, None, mask_cpu)
    got, cmd = r.cull_terrain(L.CULL_TEST_FRUSTUM, cam, wmin, wsize, pc, base_h, hscale, gs["patch_minmax"].tensor, mask_gpu)
    assert cmd == [4, want.numel(), 0, 0]
    assert torch.equal(got.cpu(), want)
    assert 0 < want.numel() < total


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal(r):
    res, pc = (17, 6), (2, 1)
    G, D, images = _frame(res, pc)
    gs = TF.guards(images)
    return res, pc, G, D, images, gs, TF.context(G, D, res, pc, gs, region=TF.region_tensor((0, 0, 0, 0)))


def _refused(r, context, message, gs, images):
    raises_refusal(lambda: r.generate_terrain_maps(context), message)
    got = TF.got_of(gs, images)
    for name, g in gs.items():
        g.check("refused")
        assert (got[name].view(np.uint8) == images[name].view(np.uint8)).all(), f"{name} was written"


def _cases(base, gs):
    """(changes to the context, message) for every limit on its own, in the header's order."""
    rep = dataclasses.replace
    flat = lambda n: gs[n].tensor.view(-1)  # noqa: E731
    half = lambda t: t.view(torch.int16)  # noqa: E731
    cases = [
        (dict(stages=0), "stages must be"), (dict(stages=8), "stages must be"), (dict(stages=15), "stages must be"),
        (dict(resolution=(0, 6)), "resolution: every side"), (dict(resolution=(17, 16385)), "resolution: every side"),
        (dict(patch_count=(0, 1)), "patch_count: every side"), (dict(patch_count=(2, 4097)), "patch_count: every side"),
        (dict(generate=rep(base.generate, resolution=(16, 6))), "generate.resolution must equal"),
        (dict(derive=rep(base.derive, resolution=(17, 7))), "derive.resolution must equal"),
        (dict(generate=rep(base.generate, height_octaves=17)), "height_octaves must be at most 16"),
        (dict(generate=rep(base.generate, erosion=rep(base.generate.erosion, octaves=17))), "erosion.octaves must be at most 16"),
    ]
    for detail in (0.0, -1.0, float("nan"), float("inf")):
        cases.append((dict(generate=rep(base.generate, erosion=rep(base.generate.erosion, detail=detail))), "erosion.detail must be finite and above 0"))
    cases += [(dict(region=base.region[1:]), "region" + ALIGNED), (dict(region=base.region[:2]), "region" + SHORT)]
    for name in ("heightmap", "ridgemap", "normalmap", "splatmap", "height_edit", "splat_edit"):
        cases.append(({name: None}, name + NULL))
        cases.append(({name: half(flat(name))[1:-1] if name != "heightmap" and name != "ridgemap" else flat(name).view(torch.int8)[1:-1]}, name + ALIGNED))
        cases.append(({name: flat(name)[:-2]}, name + SHORT))
    pm = gs["patch_minmax"].tensor
    cases += [(dict(patch_minmax=None), "patch_minmax" + NULL), (dict(patch_minmax=pm.view(-1)[1:-1].view(1, 1, 2)), "patch_minmax" + ALIGNED),
              (dict(patch_minmax=pm[:, :1]), "patch_minmax must be one RG32F level"),
              (dict(ridgemap=gs["heightmap"].tensor), "heightmap must not overlap ridgemap"),
              (dict(splatmap=gs["height_edit"].tensor), "splatmap must not overlap height_edit"),
              (dict(normalmap=gs["splat_edit"].tensor), "normalmap must not overlap splat_edit")]
    return cases


def test_every_limit_on_its_own(r, refusal):
    res, pc, G, D, images, gs, base = refusal
    for change, message in _cases(base, gs):
        _refused(r, dataclasses.replace(base, **change), message, gs, images)


def test_the_first_broken_rule_gives_the_message(r, refusal):
    """Two rules broken at once, for neighbouring pairs of the header's order: the earlier one is named."""
    res, pc, G, D, images, gs, base = refusal
    rep = dataclasses.replace
    bad_detail = rep(base.generate, erosion=rep(base.generate.erosion, detail=0.0))
    for change, message in (
            (dict(stages=0, resolution=(0, 0)), "stages must be"),
            (dict(resolution=(0, 6), patch_count=(0, 0)), "resolution: every side"),
            (dict(patch_count=(0, 1), generate=rep(base.generate, resolution=(1, 1))), "patch_count: every side"),
            (dict(generate=rep(base.generate, resolution=(1, 1)), derive=rep(base.derive, resolution=(1, 1))), "generate.resolution must equal"),
            (dict(derive=rep(base.derive, resolution=(1, 1)), generate=rep(base.generate, height_octaves=99)), "derive.resolution must equal"),
            (dict(generate=rep(base.generate, height_octaves=17, erosion=rep(base.generate.erosion, octaves=17))), "height_octaves must be at most 16"),
            (dict(generate=rep(bad_detail, erosion=rep(bad_detail.erosion, octaves=17))), "erosion.octaves must be at most 16"),
            (dict(generate=bad_detail, heightmap=None), "erosion.detail must be finite"),
            (dict(region=base.region[:2], heightmap=None), "region" + SHORT),
            (dict(heightmap=None, ridgemap=None), "heightmap" + NULL),
            (dict(ridgemap=gs["ridgemap"].tensor.view(-1)[:-2], normalmap=None), "ridgemap" + SHORT),
            (dict(splat_edit=None, patch_minmax=None), "splat_edit" + NULL),
            (dict(patch_minmax=None, ridgemap=gs["heightmap"].tensor), "patch_minmax" + NULL)):
        _refused(r, rep(base, **change), message, gs, images)


def test_null_context_and_short_struct_size(r):
    import ctypes as C

    from oxylus_amd import lib as L

    lib = L.load()
    assert lib.oxc_generate_terrain_maps(r._ctx, None, None) == L.OXC_INVALID_ARG
    assert lib.oxc_generate_terrain_maps(None, None, None) == L.OXC_INVALID_ARG
    c = L.TerrainMapsContext()
    c.struct_size = C.sizeof(L.TerrainMapsContext) - 8
    assert lib.oxc_generate_terrain_maps(r._ctx, C.byref(c), None) == L.OXC_INVALID_ARG
    assert b"struct_size" in lib.oxc_last_error(r._ctx)
