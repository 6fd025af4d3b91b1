"""oxc_apply_terrain_brush on the GPU against tests/terrain_brush_model.py: every byte of hit, region, height_edit and splat_edit equal to
the checker's, between poisoned guard bands, every untouched byte unchanged (terrain_brush_frames.run)."""
import dataclasses

import numpy as np
import pytest
import torch

import terrain_brush_frames as BF
import terrain_brush_model as TB
from refusals import ALIGNED, NULL, SHORT, raises_refusal

pytestmark = pytest.mark.gpu
RES, PC = (24, 20), (3, 5)
rep = dataclasses.replace
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def r(renderer):
    return renderer


def _params(origin, direction, res=RES, pc=PC, **kw):
    kw.setdefault("radius_texels", 2.5)
    kw.setdefault("strength", 0.5)
    return BF.params(res, pc, origin, direction, **kw)


# ---- the trace -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 255, 256, 257, 511, 512])
def test_crossings_at_the_seams_of_the_lane_mapping(r, step):
    info = {}
    got = BF.run(r, _params(*BF.ray_crossing_at_step(step)), BF.initial(RES, "flat"), f"step {step}", info=info)
    assert info["step"] == step and got["hit"][3] == 1


def test_two_crossings_the_first_wins(r):
    """A ray that falls through the ridge, leaves it on the far side and then meets the ground."""
    info = {}
    B = _params((-500.0, 300.0, 0.0), (1.0, -0.27, 0.0))
    got = BF.run(r, B, BF.initial(RES, "ridge"), "ridge", info=info)
    g = info["gaps"]
    crossings = np.flatnonzero((g[1:] <= 0) & (g[:-1] > 0)) + 1
    assert len(crossings) == 2 and info["step"] == crossings[0] and got["hit"][3] == 1


def test_a_gap_of_exactly_zero(r):
    """A vertical ray has the span (0, 1e9) and steps of exactly 1953125; from y = 3 steps above the zero map gap_3 is 0.0."""
    info = {}
    BF.run(r, _params((3.0, 5859375.0, 7.0), (0.0, -1.0, 0.0)), BF.initial(RES, "zero"), "zero gap", info=info)
    assert info["step"] == 3 and info["gaps"][3] == 0 and info["gaps"][2] > 0


@pytest.mark.parametrize("name,origin,direction,count", [
    ("under the ground", (0.0, -50.0, 0.0), (0.3, -1.0, 0.1), "miss_no_crossing"),
    ("pointing at the sky", (0.0, 500.0, 0.0), (0.3, 1.0, 0.1), "miss_no_crossing"),
    ("outside the footprint", (-900.0, 500.0, -900.0), (-1.0, -1.0, 0.5), "miss_clip"),
    ("parallel and outside", (0.0, 500.0, 900.0), (1.0, -1.0, 0.0), "miss_parallel"),
])
def test_misses_write_zeros_over_the_poison(r, name, origin, direction, count):
    counts = {}
    images = BF.initial(RES, "ramp")
    got = BF.run(r, _params(origin, direction), images, name, counts=counts)
    assert counts.get(count) == 1 and (got["hit"] == 0).all() and (got["region"] == 0).all()
    assert (got["height_edit"] == images["height_edit"]).all()


def test_special_values_in_the_ray(r):
    """A zero direction, NaN and Inf in every ray component, a zero world_size (inv_world_size Inf, as 1 / 0 gives)."""
    images = BF.initial(RES, "ramp")
    base = _params((-300.0, 420.0, -150.0), (0.6, -0.7, 0.35))
    cases = [("zero direction", rep(base, ray_direction=(0.0, 0.0, 0.0))),
             ("zero world_size", rep(base, world_size=(0.0, 0.0), inv_world_size=(INF, INF))),
             ("zero world_size.x", rep(base, world_size=(0.0, 1024.0), inv_world_size=(INF, base.inv_world_size[1])))]
    for value in (NAN, INF, -INF):
        for field in ("ray_origin", "ray_direction"):
            for k in range(3):
                v = list(getattr(base, field))
                v[k] = value
                cases.append((f"{field}[{k}] = {value}", rep(base, **{field: tuple(v)})))
    for name, B in cases:
        BF.run(r, B, images, name)


@pytest.mark.parametrize("kind,res,pc", [("pit", (1, 1), (1, 1)), ("ramp", (2, 2), (1, 1)), ("pit", (65, 31), (3, 2)), ("random", (65, 31), (7, 3))])
def test_other_extents(r, kind, res, pc):
    for mode in (TB.SMOOTH, TB.PAINT_LAYER):
        B = _params((-20.0, 450.0, 30.0), (0.05, -1.0, -0.07), res, pc, radius_texels=3.5, mode=mode, layer=1)
        got = BF.run(r, B, BF.initial(res, kind), f"{res} {mode}")
        assert got["hit"][3] == 1


# ---- the apply -------------------------------------------------------------------------------------------------------------------------------------
SPOTS = [(0, 0), (23, 0), (0, 19), (23, 19), (12, 0), (12, 19), (0, 10), (23, 10), (12, 10)]


@pytest.mark.parametrize("radius", [0.0, 0.5, 1.0, 2.5, 7.5, 8.0, 16.0])
def test_radii_at_every_corner_edge_and_the_middle(r, radius):
    """Footprints of 1 to 3 groups a side, clipped by every side of the map."""
    images = BF.initial(RES, "ramp")
    counts = {}
    for spot in SPOTS:
        B = _params(*BF.ray_down_at(spot, RES), radius_texels=radius)
        got = BF.run(r, B, images, f"radius {radius} at {spot}", counts=counts)
        assert got["hit"][3] == 1
    assert TB.footprint_threads(radius) // 16 == (1 if radius <= 2.5 else 2 if radius <= 8 else 3)
    assert (counts["texels_written"] > 0) == (radius > 0) and counts["texels_outside"] > 0


@pytest.mark.parametrize("mode", range(5))
def test_modes_with_both_signs_of_strength(r, mode):
    images = BF.initial(RES, "pit")
    for strength in (0.4, -0.4, 5.0, -5.0):  # the large ones saturate height_edit at +-1 and the painted weight at 1
        B = _params(*BF.ray_down_at((11, 9), RES), radius_texels=6.0, mode=mode, layer=2, strength=strength, flatten_height_world=300.0)
        got = BF.run(r, B, images, f"mode {mode} strength {strength}")
        if mode == TB.RAISE and abs(strength) == 5.0:
            assert (got["height_edit"] == np.sign(strength)).any()
        changed = (got["splat_edit"] != images["splat_edit"]).any() if mode == TB.PAINT_LAYER else (got["height_edit"] != images["height_edit"]).any()
        assert changed or (mode == TB.PAINT_LAYER and strength < 0)


@pytest.mark.parametrize("layer", range(5))
def test_paint_layers(r, layer):
    images = BF.initial(RES, "ramp")
    for strength in (0.3, 1.0, 2.5):
        BF.run(r, _params(*BF.ray_down_at((5, 15), RES), radius_texels=4.0, mode=TB.PAINT_LAYER, layer=layer, strength=strength), images, f"layer {layer} x {strength}")


def test_nan_strength_and_flatten_height(r):
    images = BF.initial(RES, "ramp")
    for mode in range(5):
        B = _params(*BF.ray_down_at((11, 9), RES), radius_texels=3.0, mode=mode, layer=1)
        BF.run(r, rep(B, strength=NAN), images, f"NaN strength, mode {mode}")
        BF.run(r, rep(B, strength=INF), images, f"Inf strength, mode {mode}")
    BF.run(r, rep(_params(*BF.ray_down_at((11, 9), RES), mode=TB.FLATTEN), flatten_height=NAN), images, "NaN flatten_height")


@pytest.mark.parametrize("falloff", [1e-3, 1.0, 8.0, 1e-4, 0.0, -3.0])
def test_falloff_exponents(r, falloff):
    images = BF.initial(RES, "ramp")
    BF.run(r, _params(*BF.ray_down_at((11, 9), RES), radius_texels=5.0, falloff=falloff), images, f"falloff {falloff}")


# ---- stages and buffers ----------------------------------------------------------------------------------------------------------------------------
def test_stages_alone_and_together(r):
    images = BF.initial(RES, "ramp")
    B = _params((-300.0, 420.0, -150.0), (0.6, -0.7, 0.35), mode=TB.FLATTEN, flatten_height_world=350.0)
    traced = BF.run(r, B, images, "trace only", stages=TB.TRACE)
    assert traced["hit"][3] == 1 and (traced["height_edit"] == images["height_edit"]).all()
    applied = BF.run(r, B, traced, "apply only on the earlier hit", stages=TB.APPLY)
    both = BF.run(r, B, images, "both")
    assert (applied["height_edit"] == both["height_edit"]).all() and (both["height_edit"] != images["height_edit"]).any()
    invalid = dict(images, hit=np.array([1, 2, 3, 0], np.uint32))
    untouched = BF.run(r, B, invalid, "apply only on an invalid hit", stages=TB.APPLY)
    assert (untouched["height_edit"] == images["height_edit"]).all()


@pytest.mark.parametrize("stages", [TB.TRACE, TB.APPLY, TB.BOTH])
@pytest.mark.parametrize("mode", [TB.SMOOTH, TB.PAINT_LAYER])
def test_unread_buffers_may_be_null(r, stages, mode):
    """What the requested stages do not touch is a null buffer and cannot be read; bound and poisoned it stays as it was."""
    images = BF.initial(RES, "ramp")
    images["hit"] = BF.want(_params(*BF.ray_down_at((7, 7), RES)), images, TB.TRACE)["hit"]
    B = _params(*BF.ray_down_at((7, 7), RES), mode=mode, layer=3)
    BF.run(r, B, images, f"stages {stages} mode {mode}, the rest null", stages=stages, only_touched=True)
    poisoned = dict(images)
    for name in BF.IMAGES:
        if name not in BF.touched(stages, mode):
            poisoned[name] = np.full_like(images[name], 0xABCD if images[name].dtype == np.uint16 else 0x7FC12345 if images[name].dtype == np.uint32 else np.nan)
    BF.run(r, B, poisoned, f"stages {stages} mode {mode}, the rest poisoned", stages=stages)


# ---- the editing loop in one graph -----------------------------------------------------------------------------------------------------------------
def test_edit_loop_in_captured_graphs(r):
    """trace -> apply -> regional generate / derive / minmax on 48 x 40, the region being the record the trace wrote, with the reference's
    dispatch sizes (Passes/Terrain.cpp:147-156).  The ray is part of the params, which the call takes by value: each of three rays gets its
    own capture, and the three graphs are replayed one after the other on the same images, so each stroke lands on the one before.  Compared
    with the two checkers chained; patch_minmax then goes to oxc_cull_terrain."""
    import terrain_maps_frames as TF
    import terrain_maps_model as TM
    from gpu_passes import same
    from oxylus_amd import lib as L
    from test_terrain import _camera, _mask

    res, pc = (48, 40), (5, 3)
    G, D = TF.engine(res)
    he, se = TF.edits(res)
    images = TF.initial(res, pc, he, se)
    gs = TF.guards(images)
    records = BF.guards({"hit": np.zeros(4, np.uint32), "region": np.zeros(4, np.uint32)}, ("hit", "region"))
    r.generate_terrain_maps(TF.context(G, D, res, pc, gs))  # the bake
    torch.cuda.synchronize()
    state = TF.want(G, D, res, pc, images)
    radius = 5.0
    derive_texels = 2 * int(np.ceil(np.float32(radius) + np.float32(1.0))) + 1
    patch_texels = min(np.float32(res[0]) / np.float32(pc[0]), np.float32(res[1]) / np.float32(pc[1]))
    derive_patches = int(np.ceil(np.float32(derive_texels) / patch_texels)) + 1
    rebake = TF.context(G, D, res, pc, gs, region=records["region"].tensor, dispatch_texels=(derive_texels,) * 2, dispatch_patches=(derive_patches,) * 2)
    rays = [((-200.0, 450.0, -100.0), (0.2, -1.0, 0.1), TB.RAISE), ((300.0, 500.0, 350.0), (0.1, -1.0, 0.05), TB.SMOOTH), ((-600.0, 430.0, 20.0), (1.0, -0.3, 0.0), TB.PAINT_LAYER)]
    stream = torch.cuda.Stream()
    graphs = []
    for k, (origin, direction, mode) in enumerate(rays):
        B = BF.params(res, pc, origin, direction, mode=mode, layer=2, radius_texels=radius, strength=0.6 if mode != TB.RAISE else 0.2)
        brush = BF.context(B, {"heightmap": gs["heightmap"], "height_edit": gs["height_edit"], "splat_edit": gs["splat_edit"], **records})
        if k == 0:  # both kernels eagerly once before any capture: the hit record is still invalid, so the apply writes nothing
            r.apply_terrain_brush(rep(brush, stages=TB.APPLY))
            r.apply_terrain_brush(rep(brush, stages=TB.TRACE))
            torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            r.apply_terrain_brush(brush, stream=stream)
            r.generate_terrain_maps(rebake, stream=stream)
        graphs.append((graph, B))
    for replay, (graph, B) in enumerate(graphs):
        graph.replay()
        torch.cuda.synchronize()
        brushed = BF.want(B, {"heightmap": state["heightmap"], "height_edit": state["height_edit"], "splat_edit": state["splat_edit"], "hit": np.zeros(4, np.uint32),
                              "region": np.zeros(4, np.uint32)})
        assert brushed["hit"][3] == 1
        state = dict(state, height_edit=brushed["height_edit"], splat_edit=brushed["splat_edit"])
        state = TF.want(G, D, res, pc, state, region=tuple(int(v) for v in brushed["region"]), dispatch_texels=(derive_texels,) * 2, dispatch_patches=(derive_patches,) * 2)
        got = TF.got_of(gs, images)
        for name, g in gs.items():
            g.check(f"replay {replay}")
            same(got[name], state[name], f"replay {replay}: {name}")
        rec = BF.got_of(records, brushed)
        for name, g in records.items():
            g.check(f"replay {replay}")
            same(rec[name], brushed[name], f"replay {replay}: {name}")
    assert (state["height_edit"] != he).any() and (state["splat_edit"] != se).any()
    total = pc[0] * pc[1]
    mask = _mask(total, 7, 1.0).cuda()
    _, cmd = r.cull_terrain(L.CULL_TEST_FRUSTUM, _camera(eye=(0.0, 150.0, 300.0)), [-300.0, -500.0], [600.0, 650.0], pc, 0.0, 400.0, gs["patch_minmax"].tensor, mask)
    assert cmd[0] == 4 and 0 <= cmd[1] <= total
    assert TM.ALL == 7


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal(r):
    images = BF.initial(RES, "ramp")
    gs = BF.guards(images)
    return images, gs, BF.context(_params(*BF.ray_down_at((7, 7), RES)), gs)


def _refused(r, context, message, gs, images):
    raises_refusal(lambda: r.apply_terrain_brush(context), message)
    got = BF.got_of(gs, images)
    for name, g in gs.items():
        g.check("refused")
        assert (got[name].view(np.uint8) == images[name].view(np.uint8)).all(), f"{name} was written"


def _with(base, **params):
    return rep(base, params=rep(base.params, **params))


def _cases(base, gs):
    """(context, message) for every limit on its own, in the header's order."""
    flat = lambda n: gs[n].tensor.view(-1)  # noqa: E731
    paint = _with(base, mode=TB.PAINT_LAYER)
    cases = [(rep(base, stages=0), "stages must be"), (rep(base, stages=4), "stages must be"), (rep(base, stages=7), "stages must be"),
             (_with(base, resolution=(0, 20)), "resolution: every side"), (_with(base, resolution=(24, 16385)), "resolution: every side"),
             (_with(base, patch_count=(0, 1)), "patch_count: every side"), (_with(base, patch_count=(3, 4097)), "patch_count: every side"),
             (_with(base, mode=5), "mode must be in 0 .. 4"), (_with(base, mode=0xFFFFFFFF), "mode must be in 0 .. 4")]
    cases += [(_with(base, radius_texels=v), "radius_texels must be finite and in 0 .. 4096") for v in (-0.5, 4096.5, NAN, INF)]
    cases += [(_with(base, falloff=v), "falloff must be finite") for v in (NAN, INF, -INF)]
    for name, ctx in (("heightmap", base), ("height_edit", base), ("splat_edit", paint)):
        cases.append((rep(ctx, **{name: None}), name + NULL))
        cases.append((rep(ctx, **{name: flat(name).view(torch.int8)[1:-1]}), name + ALIGNED))
        cases.append((rep(ctx, **{name: flat(name)[:-2]}), name + SHORT))
    for name in ("hit", "region"):
        cases += [(rep(base, **{name: None}), name + NULL), (rep(base, **{name: flat(name)[1:]}), name + ALIGNED), (rep(base, **{name: flat(name)[:2]}), name + SHORT)]
    cases += [(rep(base, region=gs["hit"].tensor), "hit must not overlap region"),
              (rep(base, hit=gs["height_edit"].tensor.view(-1)[1:5]), "height_edit must not overlap hit"),  # the window starts 4 bytes before a multiple of 8
              (rep(paint, region=gs["splat_edit"].tensor.view(-1)[1:5]), "splat_edit must not overlap region")]
    return cases


def test_every_limit_on_its_own(r, refusal):
    images, gs, base = refusal
    for context, message in _cases(base, gs):
        _refused(r, context, message, gs, images)
    BF.run(r, _params(*BF.ray_down_at((7, 7), RES)), images, "the context still works")


def test_the_first_broken_rule_gives_the_message(r, refusal):
    """Two rules broken at once, for neighbouring pairs of the header's order: the earlier one is named."""
    images, gs, base = refusal
    for context, message in (
            (rep(_with(base, resolution=(0, 0)), stages=0), "stages must be"),
            (_with(base, resolution=(0, 20), patch_count=(0, 0)), "resolution: every side"),
            (_with(base, patch_count=(0, 1), mode=9), "patch_count: every side"),
            (_with(base, mode=9, radius_texels=NAN), "mode must be in"),
            (_with(base, radius_texels=-1.0, falloff=NAN), "radius_texels must be finite"),
            (rep(_with(base, falloff=INF), heightmap=None), "falloff must be finite"),
            (rep(base, heightmap=None, height_edit=None), "heightmap" + NULL),
            (rep(base, height_edit=gs["height_edit"].tensor.view(-1)[:-2], hit=None), "height_edit" + SHORT),
            (rep(base, hit=None, region=None), "hit" + NULL),
            (rep(base, region=gs["region"].tensor[:2], hit=gs["height_edit"].tensor.view(-1)[1:5]), "region" + SHORT)):
        _refused(r, context, message, gs, images)
    BF.run(r, _params(*BF.ray_down_at((7, 7), RES)), images, "the context still works")


def test_null_context_and_short_struct_size(r):
    import ctypes as C

    from oxylus_amd import lib as L

    lib = L.load()
    assert lib.oxc_apply_terrain_brush(r._ctx, None, None) == L.OXC_INVALID_ARG
    assert lib.oxc_apply_terrain_brush(None, None, None) == L.OXC_INVALID_ARG
    c = L.TerrainBrushContext()
    c.struct_size = C.sizeof(L.TerrainBrushContext) - 8
    assert lib.oxc_apply_terrain_brush(r._ctx, C.byref(c), None) == L.OXC_INVALID_ARG
    assert b"struct_size" in lib.oxc_last_error(r._ctx)
