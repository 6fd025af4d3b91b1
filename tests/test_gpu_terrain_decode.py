"""oxc_decode_terrain on the GPU against tests/terrain_decode_model.py: every word of the four G-buffer images equal to the checker's between
poisoned guard bands, every pixel that is not terrain keeping its earlier bytes (terrain_decode_frames.run)."""
import dataclasses

import numpy as np
import pytest
import torch

import terrain_decode_frames as DF
import terrain_decode_model as TD
from refusals import ALIGNED, NULL, SHORT, Raw, raises_refusal

pytestmark = pytest.mark.gpu
rep = dataclasses.replace
NAN, INF = float("nan"), float("inf")
INVALID = TD.INVALID_LAYER
H_DENORMAL, H_NAN, H_INF, H_NEG_INF = 0x0001, 0x7E01, 0x7C00, 0xFC00


@pytest.fixture(scope="module")
def r(renderer):
    return renderer


# ---- extents, maps, pixel classes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", DF.EXTENTS)
def test_extents_over_the_baked_map(r, extent):
    counts = {}
    DF.run(r, DF.frame(extent, T=DF.terrain(brush_radius=400.0), hit=DF.hit_record((-100.0, 100.0, 60.0))), f"{extent}", counts)
    assert counts["pixels_terrain"] > 0 and counts["ring_on"] == 1


@pytest.mark.parametrize("name,maps", [
    ("1x1", DF.hand_maps((1, 1), np.array([0.3, -0.2], np.float32), 0x40FF8020)),
    ("2x2", {**DF.hand_maps((2, 2), np.zeros(2, np.float32), 0), "normalmap": DF.half_bits(np.array([[[0.1, 0.2], [-0.3, 0.4]], [[0.5, -0.6], [0.0, 0.0]]], np.float32)),
             "splatmap": np.array([[0x000000FF, 0x0000FF00], [0x00FF0000, 0xFF000000]], np.uint32)}),
    ("24x20", None)])
def test_maps_seen_past_every_edge(r, name, maps):
    """The view spans about +-660 world units over a map that ends at +-512: the clamp runs on all four sides."""
    f = DF.frame((33, 19), maps=maps, pattern="all")
    pre = {}
    DF.want(f, pre=pre)
    wx, _, wz = pre["world"]
    assert wx.min() < -520 and wx.max() > 520 and wz.min() < -520 and wz.max() > 520
    DF.run(r, f, name)


@pytest.mark.parametrize("pattern", ["all", "none", "checker", "mixed"])
def test_pixel_classes(r, pattern):
    """Mesh texels and ~0u keep their earlier bytes; a terrain texel over depth bits 0 is decoded by the rule."""
    counts = {}
    f = DF.frame((17, 9), pattern=pattern)
    DF.run(r, f, pattern, counts)
    assert (counts["pixels_terrain"] == 0) == (pattern == "none") and (counts["pixels_not_terrain"] == 0) == (pattern == "all")
    if pattern == "mixed":
        assert ((f.inputs["depth"].view(np.uint32) == 0) & TD.is_terrain(f.inputs["vis"])).any()


# ---- layers and materials ------------------------------------------------------------------------------------------------------------------------
LAYER_CASES = [("four valid", (0, 1, 2, 3)), ("dark and bright", (4, 4, 3, 3))]
LAYER_CASES += [(f"slot {k} invalid", tuple(INVALID if i == k else i for i in range(4))) for k in range(4)]
LAYER_CASES += [(f"slot {k} out of range", tuple(5 + k if i == k else i for i in range(4))) for k in range(4)]
LAYER_CASES += [("all invalid", (INVALID,) * 4), ("far out of range", (0xFFFFFFFE, 0x80000000, 5, 0x7FFFFFFF))]


@pytest.mark.parametrize("name,layers", LAYER_CASES)
def test_layer_indices(r, name, layers):
    """On the baked map every one of the four splat channels has a positive weight at some terrain pixel of the 33 x 19 frame (asserted
    through the count of not-skipped pixels below), so every slot's kind is reached."""
    counts = {}
    DF.run(r, DF.frame((33, 19), T=DF.terrain(layers), pattern="all"), name, counts)
    for k, index in enumerate(layers):
        kind = "invalid" if index == INVALID else "out_of_range" if index >= 5 else "valid"
        assert counts[f"layer{k}_{kind}"] > 0 and counts[f"layer{k}_skipped"] > 0, (name, k, counts)


def test_no_materials_and_a_null_buffer(r):
    DF.run(r, DF.frame((17, 9), factors=None), "material_count 0, null buffer")
    DF.run(r, DF.frame((7, 5), factors=None, T=DF.terrain((INVALID, 0, INVALID, 1))), "material_count 0, mixed slots")


@pytest.mark.parametrize("half", [H_DENORMAL, 0x83FF, H_NAN, 0xFE00, H_INF, H_NEG_INF])
def test_denormal_nan_inf_in_every_factor(r, half):
    """Each of the nine factors of the material every layer uses is the special half in turn; the other factors stay ordinary."""
    base = DF.half_bits(np.array(DF.MATERIAL_FACTORS[3], np.float32)).astype(np.int64)
    rows = []
    for k in range(9):
        row = base.copy()
        row[k] = half
        rows.append(row)
    for k in range(0, 9, 3):  # three materials a call, on three layer slots
        DF.run(r, DF.frame((7, 5), T=DF.terrain((0, 1, 2, 1)), factors=tuple(rows[k:k + 3]), pattern="all"), f"half 0x{half:04X} in factors {k} .. {k + 2}")


@pytest.mark.parametrize("word", [0x00000000, 0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000, 0xFFFFFFFF, 0x00000001])
def test_splat_texels(r, word):
    counts = {}
    DF.run(r, DF.frame((7, 5), maps=DF.flat_maps((2, 2), word), pattern="all"), f"splat 0x{word:08X}", counts)
    assert (counts.get("weight_sum_default", 0) > 0) == (word == 0)


@pytest.mark.parametrize("name,normals", [
    ("dot above 1", np.array([0.9, 0.8], np.float32)), ("dot exactly 1", np.array([1.0, 0.0], np.float32)), ("large", np.array([300.0, -200.0], np.float32)),
    ("NaN x", np.array([H_NAN, 0x3000], np.uint16)), ("NaN y", np.array([0x3000, 0xFE00], np.uint16)), ("Inf", np.array([H_INF, H_NEG_INF], np.uint16)),
    ("denormal", np.array([0x0001, 0x83FF], np.uint16))])
def test_normal_map_halves(r, name, normals):
    """One special texel among ordinary ones on a 2 x 2 map, so the bilinear blends it with finite values."""
    maps = DF.hand_maps((2, 2), np.array([0.2, 0.1], np.float32), 0x10204080)
    maps["normalmap"][0, 1] = normals if normals.dtype == np.uint16 else DF.half_bits(normals)
    DF.run(r, DF.frame((17, 9), maps=maps, pattern="all"), name)


# ---- the ring ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.0, -5.0, NAN, -INF])
@pytest.mark.parametrize("hit", [None, DF.POISONED_HIT])
def test_no_ring_without_a_positive_radius(r, radius, hit):
    counts = {}
    DF.run(r, DF.frame((7, 5), T=DF.terrain(brush_radius=radius), hit=hit), f"radius {radius}", counts)
    assert counts["ring_off"] == 1


def test_an_invalid_hit_draws_no_ring(r):
    counts = {}
    DF.run(r, DF.frame((17, 9), T=DF.terrain(brush_radius=300.0), hit=DF.hit_record((0.0, 0.0, 0.0), valid=0)), "invalid hit", counts)
    assert counts["ring_invalid_hit"] == 1


@pytest.mark.parametrize("name,position,radius", [
    ("inside the view, wide ring", (-50.0, 150.0, 30.0), 3000.0 / 8), ("inside, ring_width at its floor", (10.0, 150.0, -20.0), 2.0),
    ("inside, the last radius whose ring_width is the floor", (10.0, 150.0, -20.0), 2.5), ("inside, ring_width just above its floor", (10.0, 150.0, -20.0), 2.5000002), ("at the view's edge", (655.0, 100.0, 0.0), 300.0),
    ("outside the view", (5000.0, 0.0, 5000.0), 100.0), ("outside, the ring crossing the view", (2000.0, 0.0, 0.0), 2000.0),
    ("infinite radius", (0.0, 0.0, 0.0), INF), ("NaN hit position", (NAN, 0.0, NAN), 100.0), ("valid is any non-zero word", (0.0, 0.0, 0.0), 500.0)])
def test_ring(r, name, position, radius):
    counts = {}
    valid = 0x80000000 if name.startswith("valid") else 1
    DF.run(r, DF.frame((33, 19), T=DF.terrain(brush_radius=radius), hit=DF.hit_record(position, valid), pattern="all"), name, counts)
    assert counts["ring_on"] == 1
    if name in ("inside the view, wide ring", "outside, the ring crossing the view", "infinite radius", "valid is any non-zero word"):
        assert counts["ring_pixels_touched"] > 0


# ---- non-finite settings ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_nan_inf_in_the_matrix_and_the_world_fields(r, value):
    f = DF.frame((17, 9), T=DF.terrain(brush_radius=400.0), hit=DF.hit_record((0.0, 0.0, 0.0)))
    for k in (0, 5, 10, 14, 15, 3):
        ipv = f.ipv.copy()
        ipv[k] = value
        DF.run(r, rep(f, ipv=ipv), f"inv_projection_view[{k}] = {value}")
    for field in ("world_min", "inv_world_size"):
        for k in range(2):
            v = list(getattr(f.T, field))
            v[k] = value
            DF.run(r, rep(f, T=rep(f.T, **{field: tuple(v)})), f"{field}[{k}] = {value}")


def test_capturable_and_replayed(r):
    """The call in a captured graph, replayed over re-poisoned outputs: the replay's bytes equal the checker's."""
    from gpu_passes import same

    f = DF.golden_frame()
    gs = DF.guards(f)
    c = DF.context(f, gs)
    r.decode_terrain(c)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        r.decode_terrain(c, stream=stream)
    for _ in range(2):
        for name in DF.OUTPUTS:
            a = f.init[name]
            gs[name].tensor.copy_(torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.int32).copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        same(DF.got_of(gs, f), DF.want(f), "replay")
        for g in gs.values():
            g.check("replay")


# ---- the frame chain -----------------------------------------------------------------------------------------------------------------------------
def test_the_frame_chain_in_one_graph_then_eagerly(r):
    """oxc_generate_terrain_maps -> oxc_apply_terrain_brush (trace) -> oxc_decode_visbuffer(clear) -> oxc_decode_terrain -> oxc_apply_pbr on
    one set of attachments, captured in one graph and replayed, then run eagerly, both against the checkers chained.  The mesh pixels are
    main_scene drawn by oxc_draw_visbuffer.  The pixels it left uncovered become terrain: their texels and depth come from the CPU stand-in
    for the terrain draw over the checker's 48 x 40 heightmap, seen by the camera above the map, whose matrix the terrain decode and the
    lighting use; every 17th of them stays empty.  The decode reads the device's normal map, splat map and hit record as their producers
    wrote them inside the same graph.  The terrain pixels come out lit, not black."""
    import gpu_passes as GP
    import terrain_brush_frames as BF
    import terrain_brush_model as TB
    import terrain_maps_frames as TF
    from gpu_passes import same
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import PBRContext, TerrainDecodeContext
    from pixel_rules import unpack_b10g11r11
    from scenes import main_scene
    from test_gpu_visbuffer_decode import draw

    W, H = 96, 64
    cpu, _ = main_scene()
    gpu, vis_t, depth_t, _, _ = draw(r, cpu, W, H)
    frame_of_scene = r.prepared_frame
    res, pc, G, D, images, maps_want, _ = TF.engine_48x40()
    T = DF.terrain((0, 1, 2, INVALID), brush_radius=300.0)
    pv, ipv = DF.camera(W, H)
    tvis, tdepth = DF.draw(T, maps_want["heightmap"], W, H, pv, ipv)
    vis, depth = vis_t.cpu().numpy().view(np.uint32).copy(), depth_t.cpu().numpy().copy()
    ground = (depth.view(np.uint32) == 0) & ((np.arange(W * H).reshape(H, W) % 17) != 0)
    assert 0.2 < ground.mean() < 0.9 and (depth != 0).mean() > 0.1  # both mesh and terrain pixels
    vis[ground], depth[ground] = tvis[ground], tdepth[ground]
    vis_t.copy_(torch.from_numpy(vis.view(np.int32)).cuda())
    depth_t.copy_(torch.from_numpy(depth).cuda())

    gs = TF.guards(images)
    maps_ctx = TF.context(G, D, res, pc, gs)
    B = BF.params(res, pc, (-200.0, 450.0, -100.0), (0.2, -1.0, 0.1), radius_texels=5.0)
    records = BF.guards({"hit": np.zeros(4, np.uint32), "region": np.zeros(4, np.uint32)}, ("hit", "region"))
    brush = BF.context(B, {"heightmap": gs["heightmap"], **records}, stages=TB.TRACE)
    dctx = GP.decode_context(gpu, vis_t, depth_t, cpu.camera["projection_view"])
    tctx = TerrainDecodeContext.over(dctx, maps_ctx, ipv, DF.renderer_terrain(T), records["hit"].tensor)
    assert tctx.map_resolution == res and tctx.normalmap is maps_ctx.normalmap and tctx.albedo_attachment is dctx.albedo_attachment
    ones = torch.ones((H, W), dtype=torch.float32, device="cuda")
    pctx = PBRContext.create(depth_t, dctx.albedo_attachment, dctx.normal_attachment, dctx.emissive_attachment, dctx.metallic_roughness_occlusion_attachment,
                             ones.to(torch.float16).view(torch.int16), ones, None, L.SCENE_HAS_DIRECTIONAL_LIGHT | L.SCENE_HAS_SKY, ipv, (0.0, DF.CAMERA_HEIGHT, 0.0),
                             (0.3, 0.8, 0.5), 3.0, sky_solid_color=(0.25, 0.5, 1.0, 1.0), sky_ambient_color=(0.1, 0.15, 0.2))
    outputs = (gs["normalmap"].tensor, gs["splatmap"].tensor, records["hit"].tensor, dctx.albedo_attachment, dctx.normal_attachment, dctx.emissive_attachment,
               dctx.metallic_roughness_occlusion_attachment, pctx.final_attachment)

    def chain(stream=None):
        r.generate_terrain_maps(maps_ctx, stream=stream)
        r.apply_terrain_brush(brush, stream=stream)
        r.prepared_frame = frame_of_scene
        r.decode_visbuffer(dctx, stream=stream)
        r.decode_terrain(tctx, stream=stream)
        r.apply_pbr(pctx, stream=stream)

    # the checkers chained
    hit_want, _ = TB.trace(B, maps_want["heightmap"])
    assert hit_want[3] == 1
    mesh_want = GP.decode_want_of(dctx, cpu)
    counts = {}
    gbuffer_want = TD.decode(T, vis, depth, ipv, maps_want["normalmap"], maps_want["splatmap"], gpu.materials.cpu().numpy(), dctx.material_count, hit_want, mesh_want, counts)
    assert counts["pixels_terrain"] == ground.sum() and counts["ring_on"] == 1 and counts["layer3_invalid"] > 0
    assert all((mesh_want[k][ground] == 0).all() for k in TD.IMAGES) and (gbuffer_want["mro"][ground] != 0).all()  # the hole, and the hole filled

    def check(label):
        torch.cuda.synchronize()
        same(TF.got_of(gs, images), maps_want, f"{label}: maps")
        same(BF.got_of(records, {"hit": hit_want, "region": hit_want})["hit"], hit_want, f"{label}: hit")
        same(GP.decode_got_of(dctx), gbuffer_want, f"{label}: G-buffer")
        final = GP.pbr_got_of(pctx)
        same(final, GP.pbr_want_of(pctx), f"{label}: lit image")  # the checker on the G-buffer just shown equal to the chained one
        lit = np.stack(unpack_b10g11r11(final[ground]), axis=-1)
        assert np.isfinite(lit).all() and (lit.sum(-1) > 0).all(), f"{label}: {int((lit.sum(-1) <= 0).sum())} terrain pixels are black"

    def poison():
        for t in outputs:
            t.fill_(-5)

    chain()  # eagerly once before the capture
    check("first eager run")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        chain(stream)
    for replay in range(2):
        poison()
        graph.replay()
        check(f"replay {replay}")
    poison()
    chain()
    check("eager run after the replays")
    for g in list(gs.values()) + list(records.values()):
        g.check("chain")


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
BUFFERS = ("visbuffer_attachment", "normalmap", "splatmap", "materials_buffer", "brush_hit", "albedo_attachment", "normal_attachment", "emissive_attachment",
           "metallic_roughness_occlusion_attachment")
GUARD_OF = {"visbuffer_attachment": "vis", "materials_buffer": "materials", "brush_hit": "hit", "albedo_attachment": "albedo", "normal_attachment": "normal",
            "emissive_attachment": "emissive", "metallic_roughness_occlusion_attachment": "mro"}


@pytest.fixture(scope="module")
def refusal(r):
    f = DF.frame((17, 9), T=DF.terrain(brush_radius=300.0), hit=DF.hit_record((0.0, 0.0, 0.0)))
    gs = DF.guards(f)
    return f, gs, DF.context(f, gs)


def _refused(r, context, message, gs, f):
    raises_refusal(lambda: r.decode_terrain(context), message)
    DF.check_unwritten(gs, f, message)


def _flat(gs, field):
    return gs[GUARD_OF.get(field, field)].tensor.view(-1)


def _cases(base, gs):
    """(context, message) for every limit on its own, in the header's order."""
    from oxylus_amd.renderer import ImageAttachment

    d = base.depth_attachment
    cases = [(Raw(base, width=16), "depth_attachment extent differs"), (Raw(base, height=10), "depth_attachment extent differs"),
             (rep(base, depth_attachment=ImageAttachment(d.data, 17, 9, 2, [0, 4])), "depth_attachment must be one R32F level"),
             (rep(base, depth_attachment=ImageAttachment(d.data, 17, 9, 1, [4])), "depth_attachment must be one R32F level")]
    cases += [(rep(base, map_resolution=v), "map_resolution: every side") for v in ((0, 20), (24, 0), (16385, 20), (24, 16385))]
    for field in BUFFERS:
        flat = _flat(gs, field)
        short = "materials_buffer is smaller than material_count records" if field == "materials_buffer" else field + SHORT
        cases += [(rep(base, **{field: None}), field + NULL), (rep(base, **{field: flat.view(torch.int8)[1:-1]}), field + ALIGNED), (rep(base, **{field: flat[:-2]}), short)]
    cases.append((rep(base, brush_hit=_flat(gs, "brush_hit")[1:]), "brush_hit" + ALIGNED))
    outs = BUFFERS[5:]
    cases += [(rep(base, **{outs[k]: gs["albedo"].tensor}), "albedo_attachment must not overlap") for k in (2, 3)]
    cases += [(rep(base, emissive_attachment=gs["vis"].tensor), "emissive_attachment must not overlap visbuffer_attachment"),
              (rep(base, metallic_roughness_occlusion_attachment=gs["depth"].tensor.view(torch.int32)), "metallic_roughness_occlusion_attachment must not overlap depth_attachment"),
              (rep(base, brush_hit=gs["normal"].tensor.view(-1).view(torch.int32)[2:6]), "normal_attachment must not overlap brush_hit"),
              (rep(base, materials_buffer=gs["albedo"].tensor.view(-1)[:70]), "albedo_attachment must not overlap materials_buffer")]
    return cases


def test_every_limit_on_its_own(r, refusal):
    f, gs, base = refusal
    for context, message in _cases(base, gs):
        _refused(r, context, message, gs, f)
    DF.run(r, f, "the frame still decodes")


def test_zero_extent(r, refusal):
    from oxylus_amd.renderer import ImageAttachment

    f, gs, base = refusal
    d = base.depth_attachment
    for w, h in ((0, 9), (17, 0), (0, 0)):
        _refused(r, Raw(base, width=w, height=h), "the extent must not be zero", gs, f)
    _refused(r, rep(base, depth_attachment=ImageAttachment(d.data, 0, 9, 1, [0])), "the extent must not be zero", gs, f)


def test_the_first_broken_rule_gives_the_message(r, refusal):
    """Two rules broken at once, for neighbouring pairs of the header's order: the earlier one is named."""
    from oxylus_amd.renderer import ImageAttachment

    f, gs, base = refusal
    d = base.depth_attachment
    pairs = [(Raw(rep(base, depth_attachment=ImageAttachment(d.data, 17, 9, 2, [0, 4])), width=0), "the extent must not be zero"),
             (Raw(rep(base, depth_attachment=ImageAttachment(d.data, 17, 9, 2, [0, 4])), height=8), "depth_attachment extent differs"),
             (rep(base, depth_attachment=ImageAttachment(d.data, 17, 9, 2, [0, 4]), map_resolution=(0, 0)), "depth_attachment must be one R32F level"),
             (rep(base, map_resolution=(0, 0), visbuffer_attachment=None), "map_resolution: every side")]
    for a, b in zip(BUFFERS[:-1], BUFFERS[1:]):
        pairs.append((rep(base, **{a: None, b: None}), a + NULL))
        pairs.append((rep(base, **{a: _flat(gs, a)[:-2], b: None}), a + (" is smaller than" if a == "materials_buffer" else SHORT)))
    pairs.append((rep(base, metallic_roughness_occlusion_attachment=None, emissive_attachment=gs["albedo"].tensor), "metallic_roughness_occlusion_attachment" + NULL))
    for context, message in pairs:
        _refused(r, context, message, gs, f)
    DF.run(r, f, "the frame still decodes")


def test_null_context_and_short_struct_size(r, refusal):
    import ctypes as C

    from oxylus_amd import lib as L

    f, gs, base = refusal
    lib = L.load()
    assert lib.oxc_decode_terrain(r._ctx, None, None) == L.OXC_INVALID_ARG
    assert lib.oxc_decode_terrain(None, None, None) == L.OXC_INVALID_ARG
    c = base.c()
    c.struct_size = C.sizeof(L.TerrainDecodeContext) - 8
    assert lib.oxc_decode_terrain(r._ctx, C.byref(c), None) == L.OXC_INVALID_ARG
    assert b"struct_size" in lib.oxc_last_error(r._ctx)
    torch.cuda.synchronize()
    DF.check_unwritten(gs, f, "short struct_size")
