"""oxc_draw_sprites and oxc_pick_sprite on the GPU against tests/sprites_model.py: every word of the depth, of visbuffer_2d and of the lit
image equal to the checker's between poisoned guard bands (sprites_frames.run / run_pick) -- at the tile and bin seams, at the chunk and list
capacities, in and against the sprite order, around the scene depth, under clipping, discard and the quantisation between sprites, after
the library's own frame chain, in a captured graph, and at every limit.  The shapes are the smallest at which each mechanism can go wrong."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import refusals as R
import sprites_frames as SF
import sprites_model as SM
from gpu_passes import ALL_FLAGS, DrawnFrame, Guard, lights_tensor, same

pytestmark = pytest.mark.gpu
rep = dataclasses.replace
F = np.float32
NAN = float("nan")
STAGE_IDS = ["vis", "color", "both"]
FORMAT_IDS = ["b10g11r11", "rgba16f"]
BIN, TILE, CHUNK, CAP = SF.BIN, SF.TILE, SF.CHUNK, SF.BIN_CAPACITY


@pytest.fixture(scope="module")
def r(renderer):
    return renderer


def run_all(r, f, label, formats=SF.FORMATS, stages=SF.STAGES):
    out = {}
    for fmt in formats:
        for st in stages:
            out[st, fmt] = SF.run(r, f, f"{label} stages {st} format {fmt}", st, fmt)
    return out


# ---- extents and seams ----------------------------------------------------------------------------------------------------------------------
def test_the_golden_frame(r):
    f = SF.golden_frame()
    got = run_all(r, f, "golden")
    with np.load(SF.GOLDEN) as g:
        for (st, fmt), images in got.items():
            same(images, {k: g[f"{k}_format{fmt}_stages{st}"] for k in images}, f"fixture stages {st} format {fmt}")


@pytest.mark.parametrize("extent", [(1, 1), (17, 9)])
def test_tiny_extents(r, extent):
    run_all(r, SF.stack_frame(extent, n=3), f"{extent}")


def seam_frame(side):
    """An extent of `side` + 1 each way: one sprite across each seam of the `side` grid, one ending exactly on it, one in the far corner."""
    W = H = side + 1
    d, color = SF.background(W, H)
    quads = [SF.quad(W, H, side, side / 2.0, 6, 5, 0.5, angle=0.2),            # across the vertical seam
             SF.quad(W, H, side / 2.0, side, 5, 6, 0.5, shear=0.3),           # across the horizontal seam
             SF.quad(W, H, side - 3, side - 3, 6, 6, 0.6),                    # exactly on both seams: its last pixel is side - 1
             SF.quad(W, H, side + 0.5, side + 0.5, 1, 1, 0.7),                # the one pixel beyond both
             SF.quad(W, H, side / 2.0, side / 2.0, side * 1.5, side * 1.5, 0.3, angle=0.4)]  # over everything, behind the others
    return SF.Frame(SF.sprites_of([(k, k) for k in range(5)]), SF.materials_of(SF.PALETTE[:5]), np.stack(quads), d, color)


@pytest.mark.parametrize("side", [TILE, BIN], ids=["tile", "bin"])
def test_one_pixel_past_a_tile_and_past_a_bin(r, side):
    f = seam_frame(side)
    stats = {}
    SF.want(f, SM.COLOR, stats=stats)
    assert stats["blends"][3][side, side] == 1 and stats["blends"][2][side - 1, side - 1] == 1 and stats["blends"][2][side, side] == 0
    run_all(r, f, f"seam {side}", formats=(SM.B10G11R11,) if side == BIN else SF.FORMATS)


# ---- sprite counts --------------------------------------------------------------------------------------------------------------------------
def many_frame(n, extent=(21, 13), seed=1):
    """n small translucent sprites scattered over a small image, eight materials, a few at equal depths."""
    W, H = extent
    rng = np.random.default_rng(seed + n)
    d, color = SF.background(W, H)
    quads = np.stack([SF.quad(W, H, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1, 6), rng.uniform(1, 6), 0.3 + 0.05 * int(rng.integers(0, 8)), angle=rng.uniform(0, 3))
                      for _ in range(max(n, 1))])
    return SF.Frame(SF.sprites_of([(k, k % 8) for k in range(n)]), SF.materials_of(SF.PALETTE), quads, d, color)


@pytest.mark.parametrize("n", [0, 1, 64, 65, CHUNK, CHUNK + 1])
def test_sprite_counts_around_the_wave_and_the_chunk(r, n):
    run_all(r, many_frame(n), f"{n} sprites", formats=(SM.B10G11R11,))
    if n == 65:
        SF.run(r, many_frame(n), "65 sprites rgba16f", SM.ALL, SM.RGBA16F)


def test_a_count_beyond_the_bin_list_capacity(r):
    """CAP + 1 sprites in one bin: the tiles walk the sprite range themselves; the picture is the checker's."""
    f = many_frame(CAP + 1, extent=(19, 7))
    SF.run(r, f, "capacity + 1, both", SM.ALL)
    SF.run(r, f, "capacity + 1, color", SM.COLOR, SM.RGBA16F)


def test_first_sprite_and_a_shorter_batch(r):
    f = rep(many_frame(40), first_sprite=7, sprite_count=20)
    a = run_all(r, f, "first_sprite 7", formats=(SM.B10G11R11,))
    whole = SF.want(rep(f, first_sprite=0, sprite_count=None), SM.ALL)
    assert (a[SM.ALL, 0]["color"] != whole["color"]).any()


def test_no_clear_keeps_the_words_no_fragment_reaches(r):
    f = many_frame(9)
    W, H = f.extent
    f = rep(f, clear=False, vis=(np.arange(W * H, dtype=np.uint32).reshape(H, W) + np.uint32(1000)))
    got = SF.run(r, f, "no clear", SM.VIS)
    assert (got["vis"] >= 1000).any() and (got["vis"] < 9).any()


# ---- order, depth ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", SF.FORMATS, ids=FORMAT_IDS)
def test_eight_sprites_at_one_depth_blend_in_list_order(r, fmt):
    f = SF.stack_frame((23, 19))
    back = rep(f, sprites=f.sprites[::-1].copy())
    a, b = SF.run(r, f, "in order", SM.COLOR, fmt), SF.run(r, back, "reversed", SM.COLOR, fmt)
    assert (a["color"] != b["color"]).any()
    stats = {}
    SF.want(f, SM.VIS, stats=stats)
    last = stats["blends"][7] > 0
    vis = SF.run(r, f, "vis", SM.VIS)["vis"]
    assert last.sum() > 20 and (vis[last] == 7).all()


def test_back_to_front_and_front_to_back(r):
    """COLOR alone depends on the list's direction, VIS | COLOR does not (S7)."""
    f = SF.stack_frame((23, 19), same_depth=False)
    back = rep(f, sprites=f.sprites[::-1].copy())
    assert (SF.run(r, f, "b2f color", SM.COLOR)["color"] != SF.run(r, back, "f2b color", SM.COLOR)["color"]).any()
    same(SF.run(r, f, "b2f both", SM.ALL), SF.run(r, back, "f2b both", SM.ALL), "both stages")


def test_sprites_around_the_scene_depth(r):
    """In front of, behind and exactly at the stored depth (>=), and depths outside (0, 1]; a NaN and an Inf in the attachment."""
    W, H = 19, 11
    d, color = SF.background(W, H, depth=0.5)
    d[0, :4] = [NAN, np.inf, -np.inf, 0.0]
    zs = [0.75, 0.25, 0.5, 0.0, -0.25, 1.0, float(np.nextafter(F(1.0), F(2.0))), 1.5, float(np.nextafter(F(0.5), F(0.0)))]
    quads = np.stack([SF.quad(W, H, 2 + 2 * k, 5, 3, 12, z) for k, z in enumerate(zs)])
    f = SF.Frame(SF.sprites_of([(k, k % 8) for k in range(len(zs))]), SF.materials_of(SF.PALETTE), quads, d, color)
    stats = {}
    SF.want(f, SM.COLOR, stats=stats)
    drawn = [int(stats["blends"][k].sum() > 0) for k in range(len(zs))]
    assert drawn == [1, 0, 1, 0, 0, 1, 0, 0, 0], drawn
    run_all(r, f, "depths")


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
def test_rotated_sheared_flipped_mirrored_and_degenerate(r):
    W, H = 37, 29
    d, color = SF.background(W, H)
    skew = SF.column_major([[0.3, 0.1, 0, -0.2], [-0.05, 0.4, 0, 0.1], [0.2, 0.1, 1, 0.5], [0, 0, 0, 1]])  # not symmetric in x: FLIP_X shows
    quads = np.stack([SF.quad(W, H, 10, 10, 14, 9, 0.5, angle=0.6), SF.quad(W, H, 24, 18, 12, 10, 0.5, shear=0.5), skew, skew,
                      SF.quad(W, H, 20, 8, 9, 7, 0.6, angle=1.0, mirror=True), SF.quad(W, H, 5, 20, 0, 0, 0.7), SF.quad(W, H, 30, 5, 6, 0, 0.7)])
    flags = [0, 0, 0, SM.FLIP_X, 0, 0, SM.FLIP_X]
    f = SF.Frame(SF.sprites_of([(k, 0, flags[k]) for k in range(7)]), SF.materials_of([(1.0, 0.5, 0.25, 0.5)]), quads, d, color)
    stats = {}
    SF.want(f, SM.COLOR, stats=stats)
    b = stats["blends"]
    assert all(b[k].max() == 1 for k in (0, 1, 2, 3, 4)) and b[5].sum() == 0 and b[6].sum() == 0
    # FLIP_X mirrors the corners: the parallelogram is the same set of pixels, cut along its other diagonal
    assert (b[2] == b[3]).all() and b[2].sum() > 10 and b[4].sum() > 20
    run_all(r, f, "shapes")


def clip_frame():
    """A perspective camera (w = world z): a sprite wholly inside, one crossing w = 2^-10, one crossing a guard-band plane, one wholly behind
    the camera."""
    W, H = 41, 31
    d, color = SF.background(W, H, depth=0.0001)
    pv = SF.column_major([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0.0002], [0, 0, 1, 0]])
    tilted = lambda x0, z0, dzdx, size: SF.column_major([[size, 0, 0, x0], [0, size, 0, 0.1], [dzdx, 0, 1, z0], [0, 0, 0, 1]])  # noqa: E731
    quads = np.stack([tilted(0.0, 0.2, 1.0, 0.8),       # z from -0.2 to 0.6: crosses w = 2^-10
                      tilted(0.3, 0.004, 0.0, 0.7),     # w = 0.004 everywhere, |x| up to 0.65 > 64 w: crosses the guard planes
                      tilted(0.0, -1.0, 0.1, 0.5),      # behind the camera
                      tilted(-0.1, 0.5, 0.2, 0.6)])
    return SF.Frame(SF.sprites_of([(3, 3), (0, 0), (1, 1), (2, 2)]), SF.materials_of(SF.PALETTE[:4]), quads, d, color, pv=pv)


def test_clipped_sprites(r):
    f = clip_frame()
    W, H = f.extent
    n, m, t = f.counts
    pieces = [SM.sprite_setup(f.sprites[k], f.materials, m, f.transforms, t, f.pv, W, H) for k in range(4)]
    assert len(pieces[0][2]) == 2 and len(pieces[1][2]) > 2 and len(pieces[2][2]) > 2 and len(pieces[3][2]) == 0
    stats = {}
    SF.want(f, SM.COLOR, stats=stats)
    assert all(stats["blends"][k].sum() > 10 and stats["blends"][k].max() == 1 for k in (0, 1, 2))
    run_all(r, f, "clip")


def test_discard_and_out_of_range_indices(r):
    """Alpha below, equal to and above the cutoff; a NaN alpha and a NaN cutoff; a material index at material_count; a transform_id at
    transform_count."""
    W, H = 29, 9
    d, color = SF.background(W, H)
    colors = [(1, 0, 0, 0.25), (0, 1, 0, 0.5), (0, 0, 1, 0.75), (1, 1, 0, NAN), (0, 1, 1, 0.5), (1, 0, 1, 0.5)]
    mats = SF.materials_of(colors, cutoffs=[0.5, 0.5, 0.5, 0.5, NAN, -1.0])
    entries = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 5)]  # sprite 6: the material beyond the count; sprite 7: the transform beyond it
    quads = np.stack([SF.quad(W, H, 2 + 3.5 * k, 4, 3, 7, 0.5) for k in range(8)])
    f = SF.Frame(SF.sprites_of(entries), mats, quads, d, color, material_count=6, transform_count=7)
    stats = {}
    SF.want(f, SM.COLOR, stats=stats)
    assert [int(k in stats["blends"] and stats["blends"][k].sum() > 0) for k in range(8)] == [0, 0, 1, 1, 1, 1, 0, 0]
    run_all(r, f, "discard")


@pytest.mark.parametrize("fmt", SF.FORMATS, ids=FORMAT_IDS)
def test_the_attachments_quantisation_sits_between_two_sprites(r, fmt):
    f = SF.stack_frame((23, 19))
    got = SF.run(r, f, "requantised", SM.COLOR, fmt)
    assert (got["color"] != SF.want(f, SM.COLOR, fmt, requantize=False)["color"]).any()


# ---- after the real chain, determinism, graph -----------------------------------------------------------------------------------------------
def chain_frame(d, fmt):
    """Sprites over the depth and the lit image of the drawn 192 x 192 frame."""
    W, H = d.W, d.H
    depth = d.f.depth.cpu().numpy()
    lit = np.ascontiguousarray(d.pbr_ctx.final_attachment.cpu().numpy()).view(np.uint32)
    rng = np.random.default_rng(9)
    quads = np.stack([SF.quad(W, H, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(8, 150), rng.uniform(8, 90), float(depth.max()) * rng.uniform(0.2, 1.2), angle=rng.uniform(0, 3))
                      for _ in range(24)])
    return SF.Frame(SF.sprites_of([(k, k % 8) for k in range(24)]), SF.materials_of(SF.PALETTE), quads, depth, lit)


def test_after_the_frame_chain_and_into_fxaa(r):
    from oxylus_amd.renderer import FxaaContext

    d = DrawnFrame(r)
    d.passes()
    d.pbr_ctx = d.pbr(ALL_FLAGS, lights_tensor(d.four_lights()))
    r.apply_pbr(d.pbr_ctx)
    torch.cuda.synchronize()
    f = chain_frame(d, SM.B10G11R11)
    got = SF.run(r, f, "chain", SM.ALL)
    assert (got["color"] != f.color).sum() > 1000 and (got["vis"] != SM.EMPTY).sum() > 1000
    image = torch.from_numpy(got["color"].view(np.int32).copy()).cuda()
    fx = FxaaContext.create(image)
    r.apply_fxaa(fx)
    torch.cuda.synchronize()
    assert fx.fxaa_attachment.shape == image.shape and bool((fx.fxaa_attachment != 0).any())


def test_two_runs_are_identical_and_a_captured_graph_replays(r):
    f = many_frame(300, extent=(BIN + 9, 40))
    for fmt in SF.FORMATS:
        same(SF.run(r, f, "first", SM.ALL, fmt), SF.run(r, f, "second", SM.ALL, fmt), "two runs")
    gs = SF.guards(f, SM.ALL)
    r.prepared_frame = SF.prepared_frame(gs, f)
    ctx = SF.context(f, gs, SM.ALL)
    originals = {k: gs[k].tensor.clone() for k in ("depth", "color")}
    r.draw_sprites(ctx)  # the warm call: the scratch is sized
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        r.draw_sprites(ctx, stream=stream)
    want = SF.want(f, SM.ALL)
    for replay in range(2):
        for k, t in originals.items():
            gs[k].tensor.copy_(t)
        gs["vis"].refill()
        graph.replay()
        torch.cuda.synchronize()
        for g in gs.values():
            g.check(f"replay {replay}")
        same(SF.outputs(gs, f, SM.ALL, 0), want, f"replay {replay}")


def test_a_larger_call_is_refused_under_capture(r):
    from oxylus_amd import lib as L

    f = many_frame(5000, extent=(9, 9))  # more sprites than any call of this module before it
    gs = SF.guards(f, SM.VIS)
    r.prepared_frame = SF.prepared_frame(gs, f)
    ctx = SF.context(f, gs, SM.VIS)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(L.OxcError, match="make one un-captured call first"):
            r.draw_sprites(ctx, stream=stream)
    torch.cuda.synchronize()
    assert (gs["vis"].bits()[1] == SF.FILL_VIS).all()


# ---- pick -----------------------------------------------------------------------------------------------------------------------------------
def test_pick_sprite_on_hit_empty_and_corner_texels(r):
    f = SF.golden_frame()
    W, H = f.extent
    vis = SF.want(f, SM.VIS)["vis"]
    ys, xs = np.nonzero(vis != SM.EMPTY)
    ye, xe = np.nonzero(vis == SM.EMPTY)
    texels = [(int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1])), (int(xe[0]), int(ye[0])), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    got = SF.run_pick(r, vis, texels, "pick")
    assert got[2] == SM.EMPTY and got[0] != SM.EMPTY


# ---- limits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", SF.FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("stages", SF.STAGES, ids=STAGE_IDS)
def test_sprite_limits_alone_and_in_pairs(r, stages, fmt):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    f = SF.golden_frame()
    W, H = f.extent
    gs = SF.guards(f, stages, fmt)
    frame = SF.prepared_frame(gs, f)
    base = SF.context(f, gs, stages, fmt)
    before = {k: g.bits()[1].copy() for k, g in gs.items()}
    t = lambda name: gs[name].tensor  # noqa: E731
    has_vis, has_color = bool(stages & SM.VIS), bool(stages & SM.COLOR)
    extent = "extent beyond 16384"
    cases = [("struct_size", {"raw:struct_size": C.sizeof(L.SpriteContext) - 8}, "bad context / struct_size"),
             ("no stage", dict(stages=0), "stages must be"), ("an unknown stage", dict(stages=stages | 4), "stages must be"),
             ("width 0", dict(width=0), "the extent must not be zero"), ("height 0", dict(height=0), "the extent must not be zero"),
             ("16385 wide", dict(width=16385), extent), ("16385 tall", dict(height=16385), extent)]
    if has_color:
        cases.append(("format 2", dict(source_format=2), "source_format must be 0"))
    cases += [("the range wraps", dict(first_sprite=0xFFFFFFFF, sprite_count=2), "first_sprite + sprite_count wraps"),
              ("too many sprites", {"raw:sprite_count": SM.MAX_SPRITES + 1}, "sprite_count beyond 1048576"),
              ("depth of another extent", dict(depth_attachment=ImageAttachment.depth(torch.zeros((H, W + 1), device="cuda"))), "depth_attachment extent differs"),
              ("two depth levels", dict(depth_attachment=rep(ImageAttachment.depth(t("depth")), levels=2, level_offset=[0, 0])), "depth_attachment must be one R32F level"),
              ("no frame", {"frame": None}, "the frame must not be null")]
    cases += R.buffer_cases("sprites_buffer", t("sprites"), torch.int16, " is smaller than first_sprite + sprite_count records")
    cases += R.buffer_cases("materials_buffer", t("materials").view(-1), torch.int16, " is smaller than material_count records")
    cases.append(("depth null", dict(depth_attachment=R.null_image(W, H)), "depth_attachment must not be null"))
    if has_vis:
        cases += R.buffer_cases("visbuffer_2d", t("vis"), torch.int16)
    if has_color:
        cases += R.buffer_cases("final_attachment", t("color"), torch.int32 if fmt else torch.int16)
    cases += R.buffer_cases("frame:transforms", t("transforms"), torch.int16, " is smaller than transform_count matrices", "transforms_world_buffer")
    # every written buffer over every other buffer of the call
    written = (["depth_attachment"] + (["visbuffer_2d"] if has_vis else []) + (["final_attachment"] if has_color else []))
    tensors = {"sprites_buffer": t("sprites"), "materials_buffer": t("materials").view(-1), "depth_attachment": t("depth"), "frame:transforms": t("transforms")}
    tensors.update({"visbuffer_2d": t("vis")} if has_vis else {})
    tensors.update({"final_attachment": t("color")} if has_color else {})
    shown = lambda k: "transforms_world_buffer" if k == "frame:transforms" else k  # noqa: E731
    table = ["sprites_buffer", "materials_buffer", "depth_attachment", "visbuffer_2d", "final_attachment", "frame:transforms"]  # the checking order
    need = {"sprites_buffer": 60, "materials_buffer": 280, "depth_attachment": W * H * 4, "visbuffer_2d": W * H * 4, "final_attachment": W * H * (8 if fmt else 4),
            "frame:transforms": 320}
    for wname in written:
        for oname in tensors:
            wt = tensors[wname]
            if oname == wname or wt.numel() * wt.element_size() < need[oname] or wt.data_ptr() % (8 if fmt and oname == "final_attachment" else 4):
                continue  # the other buffer does not fit on the written one's bytes: the pair is met from its other side
            alias = ImageAttachment.depth(wt.view(-1).view(torch.float32)[:W * H].view(H, W)) if oname == "depth_attachment" else wt
            first, second = sorted((wname, oname), key=table.index) if oname in written else (wname, oname)
            cases.append((f"{oname} on the bytes of {wname}", {oname: alias}, f"{shown(first)} must not overlap {shown(second)}"))

    def unwritten(label):
        for k, g in gs.items():
            g.check(label)
            assert (g.bits()[1] == before[k]).all(), f"{label}: {k} written after a refusal"

    # a case that aliases replaces a field a pair partner might need intact: pairs only among the cases before the overlaps
    first_overlap = next(i for i, c in enumerate(cases) if " on the bytes of " in c[0])
    R.alone_and_in_pairs(r, "oxc_draw_sprites", cases[:first_overlap], base, frame, unwritten)
    for name, changes, message in cases[first_overlap:]:
        R.refused(r, "oxc_draw_sprites", base, changes, message, name, frame)
    torch.cuda.synchronize()
    unwritten("overlaps")
    # an input the stage does not read is not checked; a null materials_buffer is fine with material_count 0; sprite_count 0 only clears
    status, error = R.attempt(r, "oxc_draw_sprites", base, dict(materials_buffer=None, material_count=0, sprite_count=0, **({} if has_color else dict(source_format=9))), frame)
    assert status == L.OXC_OK, error
    torch.cuda.synchronize()
    if has_vis:
        assert (gs["vis"].bits()[1] == SM.EMPTY).all()
    for k in ("depth", "color"):
        if k in gs:
            assert (gs[k].bits()[1] == before[k]).all()


def test_pick_sprite_limits(r):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import SpritePickContext

    W, H = 17, 9
    src = Guard("vis", (H, W), torch.int32, W, SF.POISON32, 4, fill=7)
    out = Guard("transform_id", (1,), torch.int32, 1, SF.POISON32, 4, fill=0x0BADBAD0)
    base = SpritePickContext.over(src.tensor, (3, 5), out.tensor)
    cases = [("struct_size", {"raw:struct_size": C.sizeof(L.SpritePickContext) - 8}, "bad context / struct_size"),
             ("width 0", dict(width=0), "the extent must not be zero"), ("65537 wide", dict(width=65537), "extent beyond 65536"),
             ("x outside", dict(picking_texel=(W, 5)), "the texel lies outside the image"), ("y outside", dict(picking_texel=(3, H)), "the texel lies outside the image")]
    cases += R.buffer_cases("visbuffer_2d", src.tensor, torch.int16)
    cases += R.buffer_cases("transform_id", out.tensor, torch.int16, None)
    cases.append(("the word inside the image", dict(transform_id=src.tensor.view(-1)[4:5]), "transform_id must not overlap visbuffer_2d"))

    def unwritten(label):
        src.check(label), out.check(label)
        assert (out.bits()[1] == 0x0BADBAD0).all() and (src.bits()[1] == 7).all(), label

    R.alone_and_in_pairs(r, "oxc_pick_sprite", cases, base, R.NO_FRAME, unwritten)
