"""oxc_decode_visbuffer_textured on the GPU: every word of the four G-buffer images equals tests/textured_decode_model.py and every counter
equals its count -- with no flag set the bytes of oxc_decode_visbuffer on the drawn 192 x 192 frame; each of the 32 image-flag
combinations over poisoned unread images; the five sampler presets by the three formats on the four image sizes; magnified, integer and
past-the-end LODs, zero and NaN gradients, special halves; negative and large uv under both address modes, texel centres and edges;
normal maps flipped, two-component, under a zero Jacobian and a mirrored chart; waves of one material and of 64; extents between guard
bands; every 4-byte alignment of an image base; the frame from draw to PBR in one graph with an image rewritten between replays; every
limit alone and in pairs."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import textured_decode_frames as FR
import textured_decode_model as TM
from gpu_passes import DrawnFrame, Guard, decode_got_of, same
from scenes import OUT16, OUT32

pytestmark = pytest.mark.gpu

LIN_REP, LIN_CLAMP, NEAR_REP, NEAR_CLAMP = (FR.PRESET_RECORDS[p] for p in FR.PRESETS[:4])
NAN_H, INF_H, NINF_H, DEN_H, NDEN_H, NZERO_H = 0x7E00, 0x7C00, 0xFC00, 0x0001, 0x83FF, 0x8000


# ---- flags clear ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["null", "poisoned"])
def test_no_flag_set_is_the_untextured_decode(renderer, tables):
    """The drawn 192 x 192 frame of main_scene (no material has a flag): the bytes of oxc_decode_visbuffer, with the tables null or holding
    records that must not be read."""
    from oxylus_amd.renderer import MaterialImagesContext

    fr = DrawnFrame(renderer)
    fr.passes()
    old = decode_got_of(fr.dctx)
    assert (old["albedo"] != 0).sum() > 0.3 * fr.W * fr.H
    for t in (fr.dctx.albedo_attachment, fr.dctx.normal_attachment, fr.dctx.emissive_attachment, fr.dctx.metallic_roughness_occlusion_attachment):
        t.fill_(-5)
    rec = smp = None
    if tables == "poisoned":
        rec = torch.full((4 * 144,), 0xA5, dtype=torch.uint8, device="cuda")
        smp = torch.full((4, 4), -1, dtype=torch.int32, device="cuda")
    images = MaterialImagesContext.create(fr.cpu.camera["position"], rec, smp)
    dev = FR.counted(renderer, fr.dctx, images)
    same(decode_got_of(fr.dctx), old, "against oxc_decode_visbuffer")
    assert dev["decoded"] == int((old["mro"] != 0).sum()) and dev["level_taps"] == 0 and all(dev["sampled_" + k] == 0 for k in TM.KINDS)
    assert dev["uniform_waves"] > 0 and dev["per_lane_waves"] > 0, dev  # both paths write the same bytes


# ---- flag combinations ------------------------------------------------------------------------------------------------------------------------------
def test_the_32_flag_combinations(renderer):
    """One material per combination; an image whose flag is clear is named by an index past the table or by a record that cannot be read
    (levels 0 over a wild pointer, a null pointer)."""
    flags = list(range(32))
    images = FR.five_images() + [dict(width=4, height=4, format=0, levels=[]), None]
    idx = np.zeros((32, 5), np.int64)
    for m, kind in itertools.product(range(32), range(5)):
        idx[m, kind] = kind if (m >> kind) & 1 else (5, 6, 7, 0xFFFFFFFF, 1000)[(m + kind) % 5]
    f = FR.frame(64, 16, flags, mode="bands", images=images, image_indices=idx)
    f.vis = FR.assign(64, 16, 32, "pixels")
    st = FR.check(renderer, f, "32 combinations")
    assert all(st["sampled_" + k] > 0 for k in TM.KINDS) and st["per_lane_waves"] > 0


def test_flagged_images_that_are_absent_fall_back_to_the_factor(renderer):
    """Every flag set, every image absent by one of the rules of step 13: the untextured result."""
    images = [None, dict(width=4, height=4, format=0, levels=[]), dict(FR.chain(4, 4, 1, 0, 3), format=3), dict(FR.chain(4, 4, 1, 0, 3), width=0),
              dict(FR.chain(4, 4, 1, 0, 3), height=16385)]
    f = FR.frame(17, 9, [FR.ALL_IMAGES, FR.ALL_IMAGES], images=images, image_indices=[[0, 1, 2, 3, 4], [4, 3, 9, 1, 0]])
    st = FR.check(renderer, f, "absent")
    assert st["level_taps"] == 0 and st["decoded"] > 100
    plain = dataclasses.replace(f, images=[], samplers=[])
    same(FR.want(f), FR.want(plain), "the checker's own fallback")


# ---- sampler presets x formats ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [TM.UNORM, TM.SRGB, TM.RG8], ids=["unorm", "srgb", "rg8"])
@pytest.mark.parametrize("preset", FR.PRESETS)
def test_sampler_presets_and_formats(renderer, preset, fmt):
    """Four materials, one per image size (1 x 1, 2 x 2, 5 x 3 with 3 levels, 16 x 16 with 5), all five kinds from that image; uv_size 3
    and a tilted quad spread lambda over the chains."""
    images = FR.image_set(fmt)
    idx = np.repeat(np.arange(4)[:, None], 5, axis=1)
    f = FR.frame(33, 19, [FR.ALL_IMAGES | (TM.TWO_COMPONENT if fmt == TM.RG8 else 0)] * 4, mode="pixels", images=images, samplers=[FR.PRESET_RECORDS[preset]],
                 image_indices=idx, uv_size=[[3.0, 3.0]] * 4, uv_offset=[[-0.5, 0.25]] * 4)
    st = FR.check(renderer, f, f"{preset}, format {fmt}")
    assert st["sampled_albedo"] == st["decoded"] and st["level_taps"] == 5 * st["decoded"] * (2 if FR.PRESET_RECORDS[preset][2] else 1)


def test_sampler_index_out_of_range_is_linear_repeat_linear(renderer):
    f = FR.frame(17, 9, [FR.ALL_IMAGES] * 2, samplers=[NEAR_CLAMP], sampler_index=[1, 0xFFFFFFFF], uv_size=[[2.0, 2.0]] * 2)
    FR.check(renderer, f, "sampler out of range")
    out_of_range = FR.want(f)
    f.cpu.materials.view(torch.int32).view(-1, 14)[:, 6] = 0  # the same frame, every material on sampler 0 = linear / repeat / linear
    same(out_of_range, FR.want(dataclasses.replace(f, samplers=[LIN_REP])), "the default sampler")


# ---- LOD ------------------------------------------------------------------------------------------------------------------------------------------------
LOD_CASES = {
    "magnified": dict(uv_size=[[0.01, 0.01]] * 2),                      # rho < 1: lambda < 0 clamps to level 0
    "integer": dict(uv_size=[[1.0, 1.0], [2.0, 2.0]], flat=16),         # the exact frame, one texel and two texels a pixel row: lambda 0.0 and 1.0, asserted
    "past the end": dict(uv_size=[[512.0, 512.0]] * 2),                 # lambda beyond levels - 1
    "zero size": dict(uv_size=[[0.0, 0.0], [NZERO_H, 0]]),              # rho = 0: log2 gives -Inf
    "special size": dict(uv_size=np.array([[NAN_H, 0x3C00], [INF_H, NINF_H]]), uv_offset=np.array([[DEN_H, NDEN_H], [NAN_H, INF_H]])),
    "special offset": dict(uv_offset=np.array([[INF_H, 0], [NINF_H, NAN_H]])),
}


@pytest.mark.parametrize("case", LOD_CASES)
@pytest.mark.parametrize("sampler", [LIN_REP, NEAR_CLAMP], ids=["linear", "nearest"])
def test_lod(renderer, case, sampler):
    kw = dict(LOD_CASES[case])
    flat = kw.pop("flat", 0)
    if flat:  # 32 x 16 pixels over the 16 x 16 images: uv advances 1 / 32 and 1 / 16 a pixel, rho = max(0.5, 1) texels; both 16-pixel bands show
        f = FR.exact_frame(2 * flat, flat, [FR.ALL_IMAGES] * 2, samplers=[sampler], **kw)
    else:
        f = FR.frame(17, 9, [FR.ALL_IMAGES] * 2, samplers=[sampler], **kw)
    st = FR.check(renderer, f, case)
    assert st["sampled_albedo"] > 0
    if flat:
        material = st["fetched"]["material_index"][st["fetched"]["valid"]][st["triangle_slot"]]
        for kind in range(5):
            assert (st["lod"][kind][material == 0] == 0.0).all() and (st["lod"][kind][material == 1] == 1.0).all(), kind
        assert (material == 0).sum() > 200 and (material == 1).sum() > 200


def test_degenerate_triangles_and_special_texcoords(renderer):
    """A zero-area triangle (NaN gradients), a mesh without texcoords, and texcoords that are NaN, Inf and denormal halves."""
    zero = list(FR.quad_mesh())
    zero[0] = zero[0].copy()
    zero[0][2] = zero[0][1]  # two equal corners
    special = FR.quad_mesh(uv=np.array([[NAN_H, 0x3800], [INF_H, DEN_H], [0x3C00, NINF_H], [NDEN_H, 0x4000]]))
    meshes = [FR.quad_mesh(), tuple(zero), FR.quad_mesh(uv=None), special]
    for sampler in (LIN_REP, LIN_CLAMP, NEAR_REP):
        f = FR.frame(33, 9, [FR.ALL_IMAGES] * 4, mode="pixels", meshes=meshes, mesh_of=[0, 1, 2, 3], samplers=[sampler])
        st = FR.check(renderer, f, f"degenerate, {sampler}")
        assert st["sampled_normal"] == st["decoded"]


def test_levels_1_with_linear_mips_and_non_power_of_two(renderer):
    images = [FR.chain(5, 3, 1, TM.SRGB, 3), FR.chain(5, 3, 3, TM.UNORM, 4), FR.chain(7, 2, 3, TM.SRGB, 5), FR.chain(3, 6, 3, TM.UNORM, 6), FR.chain(1, 9, 4, TM.UNORM, 7)]
    for sampler in (LIN_REP, LIN_CLAMP):
        f = FR.frame(33, 19, [FR.ALL_IMAGES] * 2, images=images, samplers=[sampler], uv_size=[[1.0, 1.0], [6.0, 6.0]])
        FR.check(renderer, f, f"non power of two, {sampler}")


# ---- addressing -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [LIN_REP, LIN_CLAMP, NEAR_REP, NEAR_CLAMP], ids=FR.PRESETS[:4])
def test_addressing(renderer, sampler):
    """uv below 0 and above 1 (offset -3.5 and +2.25, size 2); uv on texel centres and on texel edges: the fronto-parallel quad over a
    16 x 16 frame puts pixel centres at (k + 0.5) / 16, the centres of the 16 x 16 level's texels, and an offset of half a texel moves them
    onto its edges."""
    scale = 4.0 * np.tan(np.radians(30.0)) / 3.0
    flat = [FR.view_matrix(0.0, scale)] * 4
    f = FR.frame(16, 16, [FR.ALL_IMAGES] * 4, mode="pixels", worlds=flat, samplers=[sampler], holes=False,
                 uv_size=[[2.0, 2.0], [2.0, 2.0], [1.0, 1.0], [1.0, 1.0]], uv_offset=[[-3.5, -3.5], [2.25, 2.25], [0.0, 0.0], [0.03125, 0.03125]])
    st = FR.check(renderer, f, "addressing")
    uv = st["uv"]
    assert (uv < 0).any() and (uv > 1).any()


# ---- normals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_normal_maps(renderer):
    """Flip-y on and off; a two-component map whose bytes reach x^2 + y^2 > 1; a chart with constant uv (jacobian_sign 0); a mirrored chart;
    normal.zw is the untextured decode's everywhere."""
    rg = FR.chain(16, 16, 5, TM.RG8, 31)
    rg["levels"][0][:4] = 255  # (1, 1): beyond the unit disc
    images = FR.five_images() + [rg]
    idx = np.tile(np.arange(5), (5, 1))
    idx[2:4, 1] = 5
    flags = [2, 2 | TM.FLIP_Y, 2 | TM.TWO_COMPONENT, 2 | TM.TWO_COMPONENT | TM.FLIP_Y, 2]
    meshes = [FR.quad_mesh(), FR.quad_mesh(uv=((0.5, 0.5),) * 4), FR.quad_mesh(uv=((1.0, 0.0), (0.0, 0.0), (0.0, 1.0), (1.0, 1.0)))]
    for mesh_of in ([0] * 5, [1] * 5, [2] * 5):
        f = FR.frame(33, 19, flags, mode="pixels", images=images, image_indices=idx, meshes=meshes, mesh_of=mesh_of)
        st = FR.check(renderer, f, f"normal maps, meshes {mesh_of}")
        assert st["sampled_normal"] == st["decoded"]
        assert (st["jacobian_zero"] == st["decoded"]) == (mesh_of[0] == 1) and (st["jacobian_zero"] == 0) == (mesh_of[0] != 1)
        got, plain = FR.want(f), FR.want(dataclasses.replace(f, images=[], samplers=[]))
        assert np.array_equal(got["normal"][..., 2:], plain["normal"][..., 2:])
        # with a zero Jacobian T and B are zero and the map only scales N; elsewhere it turns the normal
        assert mesh_of[0] == 1 or (got["normal"][..., :2] != plain["normal"][..., :2]).mean() > 0.5


# ---- divergence -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pixels", "bands", "mixed"])
def test_uniform_and_per_lane_waves(renderer, mode):
    """64 materials, each with its own sampler, uv transform and image order."""
    n = 64
    idx = np.array([np.roll(np.arange(5), m) for m in range(n)])
    f = FR.frame(48, 32, [FR.ALL_IMAGES] * n, mode=mode, samplers=[LIN_REP, LIN_CLAMP, NEAR_REP, NEAR_CLAMP], sampler_index=np.arange(n) % 5, image_indices=idx,
                 uv_size=[[1.0 + 0.125 * (m % 8), 2.0] for m in range(n)], worlds=[FR.view_matrix(0.3, 1.0)] * n)
    st = FR.check(renderer, f, mode)
    if mode == "pixels":
        assert st["uniform_waves"] == 0 and st["per_lane_waves"] == 24
    elif mode == "bands":
        assert st["uniform_waves"] == 24 and st["per_lane_waves"] == 0
    else:
        assert st["uniform_waves"] == 12 and st["per_lane_waves"] == 12


# ---- extents ----------------------------------------------------------------------------------------------------------------------------------------------
SWEEP = [(1, 1), (2, 1), (5, 3), (16, 16), (17, 9), (33, 19), (129, 65)]


@pytest.mark.parametrize("extent", SWEEP, ids=[f"{w}x{h}" for w, h in SWEEP])
@pytest.mark.parametrize("clear", [1, 0])
def test_extent_between_guard_bands(renderer, extent, clear):
    W, H = extent
    f = FR.frame(W, H, [FR.ALL_IMAGES, 3, 0, FR.ALL_IMAGES | TM.FLIP_Y], mode="mixed" if H >= 16 else "bands", clear=bool(clear), uv_size=[[2.0, 3.0]] * 4)
    outs = {"albedo": Guard("albedo_attachment", (H, W), torch.int32, W, OUT32, 4, fill=FR.POISON["albedo"]),
            "normal": Guard("normal_attachment", (H, W, 4), torch.int16, 4 * W, OUT16, 8, fill=FR.POISON["normal"]),
            "emissive": Guard("emissive_attachment", (H, W), torch.int32, W, OUT32, 4, fill=FR.POISON["emissive"]),
            "mro": Guard("metallic_roughness_occlusion_attachment", (H, W), torch.int32, W, OUT32, 4, fill=FR.POISON["mro"])}
    ctx, images, _gpu, _keep = FR.contexts(renderer, f, guards=outs)
    st = {}
    expected = FR.want(f, st, FR.init_images(f))
    for what in ("counting", "plain"):
        for g in outs.values():
            g.refill()
        if what == "counting":
            assert FR.counted(renderer, ctx, images) == TM.counters(st)
        else:
            renderer.decode_visbuffer_textured(ctx, images)
        same(decode_got_of(ctx), expected, f"{W} x {H}, clear {clear}, {what}")
        for g in outs.values():
            g.check(f"{W} x {H}, clear {clear}, {what}")
    assert st["decoded"] >= 1


# ---- alignment --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [4, 8, 12, 20])
def test_every_4_byte_alignment_of_the_image_base(renderer, offset):
    f = FR.frame(17, 9, [FR.ALL_IMAGES] * 2, uv_size=[[2.0, 2.0]] * 2)
    FR.check(renderer, f, f"base offset {offset}", image_offset=offset)


# ---- the frame in one graph -----------------------------------------------------------------------------------------------------------------------------
def test_draw_to_pbr_in_one_graph_with_an_image_rewritten_between_replays(renderer):
    """draw -> textured decode -> resolve -> contact shadows -> ambient occlusion -> PBR captured once and replayed three times; between
    replays the texels of material 1's albedo image are rewritten: the lit image changes where material 1 is drawn and nowhere else."""
    from gpu_passes import ALL_FLAGS, pbr_got_of
    from oxylus_amd.renderer import MaterialImagesContext, pack_material_samplers

    fr = DrawnFrame(renderer)
    gpu = fr.f.gpu
    words = gpu.materials.view(torch.int32).view(-1, 14)
    words[1, 5], words[1, 7], words[1, 12] = 1, 0, 0x3C003C00  # HasAlbedoImage, image 0, uv_size (1, 1); the spheres carry no texcoords: uv (0, 0)
    image = FR.chain(2, 2, 2, TM.SRGB, 41)
    rec, keep = FR.upload_images([image])
    images = MaterialImagesContext.create(fr.cpu.camera["position"], rec, pack_material_samplers(["LinearRepeated"]))
    pbr = fr.pbr(ALL_FLAGS, None)

    def passes(stream=None):
        r, f = fr.r, fr.f
        r.prepared_frame = fr.frame
        r.draw_visbuffer(fr.main, fr.pv, fr.W, fr.H, fr.visdepth, clear=True, depth=fr.depth_image, visbuffer=fr.vis, stream=stream)
        r.decode_visbuffer_textured(fr.dctx, images, stream=stream)
        r.resolve_shadowmap(f.rctx, stream=stream)
        r.contact_shadows(fr.cctx, stream=stream)
        r.generate_ambient_occlusion(fr.actx, stream=stream)
        r.apply_pbr(pbr, stream=stream)

    passes()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        passes(s)
    lit = []
    for replay in range(3):
        keep[0].copy_(torch.full_like(keep[0], (40, 140, 250)[replay]))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        lit.append(pbr_got_of(pbr).copy())
    vis = fr.vis.cpu().numpy().view(np.uint32)
    mli = fr.cpu.meshlet_instances.numpy().reshape(-1, 2)
    inst = np.minimum(vis >> 8, len(mli) - 1)
    material = fr.cpu.mesh_instances.numpy().reshape(-1, 5)[mli[inst, 0], 2]
    drawn = (fr.f.depth.cpu().numpy() != 0) & (material == 1)
    assert drawn.sum() > 100
    for a, b in ((0, 1), (1, 2)):
        changed = (lit[a] != lit[b]).reshape(fr.H, fr.W, -1).any(axis=-1)
        assert not (changed & ~drawn).any() and changed[drawn].mean() > 0.9, (int((changed & ~drawn).sum()), float(changed[drawn].mean()))


# ---- invalid arguments ------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import MaterialImagesContext

    f = FR.frame(24, 16, [FR.ALL_IMAGES] * 2)
    ctx, images, gpu, _keep = FR.contexts(renderer, f)
    outputs = ("albedo_attachment", "normal_attachment", "emissive_attachment", "metallic_roughness_occlusion_attachment")
    W, H = 24, 16
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    bad_ctx = [dict(visbuffer_attachment=None), dict(visbuffer_attachment=i32(H - 1, W)), dict(materials_buffer=None), dict(meshlet_instance_count=gpu.n_meshlet_instances + 1),
               dict(normal_attachment=torch.zeros(H * W * 4 + 2, dtype=torch.int16, device="cuda")[2:])] + [{n: None} for n in outputs]
    rec, smp = images.images_buffer, images.samplers_buffer
    bad_img = [dict(images_buffer=None), dict(samplers_buffer=None), dict(images_buffer=rec[:144 * 4]), dict(samplers_buffer=smp.view(-1)[:3]),
               dict(images_buffer=torch.cat([rec[:4], rec])[4:]), dict(samplers_buffer=torch.cat([smp.view(torch.uint8).view(-1)[:2], smp.view(torch.uint8).view(-1)])[2:], sampler_count=1)]

    def refused(c, m):
        with pytest.raises(L.OxcError) as e:
            renderer.decode_visbuffer_textured(c, m)
        assert e.value.status == L.OXC_INVALID_ARG and "decode_visbuffer_textured: " in str(e.value)

    for kw in bad_ctx:
        refused(dataclasses.replace(ctx, **kw), images)
    for kw in bad_img:
        refused(ctx, dataclasses.replace(images, **kw))
    for a, b in itertools.product(bad_ctx[:4], bad_img[:4]):  # in pairs
        refused(dataclasses.replace(ctx, **a), dataclasses.replace(images, **b))
    lib, raw, stream = renderer._lib, renderer._ctx, renderer._stream(None)
    pf = renderer.prepared_frame.c()
    m = images.c()
    m.struct_size = 8
    assert lib.oxc_decode_visbuffer_textured(raw, pf, ctx.c(), m, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.struct_size = 4
    assert lib.oxc_decode_visbuffer_textured(raw, pf, c, images.c(), stream) == L.OXC_INVALID_ARG
    assert lib.oxc_decode_visbuffer_textured(raw, pf, ctx.c(), None, stream) == L.OXC_INVALID_ARG
    assert lib.oxc_decode_visbuffer_textured(raw, None, ctx.c(), images.c(), stream) == L.OXC_INVALID_ARG
    torch.cuda.synchronize()
    assert all((getattr(ctx, n) == -5).all() for n in outputs)  # nothing was launched
    # counts of zero: the buffers are not looked at
    renderer.decode_visbuffer_textured(ctx, MaterialImagesContext(FR.CAMERA, None, None, 0, 0))
    same(decode_got_of(ctx), FR.want(dataclasses.replace(f, images=[], samplers=[]), None, FR.init_images(f)), "empty tables")
