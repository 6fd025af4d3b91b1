"""oxc_decode_visbuffer on the GPU: the four G-buffer images byte-identical to tests/visbuffer_decode_model.py, every pixel -- a frame drawn by
oxc_draw_visbuffer with smooth and flat normals, five materials and sky; an odd extent under a rotated camera; tiny extents between poisoned
guard bands with and without `clear`; a hand-made visbuffer whose texels reach every rule that keeps a read inside its buffer; odd material
halves and degenerate triangles; draw -> decode -> resolve -> contact shadows -> ambient occlusion captured into one graph; invalid arguments."""
import dataclasses

import numpy as np
import pytest
import torch

import visbuffer_decode_model as VD
from gpu_passes import DrawnFrame, Guard, ao_check, ao_got_of, contact_check, contact_got_of
from gpu_passes import decode_check as check
from gpu_passes import decode_context as context
from gpu_passes import decode_got_of as got_of
from gpu_passes import same
from scenes import DECODE_MAIN_SIZE as MAIN_SIZE
from scenes import NAN32, OUT16, OUT32, build_scene
from scenes import decode_assert_not_degenerate as assert_not_degenerate
from scenes import main_scene, rotated_camera

pytestmark = pytest.mark.gpu

SWEEP = [(1, 1), (2, 1), (5, 3), (16, 16), (17, 9), (129, 65)]
POISON = {"albedo": 0xFFFFFFFB, "normal": 0xFFFB, "emissive": 0xFFFFFFFB, "mro": 0xFFFFFFFB}  # what an output holds before a call with clear = 0


def draw(r, cpu, W, H):
    """`cpu` culled and drawn by oxc_draw_visbuffer with its own camera: (gpu scene, vis int32 [H, W], depth float32 [H, W], cull context, visdepth).
    Leaves the scene's PreparedFrame as r.prepared_frame."""
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame

    gpu = cpu.to("cuda")
    r.reserve(gpu.n_mesh_instances, gpu.n_meshlet_instances)
    r.prepared_frame = PreparedFrame.create(gpu)
    main = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=gpu.cull_camera())
    r.seed_meshlet_instances(main, gpu.n_meshlet_instances)
    r.cull_geometry(main)
    visdepth = torch.empty((H, W), dtype=torch.int64, device="cuda")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    vis = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    r.draw_visbuffer(main, cpu.camera["projection_view"], W, H, visdepth, clear=True, depth=ImageAttachment.depth(depth), visbuffer=vis)
    torch.cuda.synchronize()
    return gpu, vis, depth, main, visdepth


def counted(r, ctx):
    """One call with the counting instantiation: the device's counters."""
    from oxylus_amd import lib as L

    r.debug_set_tuning(L.TUNE_VISBUFFER_DECODE_STATS, 1)
    try:
        r.decode_visbuffer(ctx)
        return r.debug_visbuffer_decode_stats()
    finally:
        r.debug_set_tuning(L.TUNE_VISBUFFER_DECODE_STATS, 0)


# ---- 1. the drawn frame ------------------------------------------------------------------------------------------------------------------------
def test_drawn_frame(renderer):
    """main_scene() drawn at 256 x 256: all four images == checker, the device's counters == the checker's, and the frame is not degenerate
    by the floors of tests/test_visbuffer_decode_model.py (>= 30 % decoded, >= 5 % empty, >= 200 triangles, >= 4 materials, >= 1000 distinct
    .rg values), judged by the checker on the device-drawn frame.  On the oracle-drawn frame the checker reaches: 44 083 decoded, 21 453 empty,
    1 331 triangles, 6 materials, 22 478 .rg values."""
    cpu, _ = main_scene()
    gpu, vis, depth, _, _ = draw(renderer, cpu, MAIN_SIZE, MAIN_SIZE)
    ctx = context(gpu, vis, depth, cpu.camera["projection_view"])
    dev = counted(renderer, ctx)
    st = {}
    got = check(ctx, cpu, st)
    figures = assert_not_degenerate(st, got, vis.numel())
    print("checker", figures, VD.counters(st))
    print("device", dev)
    assert dev == VD.counters(st)
    assert st["default_material"] > 0 and (got["emissive"] != 0).any()
    for t in (ctx.albedo_attachment, ctx.normal_attachment, ctx.emissive_attachment, ctx.metallic_roughness_occlusion_attachment):
        t.fill_(-5)
    renderer.decode_visbuffer(ctx)  # the plain instantiation writes the same images
    check(ctx, cpu)


# ---- 2. odd extent, rotated camera ---------------------------------------------------------------------------------------------------------------
def rotated(cpu):
    """`cpu` seen by the rotated camera of tests/test_gpu_contact_shadows.py."""
    _, view, proj, near = rotated_camera()
    pv = (proj.astype(np.float64).reshape(4, 4).T @ view.astype(np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    cpu.camera = dict(cpu.camera, projection_view=[float(x) for x in pv], position=[3.0, 1.5, -2.0], near_clip=near)
    return cpu


def test_odd_extent_rotated_camera(renderer):
    cpu = rotated(main_scene()[0])
    gpu, vis, depth, _, _ = draw(renderer, cpu, 77, 45)
    ctx = context(gpu, vis, depth, cpu.camera["projection_view"])
    renderer.decode_visbuffer(ctx)
    st = {}
    check(ctx, cpu, st)
    assert st["decoded"] > 500 and st["empty"] > 100 and st["distinct_triangles"] > 50, {k: st[k] for k in ("decoded", "empty", "distinct_triangles")}


# ---- 3. extent sweep between guard bands -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", SWEEP, ids=[f"{w}x{h}" for w, h in SWEEP])
@pytest.mark.parametrize("clear", [1, 0])
def test_extent_between_guard_bands(renderer, extent, clear):
    """Every image a window between poisoned bands: the inputs' bands hold patterns that change the result when read (an instance in range
    for the visbuffer, NaN for the depth), the outputs' bands must stay untouched.  clear = 0: the empty pixels inside the window keep
    what they held."""
    from oxylus_amd.renderer import ImageAttachment

    W, H = extent
    cpu = rotated(main_scene()[0]) if extent in ((5, 3), (17, 9)) else main_scene()[0]
    gpu, vis, depth, _, _ = draw(renderer, cpu, W, H)
    vis_g = Guard("visbuffer_attachment", (H, W), torch.int32, W, 0x00000101, 4, data=vis.cpu().numpy())
    depth_g = Guard("depth_attachment", (H, W), torch.float32, W, NAN32, 4, data=depth.cpu().numpy())
    outs = {"albedo": Guard("albedo_attachment", (H, W), torch.int32, W, OUT32, 4, fill=POISON["albedo"]),
            "normal": Guard("normal_attachment", (H, W, 4), torch.int16, 4 * W, OUT16, 8, fill=POISON["normal"]),
            "emissive": Guard("emissive_attachment", (H, W), torch.int32, W, OUT32, 4, fill=POISON["emissive"]),
            "mro": Guard("metallic_roughness_occlusion_attachment", (H, W), torch.int32, W, OUT32, 4, fill=POISON["mro"])}
    ctx = context(gpu, vis_g.tensor, ImageAttachment.depth(depth_g.tensor), cpu.camera["projection_view"], clear=bool(clear))
    ctx.albedo_attachment, ctx.normal_attachment = outs["albedo"].tensor, outs["normal"].tensor
    ctx.emissive_attachment, ctx.metallic_roughness_occlusion_attachment = outs["emissive"].tensor, outs["mro"].tensor
    init = {"albedo": np.full((H, W), POISON["albedo"], np.uint32), "normal": np.full((H, W, 4), POISON["normal"], np.uint16),
            "emissive": np.full((H, W), POISON["emissive"], np.uint32), "mro": np.full((H, W), POISON["mro"], np.uint32)}
    label = f"{W} x {H}, clear = {clear}"
    for what in ("counting", "plain"):
        for g in outs.values():
            g.refill()
        if what == "counting":
            dev = counted(renderer, ctx)
        else:
            renderer.decode_visbuffer(ctx)
        st = {}
        got = check(ctx, cpu, st, init, f"{label}, {what}: ")
        for g in list(outs.values()) + [vis_g, depth_g]:
            g.check(f"{label}, {what}")
        if what == "counting":
            assert dev == VD.counters(st), (label, dev, VD.counters(st))
    assert st["decoded"] >= 1, (label, st["decoded"])
    if W * H > 2:
        assert st["empty"] >= 1, (label, st["empty"])
    if not clear and st["empty"]:
        assert (got["albedo"] == POISON["albedo"]).sum() == st["empty"] and (got["normal"] == POISON["normal"]).all(axis=-1).sum() == st["empty"]


# ---- 4. / 5. hand-made visbuffers over a tiny scene ------------------------------------------------------------------------------------------------
NAN_H, INF_H, NINF_H, NEG_H, DEN_H, NDEN_H, NZERO_H, TWO_H, MAX_H, ONE_H, HALF_H = 0x7E00, 0x7C00, 0xFC00, 0xBC00, 0x0001, 0x83FF, 0x8000, 0x4000, 0x7BFF, 0x3C00, 0x3800


def odd_materials():
    """Eight materials whose halves are NaN, +-Inf, negative, denormal, -0, above 1 and the largest half, in albedo, emissive and the factors."""
    from oxylus_amd.synth import pack_materials

    albedo = [[ONE_H, HALF_H, 0x2E66, ONE_H], [NAN_H, INF_H, NINF_H, NAN_H], [NEG_H, DEN_H, NDEN_H, INF_H], [NZERO_H, TWO_H, MAX_H, NEG_H],
              [0x1A6A, 0x1A69, 0x1A6B, DEN_H], [HALF_H, 0x0400, 0x3BFF, TWO_H], [0x7DFF, 0xFE00, 0x0000, NZERO_H], [MAX_H, MAX_H, MAX_H, MAX_H]]
    emissive = [[ONE_H, TWO_H, HALF_H], [NAN_H, INF_H, NINF_H], [NEG_H, DEN_H, NDEN_H], [NZERO_H, MAX_H, MAX_H], [0x0400, 0x0400, 0x0400],
                [0x0200, 0x03FF, 0x0200], [0x7BFF, 0x7800, 0x7801], [0x3555, 0x0801, 0x57FF]]
    roughness = [HALF_H, NAN_H, INF_H, NEG_H, DEN_H, NZERO_H, TWO_H, 0x3BFF]
    metallic = [ONE_H, NINF_H, NAN_H, NDEN_H, MAX_H, 0x1C04, 0x2004, 0x3801]
    return pack_materials(np.array(albedo), np.array(emissive), roughness=np.array(roughness), metallic=np.array(metallic))


def tiny_scene():
    """One mesh, one meshlet of two triangles (a quad at z = -4 in front of the identity-view camera, smooth normals), plus what the hand-made
    texels name: meshlet 1 whose third vertex index equals vertex_count, meshlet 2 a zero-area triangle (two equal corners), meshlet 3 a
    triangle whose third corner is vertex 4 = (1, 1, -2^-14), mesh 1 = mesh 0 with vertex_count 0, mesh 2 = mesh 0 with a null vertex_normals.
    Mesh instances: 0..7 on mesh 0 with materials 0..7, 8 on mesh 1, 9 on mesh 2, 10 on mesh 0 with material_index = material_count, all under
    a shear; 11 on mesh 0 under the identity, so that vertex 4 keeps its z and its clip w is 2^-14 under the identity-view camera.
    MeshletInstance records: i < 11 -> (mesh instance i, meshlet 0); 11, 12, 13 -> (mesh instance 0, meshlet 1 / 2 / 3); 14 -> (mesh
    instance 11, meshlet 3): the corner with w near 0."""
    pos = np.array([[-3.0, -3.0, -4.0], [3.0, -3.0, -4.0], [3.0, 3.0, -4.0], [-3.0, 3.0, -4.0], [1.0, 1.0, -2.0 ** -14]], dtype=np.float32)
    nrm = np.array([[-0.5, -0.5, 0.7], [0.5, -0.5, 0.7], [0.5, 0.5, 0.7], [-0.5, 0.5, 0.7], [0.0, 0.0, 1.0]], dtype=np.float32)
    world = np.eye(4)
    world[:3, :3] = [[1.0, 0.25, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 2.0]]  # a shear: the cofactor matrix is not the matrix
    world[:3, 3] = [0.25, -0.5, -1.0]
    s, _ = build_scene([(pos, np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]]), nrm)],
                       [(0, world, m) for m in range(8)] + [(0, world, 0), (0, world, 1), (0, world, 8), (0, np.eye(4), 0)], odd_materials())
    V = pos.shape[0]
    assert s.meshlets.shape[0] == 1 and s.vidx.tolist() == [0, 1, 2, 3, 4] and s.micro.tolist()[:9] == [0, 1, 2, 0, 2, 3, 0, 1, 4]
    s.meshlets[0, 3] = 2
    nv, nm = s.vidx.numel(), s.micro.numel()
    s.meshlets = torch.cat([s.meshlets, torch.tensor([[nv, nm, 3, 1], [nv + 3, nm, 3, 1], [0, 6, 5, 1]], dtype=torch.int32)])
    s.vidx = torch.cat([s.vidx, torch.tensor([0, 1, V, 0, 0, 1], dtype=torch.int32)])
    s.micro = torch.cat([s.micro, torch.tensor([0, 1, 2, 0], dtype=torch.uint8)])
    s.bounds = s.bounds.repeat(4, 1)
    s.meshes, s.lods, s.n_meshes = s.meshes.repeat(3, 1), s.lods.repeat(3, 1), 3
    s._lod_tables = {k: v.repeat(3) for k, v in s._lod_tables.items()}
    s.mesh_instances[8, 0], s.mesh_instances[9, 0] = 1, 2
    s.meshlet_instances = torch.cat([s.meshlet_instances[:11], torch.tensor([[0, 1], [0, 2], [0, 3], [11, 3]], dtype=torch.int32)])
    assert s.meshlet_instances.shape[0] == 15
    return patch_tiny(s.bind())


def patch_tiny(s):
    """What Scene.bind() writes for every mesh alike: mesh 1's vertex_count is 0, mesh 2's vertex_normals is null."""
    s.meshes.view(torch.int32)[1, 6] = 0
    s.meshes[2, 1] = 0
    return s


def hand_made(r, texels, depth_bits, W, H, clear, count=15):
    """The tiny scene decoded from a hand-made visbuffer: (ctx, cpu scene, init images)."""
    from oxylus_amd.renderer import PreparedFrame

    cpu = tiny_scene()
    gpu = patch_tiny(cpu.to("cuda"))
    r.prepared_frame = PreparedFrame.create(gpu)
    vis = torch.from_numpy(np.asarray(texels, dtype=np.uint32).view(np.int32).reshape(H, W).copy()).cuda()
    depth = torch.from_numpy(np.asarray(depth_bits, dtype=np.uint32).view(np.float32).reshape(H, W).copy()).cuda()
    ctx = dataclasses.replace(context(gpu, vis, depth, cpu.camera["projection_view"], clear=bool(clear)), meshlet_instance_count=count)
    init = {}
    for k, t in (("albedo", ctx.albedo_attachment), ("normal", ctx.normal_attachment), ("emissive", ctx.emissive_attachment), ("mro", ctx.metallic_roughness_occlusion_attachment)):
        t.fill_(-5)
        init[k] = np.full(tuple(t.shape), POISON[k], np.uint16 if k == "normal" else np.uint32)
    return ctx, cpu, init


@pytest.mark.parametrize("clear", [0, 1])
def test_hand_made_texels_stay_inside_their_buffers(renderer, clear):
    """Every texel resolves to reads inside the buffers the test allocated, by rules 1 and 2 of the header: ~0u, the terrain id, depth bits 0
    under vis 0, an instance index equal to meshlet_instance_count and one far beyond (with 15 records allocated and 12 declared, the
    records 12 and 13 are 'beyond' too), a vertex index equal to vertex_count (zeros, also with clear = 0), vertex_count = 0, a material index
    equal to material_count, a null vertex_normals."""
    W, H, count = 8, 3, 12
    ONE = 0x3F000000  # depth 0.5
    texels = [0xFFFFFFFF, (0xFFFFFE << 8) | 3, 0, count << 8, (0xABCDE << 8) | 1, (11 << 8), (8 << 8) | 1, (10 << 8),
              (9 << 8), (9 << 8) | 1, (12 << 8), (13 << 8), 0xFFFFFD00, (0xFFFFFE << 8), 1, (8 << 8)] + [(k << 8) | (k & 1) for k in range(8)]
    bits = [ONE] * len(texels)
    bits[2] = 0
    bits[14] = 0x80000000  # -0.0 is not the cleared state
    ctx, cpu, init = hand_made(renderer, texels, bits, W, H, clear, count)
    dev = counted(renderer, ctx)
    st = {}
    got = check(ctx, cpu, st, init)
    assert dev == VD.counters(st)
    assert (st["empty_clear_value"], st["empty_terrain"], st["empty_depth_zero"], st["empty_instance_range"]) == (1, 2, 1, 5)
    assert st["zero_vertex_index"] == 1 and st["default_material"] == 1 and st["decoded"] == 14
    flat = {k: v.reshape(W * H, -1) for k, v in got.items()}
    assert all((flat[k][5] == 0).all() for k in VD.IMAGES)                      # the out-of-range vertex index is written as zeros
    assert (flat["normal"][8] == 0x7E00).all() and (flat["normal"][9] == 0x7E00).all()  # null vertex_normals: normalize(0) is NaN
    assert flat["albedo"][7, 0] == 0 and flat["mro"][7, 0] == 0x00FF0000 and flat["emissive"][7, 0] == 0  # the default Material
    for p in (0, 1, 2, 3, 4, 10, 11, 12, 13):
        assert all((flat[k][p] == (0 if clear else POISON[k])).all() for k in VD.IMAGES), p


def test_odd_material_halves_and_degenerate_triangles(renderer):
    """Materials 0..7 of odd_materials() on both triangles of the quad; the zero-area triangle (inv_det is infinite: NaN lambda, NaN normal);
    and the triangle with a corner at w near 0, placed by hand: under the identity world matrix vertex 4 has clip w = 2^-14 exactly (asserted
    from the checker's clip positions), inv_w = 16384 and an ndc of about 28 000 while the other two corners sit at w = 4."""
    W, H = 8, 3
    texels = [(k << 8) | t for t in (0, 1) for k in range(8)] + [(12 << 8), (13 << 8), (14 << 8), (14 << 8), (3 << 8), (6 << 8) | 1, (14 << 8), (12 << 8)]
    ctx, cpu, init = hand_made(renderer, texels, [0x3F000000] * len(texels), W, H, 1)
    renderer.decode_visbuffer(ctx)
    st = {}
    got = check(ctx, cpu, st, init)
    assert st["decoded"] == W * H and st["distinct_materials"] == 8
    near = [p for p in range(W * H) if texels[p] == (14 << 8)]
    w = {int(st["ys"][i]) * W + int(st["xs"][i]): st["clip"][i, :, 3] for i in range(st["decoded"])}
    assert len(near) == 3 and all(float(w[p][2]) == 2.0 ** -14 and float(w[p][0]) == 4.0 and float(w[p][1]) == 4.0 for p in near), [w[p] for p in near]
    normal = got["normal"].reshape(W * H, 4)
    assert (normal[16] == 0x7E00).all() and not (normal[:16] == 0x7E00).any() and not (normal[near] == 0x7E00).any()
    assert len({tuple(normal[p]) for p in near}) == 3  # three pixels, three different interpolated normals: lambda is not degenerate there
    a1 = int(got["albedo"].reshape(-1)[1])  # NaN, +Inf, -Inf, NaN
    assert (a1 & 0xFF, (a1 >> 8) & 0xFF, (a1 >> 16) & 0xFF, a1 >> 24) == (0, 255, 0, 0)
    e1 = int(got["emissive"].reshape(-1)[1])  # NaN, +Inf, -Inf
    assert (e1 & 0x7FF, (e1 >> 11) & 0x7FF, e1 >> 22) == (0x7FF, 31 << 6, 0)


# ---- 6. one captured graph ---------------------------------------------------------------------------------------------------------------------
def test_draw_decode_resolve_contact_ambient_in_one_graph(renderer):
    """Draw -> decode -> resolve -> contact shadows -> ambient occlusion captured into one graph and replayed twice: the decode's normal image
    feeds the resolve and the ambient occlusion, every output equals its checker.  Captured with the default queue settings."""
    frame = DrawnFrame(renderer)
    W, H, cpu, f = frame.W, frame.H, frame.cpu, frame.f
    vis, dctx, cctx, actx, passes = frame.vis, frame.dctx, frame.cctx, frame.actx, frame.passes

    passes()
    st = {}
    decoded = check(dctx, cpu, st)
    assert st["decoded"] > 0.3 * W * H and st["distinct_materials"] >= 4
    resolved, contact, ao = f.check(), contact_check(cctx), ao_check(actx)
    assert ((resolved > 0) & (resolved < 1)).any() and ((contact > 0) & (contact < 1)).any()
    depth_before = f.depth.clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        passes(s)
    outputs = (vis, f.depth, dctx.albedo_attachment, dctx.normal_attachment, dctx.emissive_attachment, dctx.metallic_roughness_occlusion_attachment,
               f.rctx.resolved_shadows_attachment.data, cctx.contact_shadows_attachment.data, actx.depth_differences, actx.noisy_occlusion,
               actx.ambient_occlusion_attachment, actx.prefiltered_depth.data)
    for replay in range(2):
        for t in outputs:
            t.fill_(-5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        bad = int((f.depth.view(torch.int32) != depth_before.view(torch.int32)).sum())
        assert bad == 0, f"replay {replay}: {bad} of {W * H} depth texels differ from the eager draw's"
        same(got_of(dctx), decoded)
        assert np.array_equal(f.got().view(np.uint32), resolved.view(np.uint32))
        assert np.array_equal(contact_got_of(cctx).view(np.uint32), contact.view(np.uint32))
        same(ao_got_of(actx), ao)


# ---- 7. invalid arguments ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    W, H = 24, 16
    cpu, _ = main_scene()
    gpu, vis, depth, _, _ = draw(renderer, cpu, W, H)
    ctx = context(gpu, vis, depth, cpu.camera["projection_view"])
    outputs = ("albedo_attachment", "normal_attachment", "emissive_attachment", "metallic_roughness_occlusion_attachment")
    for name in outputs:
        getattr(ctx, name).fill_(-5)

    def bad(**kw):
        c = dataclasses.replace(ctx, **kw)
        with pytest.raises(L.OxcError) as e:
            renderer.decode_visbuffer(c)
        assert e.value.status == L.OXC_INVALID_ARG, kw
        assert "decode_visbuffer: " in str(e.value)

    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    for name in outputs:
        short = torch.zeros((H - 1, W, 4), dtype=torch.int16, device="cuda") if name == "normal_attachment" else i32(H - 1, W)
        bad(**{name: None})
        bad(**{name: short})
    bad(normal_attachment=torch.zeros(H * W * 4 + 2, dtype=torch.int16, device="cuda")[2:])  # 4-byte aligned only
    bad(visbuffer_attachment=None)
    bad(visbuffer_attachment=i32(H - 1, W))
    bad(materials_buffer=None)
    bad(materials_buffer=gpu.materials[:4 * 56])
    bad(depth_attachment=ImageAttachment(depth.view(-1)[:0], 0, 0, 1, [0]))  # zero extent
    bad(depth_attachment=ImageAttachment.depth(torch.zeros((H + 1, W), dtype=torch.float32, device="cuda")))  # every buffer holds H x W texels
    bad(depth_attachment=ImageAttachment(depth.view(-1), W, H, 2, [0, 4 * W * H]))  # two levels
    bad(meshlet_instance_count=gpu.n_meshlet_instances + 1)
    lib, raw, stream = renderer._lib, renderer._ctx, renderer._stream(None)
    f = renderer.prepared_frame.c()
    c = ctx.c()
    c.struct_size = 4
    assert lib.oxc_decode_visbuffer(raw, f, c, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.width += 1  # the visbuffer's extent differs from the depth's
    assert lib.oxc_decode_visbuffer(raw, f, c, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.width = c.height = 0
    assert lib.oxc_decode_visbuffer(raw, f, c, stream) == L.OXC_INVALID_ARG
    c = ctx.c()
    c.depth_attachment.dptr = None
    assert lib.oxc_decode_visbuffer(raw, f, c, stream) == L.OXC_INVALID_ARG
    assert lib.oxc_decode_visbuffer(raw, None, ctx.c(), stream) == L.OXC_INVALID_ARG
    torch.cuda.synchronize()
    assert all((getattr(ctx, name) == -5).all() for name in outputs)  # nothing was launched
    renderer.decode_visbuffer(ctx)  # and the context still runs
    check(ctx, cpu)
