"""oxc_cull_terrain (k_cull_terrain_test, k_cull_terrain_emit and the host part) at its own switch-overs: the patch counts either side of
the word, wave and block seams, the emit kernel's second stride iteration, every HiZ shape of hiz_frames.SHAPES in both layouts, all eight
flag sets, non-finite and inverted boxes, a mask that lives on the GPU across frames, the meshlet stage's borrowed scratch, graph capture
and the argument checks.  Every comparison is byte equality with the checker (oracle.cull_terrain): the emitted list, the command
[4, count, 0, 0], every mask word with its guard words, and the visible buffer beyond the count, which keeps its fill.  What the fixtures
have to hold is asserted without a GPU in tests/test_terrain_cull_frames.py ("Terrain cull shapes pinned by the tests").
No fault was found: the kernel, the host function and the checker agree on every case below."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import hiz_frames
from hiz_frames import LAYOUTS, POISON, SHAPE_BY_ID, SHAPES, cell_depth, inside_mask, oracle_pyramid
from oxylus_amd import lib as L
from refusals import raises_refusal
from terrain_cull_frames import (EDGE_CASES, FLAG_SETS, FRUSTUM, GUARD_WORDS, LATE, MASK_GUARD, OCCLUSION, PASSES, SEAM_GRIDS, VISIBLE_FILL, World, _camera, _mask,
                                 _terrain, assert_call, assert_exercised, checker, collect, edge_case, edge_minmax, enqueue, flag_classes, flag_frame, guarded, mask_words,
                                 random_words, read_cmd, run, shape_frame, shape_report, shape_want, small_pyramid, terrain_context, two_pass_want, visible_allocation)

pytestmark = pytest.mark.gpu


def _two_passes(renderer, world, mm, cam, hiz, mask, lists, masks, what):
    """Early then late with TEST_ALL on one GPU mask; each call against the checker's list and mask."""
    mm_gpu, alloc = mm.cuda(), guarded(mask)
    for flags, want, want_mask, tag in zip(PASSES, lists, masks, ("early", "late")):
        assert_call(run(renderer, flags, cam, world, mm_gpu, alloc, hiz), want, want_mask, f"{what} {tag}")


# ---- a. patch-count seams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", SEAM_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_patch_count_seams(renderer, oracle_lib, grid):
    """1, 31 / 32 / 33 (the word seam of the mask write), 63 / 64 / 65 (the wave seam, where lane 32 has ok == 0), 1023 / 1024 / 1025 (one block
    appends in the test kernel, the second block of 1025 holds one patch), 1088 (a multiple of 64 but not of 1024), 2048 / 2049.  The mask is
    random in all 32 bits of every word: the bits past the total and the guard words come back unchanged (the checker never touches them).
    The terrain kernels run outside the profile counters, so which form ran is the launch rule restated: one block appends in the test kernel."""
    world = World(grid)
    mm, mask, lists, masks = two_pass_want(world, 100 + grid[0], 7, True)
    blocks = (world.total + 1023) // 1024
    assert (blocks == 1) == (world.total <= 1024)  # launch_cull_terrain: blocks <= 1 is the fused form, anything else test + emit
    _two_passes(renderer, world, mm, _camera(), small_pyramid(), mask, lists, masks, f"{grid}")
    tail = world.total % 32
    if tail:  # the bits past the total, spelled out
        assert (int(masks[1][-1]) ^ int(mask[-1])) >> tail == 0


# ---- b. the emit kernel's second stride iteration ---------------------------------------------------------------------------------------------
def test_emit_prefix_loop_runs_twice(renderer, oracle_lib):
    """1100 x 1000 patches are 1075 blocks: blocks 1025 .. 1074 of k_cull_terrain_emit sum their prefix in two iterations of the stride loop."""
    world = World((1100, 1000))
    mm, mask, lists, masks = two_pass_want(world, 5, 7, False)
    assert (world.total + 1023) // 1024 == 1075 and all(0 < l.numel() < world.total for l in lists)
    _two_passes(renderer, world, mm, _camera(), small_pyramid(), mask, lists, masks, "1100 x 1000")


# ---- c. HiZ shapes ----------------------------------------------------------------------------------------------------------------------------
def _relaid(pyr, layout):
    out = pyr.relaid(layout)
    if layout == "reordered":
        gaps = ~inside_mask(out.w, out.h, out.levels, out.offs, out.data.numel())
        assert gaps.sum() >= (out.levels + 1) * (out.w + 64) and (out.data.numpy()[gaps] == POISON).all()
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape_id", [s.id for s in SHAPES])
def test_hiz_shapes(renderer, oracle_lib, shape_id, layout):
    """Every level comes from global memory here (lds_first = levels).  The reordered layout's gaps hold -1.0: a stray tap shows a box."""
    rep = shape_report(shape_id)
    assert_exercised(SHAPE_BY_ID[shape_id], rep)
    world, mm, cam, pyr, mask = shape_frame(shape_id)
    lists, masks = shape_want(shape_id)
    _two_passes(renderer, world, mm, cam, _relaid(pyr, layout), mask, lists, masks, f"{shape_id} {layout}")
    print(f"\n{shape_id} {layout}: early {lists[0].numel()}, late {lists[1].numel()}, occluded {rep['removed']} of {rep['survivors']}")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_hiz_thirteen_levels_accepted(renderer, oracle_lib, layout):
    """4096 x 2 has the full 13 levels, the most s_level_off holds."""
    w, h, levels = 4096, 2, 13
    pyr = oracle_pyramid(cell_depth(2 * w + 1, 2 * h + 1, seed=3, cell=64, dist=(30.0, 800.0)), w, h, levels)
    world, mm, cam, mask = World((64, 64)), _terrain(64, 64, 164), _camera(eye=(0.0, 25.0, 0.0)), _mask(4096, 7, 0.35)
    m, lists, masks = mask.clone(), [], []
    for flags in PASSES:
        lists.append(checker(world, mm, cam, flags, pyr.struct(), m))
        masks.append(m.clone())
    assert all(0 < l.numel() < 4096 for l in lists)
    _two_passes(renderer, world, mm, cam, _relaid(pyr, layout), mask, lists, masks, f"4096 x 2 {layout}")


def _refused(renderer, flags, world, mm_gpu, hiz=None, tweak=None, message=None, cam=None):
    """A call that must return OXC_INVALID_ARG and write nothing: the mask, the visible buffer and their guard words keep their bytes."""
    mask = random_words(world.total, 21)
    alloc, vis = guarded(mask), visible_allocation(world.total)
    raises_refusal(lambda: run(renderer, flags, cam or _camera(), world, mm_gpu, alloc, hiz, visible_alloc=vis, tweak=tweak), message or "")
    assert torch.equal(alloc.cpu(), guarded(mask, "cpu")) and bool((vis == VISIBLE_FILL).all())


def test_hiz_fourteen_levels_refused(renderer):
    """8192 x 1 has 14 levels, one more than the kernel's offset table: OXC_INVALID_ARG, nothing written."""
    data = torch.zeros(2 * 8192 + 64, device="cuda")
    im = L.Image()
    im.dptr, im.width, im.height, im.levels = data.data_ptr(), 8192, 1, 14
    off = 0
    for k in range(13):  # (the struct holds 13 offsets; the call has to be refused before it reads any)
        im.level_offset[k] = 4 * off
        off += max(1, 8192 >> k)
    world = World((33, 31))
    mm_gpu = _terrain(33, 31, 1).cuda()
    for flags in (L.CULL_TEST_ALL, FRUSTUM | LATE, OCCLUSION):
        _refused(renderer, flags, world, mm_gpu, hiz=im, message="hiz_attachment")
    im.levels = 13  # the same image with 13 levels is taken
    run(renderer, L.CULL_TEST_ALL, _camera(), world, mm_gpu, guarded(random_words(world.total, 21)), im)


def test_frustum_only_runs_without_a_pyramid(renderer, oracle_lib):
    world = World((41, 25))
    mm, mask = _terrain(41, 25, 8), _mask(1025, 7, 0.35)
    for flags in (FRUSTUM, 0):
        m = mask.clone()
        want = checker(world, mm, _camera(), flags, None, m)
        assert_call(run(renderer, flags, _camera(), world, mm.cuda(), guarded(mask), None), want, m, f"flags {flags} without a pyramid")
        assert torch.equal(m, mask)


# ---- d. all eight flag sets --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_flag_sets(renderer, oracle_lib, flags):
    """The terrain straddles the camera: patches behind it, patches across the near plane and the patch the camera is inside.  LATE and
    OCCLUSION without FRUSTUM hand boxes behind the camera to project_aabb.  Without OCCLUSION and LATE the mask is bit-identical to its input;
    flags 0 emits the previously visible patches.  The other bits of CULL_TEST_ALL change nothing."""
    classes = dict(flag_classes())
    assert classes.pop("camera inside") and all(n >= 10 for n in classes.values()), classes
    world, mm, cam, pyr, mask, _ = flag_frame()
    m = mask.clone()
    want = checker(world, mm, cam, flags, pyr.struct(), m)
    mm_gpu = mm.cuda()
    got = run(renderer, flags, cam, world, mm_gpu, guarded(mask), pyr)
    assert_call(got, want, m, f"flags {flags}")
    if not flags & (OCCLUSION | LATE):
        assert torch.equal(mask_words(got[2]), mask)
    other = L.CULL_TEST_ALL & ~(FRUSTUM | OCCLUSION)
    assert other != 0
    again = run(renderer, flags | other, cam, world, mm_gpu, guarded(mask), pyr)
    assert_call(again, want, m, f"flags {flags} with the other bits of CULL_TEST_ALL")
    print(f"\nflags {flags}: emitted {want.numel()} of {world.total}")


# ---- e. edge values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_values(renderer, oracle_lib, case):
    """Rows of min == max, min > max, NaN, +-Inf, denormals and -0.0 in the min / max image, under a zero, negative and huge height_scale,
    a negative world_size, a world_min of 1e30, and a projection_view with a NaN entry or two rows scaled by 2^101."""
    world, cam = edge_case(case)
    mm, mask, pyr = edge_minmax(), _mask(world.total, 3, 0.35), small_pyramid(96, 40, 4)
    m, lists, masks = mask.clone(), [], []
    for flags in PASSES:
        lists.append(checker(world, mm, cam, flags, pyr.struct(), m))
        masks.append(m.clone())
    _two_passes(renderer, world, mm, cam, pyr, mask, lists, masks, case)


# ---- f. four frames with a moving camera -------------------------------------------------------------------------------------------------------
def test_mask_lives_on_the_gpu_across_frames(renderer, oracle_lib):
    """The mask is uploaded before frame 0 only; the checker carries its own.  Both are compared after every pass."""
    world, mm, pyr = World((64, 64)), _terrain(64, 64, 164), small_pyramid(128, 64, 2)
    mask = _mask(world.total, 7, 0.35)
    alloc, mm_gpu, counts = guarded(mask), mm.cuda(), []
    for f in range(4):
        cam = _camera(eye=(-60.0 + 45.0 * f, 40.0 - 6.0 * f, -40.0 * f))
        for flags in PASSES:
            want = checker(world, mm, cam, flags, pyr.struct(), mask)
            assert_call(run(renderer, flags, cam, world, mm_gpu, alloc, pyr), want, mask, f"frame {f} flags {flags}")
            counts.append(want.numel())
    assert len(set(counts)) > 4 and min(counts[1:]) > 0, counts


# ---- g. one context, borrowed scratch ----------------------------------------------------------------------------------------------------------
def _terrain_job(total_grid, seed):
    world = World(total_grid)
    mm, mask, lists, masks = two_pass_want(world, seed, 7, False)
    return world, mm.cuda(), mask, lists, masks


@pytest.mark.parametrize("async_triangles", [False, True], ids=["in-order", "async-triangles"])
def test_borrowed_scratch_on_one_context(oracle_lib, async_triangles):
    """The two-kernel form borrows the meshlet stage's ballots and block counts.  On a fresh context the first call is a 2049-patch terrain
    cull (it has to make the scratch); then a two-pass HiZ cull_geometry frame with a terrain cull between the early and the late call and one
    after the late call -- with async_triangles the triangle stage of the call before is still in flight -- then 65, 85 581 and 65 patches."""
    from oxylus_amd.renderer import CullGeometryContext, PreparedFrame, RendererInstance
    from util import oracle_frame

    r = RendererInstance(0)
    cam, pyr_t = _camera(), small_pyramid()
    world, mm_gpu, mask, lists, masks = _terrain_job((683, 3), 12)
    alloc = guarded(mask)
    assert_call(run(r, PASSES[0], cam, world, mm_gpu, alloc, pyr_t), lists[0], masks[0], "the context's first call")
    # the geometry frame
    scene, _, pyr, gmask = hiz_frames.shape_frame("96x40")
    want = oracle_frame(scene, use_hiz=True, hiz=pyr.hizd, mask=gmask.clone(), two_pass=True)
    gpu, att = scene.to("cuda"), pyr.attachment("cuda")
    base = PreparedFrame.create(gpu, with_triangles=True, expand=True)
    base.meshlet_instance_visibility_mask_buffer.copy_(gmask.cuda())
    ctx = CullGeometryContext(use_hiz=True, init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=gpu.cull_camera(), hiz_attachment=att, stages=L.STAGE_ALL,
                              async_triangles=async_triangles)
    r.seed_meshlet_instances(ctx, gpu.n_meshlet_instances)
    calls, pending = [], []
    for i, flags in enumerate(PASSES):
        frame = dataclasses.replace(base, reordered_indices_buffer=torch.zeros_like(base.reordered_indices_buffer))  # its own index list
        ctx.cull_flags = flags
        r.prepared_frame = frame
        r.cull_geometry(ctx)
        snap = L.CullGeometryContext()
        C.memmove(C.byref(snap), C.byref(ctx._c), C.sizeof(snap))
        calls.append((frame, snap))
        # the late terrain pass behind the early geometry call, a second early pass (of the late mask) behind the late one; nothing is read
        # back here, so with async_triangles the stage enqueued just above is still running
        pending.append(enqueue(r, PASSES[1 - i], cam, world, mm_gpu, alloc, pyr_t))
    r.join_triangles()
    torch.cuda.synchronize()
    got = {}
    for tag, (frame, snap) in zip(("early", "late"), calls):
        cnt = L.Counters()
        r._check(r._lib.oxc_read_counters(r._ctx, C.byref(snap), C.byref(cnt), r._stream(None)))
        got[f"{tag}_indices"] = frame.reordered_indices_buffer[:cnt.draw_index_count].cpu().numpy()
        got[f"{tag}_emitted"] = cnt.cull_triangles_cmd_x
    got["early"], got["late"] = cnt.early_visible_meshlet_instances, cnt.late_visible_meshlet_instances
    vis = base.visible_meshlet_instances_indices_buffer.cpu().numpy()
    got["early_visible"], got["late_visible"] = vis[:got["early"]], vis[got["early"]:got["early"] + got["late"]]
    got["mask"] = base.meshlet_instance_visibility_mask_buffer.cpu().numpy()
    for k in ("early", "late", "early_emitted", "late_emitted"):
        assert got[k] == want[k], k
    for k in ("early_visible", "late_visible", "early_indices", "late_indices", "mask"):
        assert np.array_equal(got[k], want[k]), k
    assert want["early"] > 0 and want["late"] > 0 and len(want["late_indices"]) > 0
    # the terrain calls made in between: the late pass, then an early pass over the late mask
    m = masks[1].clone()
    third = checker(world, mm_gpu.cpu(), cam, PASSES[0], pyr_t.struct(), m)
    (c1, v1), (c2, v2) = pending
    cmd1 = read_cmd(r, c1.draw_cmd_buffer.dptr)
    assert cmd1 == [4, lists[1].numel(), 0, 0]  # (read after the next terrain call: its slot is the call's own for 4096 further calls, include/oxcull.h)
    assert torch.equal(v1.cpu()[GUARD_WORDS:GUARD_WORDS + cmd1[1]], lists[1]) and bool((v1.cpu()[GUARD_WORDS + cmd1[1]:] == VISIBLE_FILL).all())
    assert_call(collect(r, c2, world, alloc, v2), third, m, "terrain cull behind the late geometry call")
    # 65, 85 581 (the scratch grows), 65 again; each command is read once more after the next call
    jobs = [_terrain_job((13, 5), 113), _terrain_job((333, 257), 433), _terrain_job((13, 5), 113)]
    kept = []
    for n, (w, mmg, msk, ls, ms) in enumerate(jobs):
        out = {}
        assert_call(run(r, PASSES[0], cam, w, mmg, guarded(msk), pyr_t, out=out), ls[0], ms[0], f"job {n}: {w.total} patches")
        kept.append((out["context"].draw_cmd_buffer.dptr, ls[0].numel()))
        if n:
            assert read_cmd(r, kept[n - 1][0]) == [4, kept[n - 1][1], 0, 0], f"the command of job {n - 1} after job {n}"
    assert jobs[1][0].total == 85581 and kept[0][0] != kept[1][0]
    r.close()


def test_large_cull_is_a_fresh_contexts_first_call(oracle_lib):
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    world, mm_gpu, mask, lists, masks = _terrain_job((333, 257), 433)
    alloc = guarded(mask)
    for flags, want, want_mask in zip(PASSES, lists, masks):
        assert_call(run(r, flags, _camera(), world, mm_gpu, alloc, small_pyramid()), want, want_mask, f"85 581 patches first, flags {flags}")
    r.close()


# ---- h. graph capture --------------------------------------------------------------------------------------------------------------------------
def test_two_passes_captured_into_a_graph(oracle_lib):
    """After an eager warm-up (which makes the scratch), early + late of a 2049-patch grid captured on a side stream and replayed twice with
    the mask restored: the bytes of the eager run.  The call launches and allocates nothing else under capture."""
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    cam, pyr = _camera(), small_pyramid()
    world, mm_gpu, mask, lists, masks = _terrain_job((2049, 1), 2149)
    alloc = guarded(mask)
    for flags, want, want_mask in zip(PASSES, lists, masks):
        assert_call(run(r, flags, cam, world, mm_gpu, alloc, pyr), want, want_mask, f"eager flags {flags}")
    att = pyr.attachment("cuda")
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    vis = [visible_allocation(world.total), visible_allocation(world.total)]
    ctxs = [terrain_context(flags, cam, world, mm_gpu, alloc, v, att)[0] for flags, v in zip(PASSES, vis)]
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        for c in ctxs:
            r._check(r._lib.oxc_cull_terrain(r._ctx, C.byref(c), C.c_void_p(s.cuda_stream)))
    for rep in range(2):
        alloc.copy_(guarded(mask))
        for v in vis:
            v.fill_(VISIBLE_FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for c, v, want, tag in zip(ctxs, vis, lists, ("early", "late")):
            got = collect(r, c, world, alloc, v)
            assert_call(got, want, masks[1], f"replay {rep} {tag}")  # (the mask is read after both passes)
    r.close()


def test_scratch_growth_is_refused_inside_a_capture(oracle_lib):
    """A fresh context has no ballot scratch: a captured 2049-patch cull fails the way test_scratch_growth_is_refused_inside_a_stream_capture
    does and enqueues nothing -- the replayed graph holds the marker alone."""
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    world = World((2049, 1))
    mask = random_words(world.total, 21)
    alloc, vis, mm_gpu, att = guarded(mask), visible_allocation(world.total), _terrain(2049, 1, 2149).cuda(), small_pyramid().attachment("cuda")
    c, _ = terrain_context(PASSES[0], _camera(), world, mm_gpu, alloc, vis, att)
    marker = torch.zeros(1, dtype=torch.int32, device="cuda")
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        marker.add_(1)
        status = r._lib.oxc_cull_terrain(r._ctx, C.byref(c), C.c_void_p(s.cuda_stream))
    assert status == L.OXC_INVALID_ARG
    with pytest.raises(L.OxcError) as ei:
        r._check(status)
    assert "captured" in str(ei.value)
    graph.replay()
    torch.cuda.synchronize()
    assert int(marker) == 1 and torch.equal(alloc.cpu(), guarded(mask, "cpu")) and bool((vis == VISIBLE_FILL).all())
    # the same call outside a capture makes the scratch and runs
    m = mask.clone()
    want = checker(world, mm_gpu.cpu(), _camera(), PASSES[0], small_pyramid().struct(), m)
    assert_call(run(r, PASSES[0], _camera(), world, mm_gpu, alloc, att, visible_alloc=vis), want, m, "after the refused capture")
    r.close()


# ---- i. arguments ------------------------------------------------------------------------------------------------------------------------------
def _set(**fields):
    def tweak(c):
        for name, value in fields.items():
            obj, leaf = c, name
            while "__" in leaf:
                head, leaf = leaf.split("__", 1)
                obj = getattr(obj, head)
            if isinstance(value, tuple):
                for i, v in enumerate(value):
                    getattr(obj, leaf)[i] = v
            else:
                setattr(obj, leaf, value)
    return tweak


def test_argument_checks_write_nothing(renderer):
    world = World((41, 25))
    mm_gpu, pyr = _terrain(41, 25, 8).cuda(), small_pyramid().attachment("cuda")
    size, words = C.sizeof(L.TerrainContext), (world.total + 31) // 32
    ALL = L.CULL_TEST_ALL
    # above 2^24 patches (4096 x 4096 itself is accepted and is not run here)
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(patch_count=(4096, 4097), patch_minmax_attachment__width=4096, patch_minmax_attachment__height=4097), "patch_count")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(patch_count=(0, 25), patch_minmax_attachment__width=0), "patch_count")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(patch_count=(41, 0), patch_minmax_attachment__height=0), "patch_count")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(patch_minmax_attachment__width=42), "patch_minmax_attachment")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(patch_minmax_attachment__height=24), "patch_minmax_attachment")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(visible_patches_buffer__bytes=4 * world.total - 4), "visible_patches_buffer")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(patch_visibility_mask_buffer__bytes=4 * words - 4), "patch_visibility_mask_buffer")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(struct_size=size + 4), "struct_size")
    _refused(renderer, ALL, world, mm_gpu, pyr, _set(struct_size=size - 4), "struct_size")
    for flags in (LATE, FRUSTUM | LATE, OCCLUSION):
        _refused(renderer, flags, world, mm_gpu, pyr, _set(hiz_attachment__levels=0), "hiz_attachment")
        _refused(renderer, flags, world, mm_gpu, pyr, _set(hiz_attachment__width=0), "hiz_attachment")
        _refused(renderer, flags, world, mm_gpu, None, None, "hiz_attachment")
