"""oxc_resolve_shadowmap on the GPU: the resolved image byte-identical to tests/vsm_resolve_model.py, every pixel -- the compute-only frame
depth -> page table -> HPB -> shadow cull -> shadow draw -> resolve at the reference's shape and at a second one, a frame after
invalidation, an allocation-failure frame, an all-sky image, non-finite texels, graph capture of the whole shadow path, and invalid
arguments."""
import numpy as np
import pytest
import torch

import vsm_resolve_model as RM
from gpu_passes import Frame

pytestmark = pytest.mark.gpu


def _outcomes(st):
    oc = st["outcome"]
    return {name: int((oc == k).sum()) for name, k in (("sky", RM.SKY), ("hard", RM.HARD), ("no_blocker", RM.NO_BLOCKER), ("all_blockers", RM.ALL_BLOCKERS))}


def test_frame_at_the_reference_shape(renderer):
    """768 x 768, page 128, table 64, physical 8192, 10 clipmaps, a third of the pages evicted before the resolve.  The fixture is not
    degenerate: asserted through the checker, each of sky / hard-shadow / "no blocker" / "all blockers" / PCF ratio strictly inside (0, 1)
    holds at least 1000 pixels and each fallback clipmap serves at least 1000 taps.  Counts reached (first tried with the checker alone
    on the CPU models' frame, then on the device's): sky 267 518, hard 58 624, no blocker 32 398, all blockers 36 570, PCF inside (0, 1)
    2 289; 10 414 106 taps, 1 542 836 missed, 311 095 served by base - 1, 810 523 by base + 1.  The device's own counters agree with the checker's."""
    f = Frame(renderer, 768, 768, evict=True)
    L = f.L
    renderer.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 1)
    try:
        f.shadow_path()
        st = {}
        got = f.check(st)
        dev = renderer.debug_vsm_resolve_stats()
    finally:
        renderer.debug_set_tuning(L.TUNE_VSM_RESOLVE_STATS, 0)
    counts = _outcomes(st)
    counts["pcf_inside"] = int(((st["outcome"] == RM.PCF) & (got > 0.0) & (got < 1.0)).sum())
    print("outcomes", counts, "taps", st["taps"], "misses", st["misses"], "fallback_minus", st["fallback_minus"], "fallback_plus", st["fallback_plus"])
    print("device", dev)
    for name, v in counts.items():
        assert v >= 1000, (name, counts)
    assert st["fallback_minus"] >= 1000 and st["fallback_plus"] >= 1000, st
    assert dev == {"non_sky_pixels": got.size - counts["sky"], "taps": st["taps"], "misses": st["misses"], "fallback_minus": st["fallback_minus"],
                   "fallback_plus": st["fallback_plus"], "hard": counts["hard"], "no_blocker": counts["no_blocker"], "all_blockers": counts["all_blockers"]}
    f.r.resolve_shadowmap(f.rctx)  # the plain instantiation writes the same image
    f.check()


def test_second_shape_odd_resolution(renderer):
    shape = dict(page_size=64, page_table_size=32, physical_page_table_size=4096, clipmap_count=6)  # V = 2048 != physical
    f = Frame(renderer, 1277, 719, shape=shape, seed=62, first_clipmap_width=12.0)
    f.shadow_path()
    got = f.check()
    assert ((got > 0) & (got < 1)).any() and (got == 0).any() and (got == 1).any()


def test_frame_after_invalidation(renderer):
    f = Frame(renderer, 384, 384, seed=63)
    f.shadow_path()
    f.check()
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")  # the scene's one mesh instance
    v, s = f.vctx, f.gpu
    v.dirty_mesh_instance_indices = ids
    v.mesh_instances_buffer, v.meshes_buffer = s.mesh_instances, s.meshes
    v.transforms_world_buffer = v.transforms_previous_buffer = s.transforms
    f.shadow_path()
    assert int(v.counters_buffer.cpu()[1]) > 0  # pages were invalidated, requested again and redrawn
    f.check()


def test_allocation_failure_frame(renderer):
    """64 physical pages for a frame that asks for more: the pages that got none stay Visible and unbacked, and their taps miss."""
    shape = dict(page_size=128, page_table_size=64, physical_page_table_size=1024, clipmap_count=10)
    f = Frame(renderer, 384, 384, shape=shape, seed=64)
    f.shadow_path()
    st = {}
    f.check(st)
    assert int(f.vctx.counters_buffer.cpu()[4]) > 0 and st["misses"] > 0


def test_all_sky_and_non_finite_texels(renderer):
    f = Frame(renderer, 256, 256, seed=65)
    f.shadow_path()
    f.check()
    # non-finite depth and normal texels: the device and the checker agree on every NaN rule
    ys, xs = np.nonzero(f.depth.cpu().numpy() != 0)
    assert len(xs) > 100
    d, nrm = f.depth, f.normal
    for k, value in enumerate((float("nan"), float("inf"), -float("inf"), -0.0, 1e-30, 3e38)):
        d[int(ys[k * 7]), int(xs[k * 7])] = value
    for k, bits in enumerate((0x7E00, 0x7C00, -1024, 0x0001, -32768)):  # NaN, +inf, -inf, a denormal, -0.0 halves
        nrm[int(ys[50 + k * 5]), int(xs[50 + k * 5]), 2] = bits
        nrm[int(ys[80 + k * 5]), int(xs[80 + k * 5]), 3] = bits
    f.r.resolve_shadowmap(f.rctx)
    f.check()
    d.zero_()
    f.rctx.resolved_shadows_attachment.data.fill_(-5.0)
    f.r.resolve_shadowmap(f.rctx)
    assert (f.got() == 1.0).all()


def test_shadow_path_is_capturable_into_a_graph(renderer):
    f = Frame(renderer, 320, 320, seed=66)
    f.shadow_path()  # eager; every scratch grows here
    eager = f.check()
    assert ((eager > 0) & (eager < 1)).any()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.shadow_path(stream=s)
    f.vctx.virtual_page_table.zero_()
    f.vctx.physical_page_image.data.zero_()
    for _ in range(2):  # the first replay is the first frame again, the second a steady one: the same shadow term
        f.rctx.resolved_shadows_attachment.data.fill_(-5.0)
        torch.cuda.synchronize()
        g.replay()
        assert np.array_equal(f.got().view(np.uint32), eager.view(np.uint32))
    f.check()


def test_invalid_arguments(renderer):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import ImageAttachment

    f = Frame(renderer, 128, 128, seed=67)
    f.shadow_path()
    torch.cuda.synchronize()
    ctx = f.rctx

    def bad(**kw):
        saved = {k: getattr(ctx, k) for k in kw}
        for k, v in kw.items():
            setattr(ctx, k, v)
        with pytest.raises(L.OxcError) as e:
            renderer.resolve_shadowmap(ctx)
        assert e.value.status == L.OXC_INVALID_ARG
        for k, v in saved.items():
            setattr(ctx, k, v)

    bad(page_size=8)
    bad(page_size=24)
    bad(page_table_size=12)
    bad(page_table_size=264)
    bad(clipmap_count=0)
    bad(clipmap_count=17)
    bad(physical_page_table_size=64)                         # not a multiple of the page, and not the image's extent
    bad(page_size=16, physical_page_table_size=8192)         # 512 x 512 physical pages: beyond 16 address bits
    bad(physical_page_table_size=4096)                       # the image is 8192 square
    bad(resolved_shadows_attachment=ImageAttachment.depth(torch.zeros((128, 64), dtype=torch.float32, device="cuda")))
    bad(normal_attachment=torch.zeros((64, 128, 4), dtype=torch.int16, device="cuda"))
    bad(virtual_page_table=torch.zeros((9, 64, 64), dtype=torch.int32, device="cuda"))
    bad(vsm_clipmaps_buffer=torch.zeros(9 * 76, dtype=torch.uint8, device="cuda"))
    c = ctx.c()
    c.struct_size = 4
    assert renderer._lib.oxc_resolve_shadowmap(renderer._ctx, c, renderer._stream(None)) == L.OXC_INVALID_ARG
    renderer.resolve_shadowmap(ctx)  # and the context still resolves
    f.check()
