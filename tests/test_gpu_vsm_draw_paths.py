"""oxc_draw_physical_pages where random scenes do not reach: the stride loops of its kernels (OXC_TUNE_VSM_DRAW_GRID), bitmap rows that
straddle words and the drawable rectangle, each switch-over between its paths (in-wave, direct, tiled, clipped), queue overflows with
known counts, the draw command's corners, extreme page offsets, the depth rule's ends, non-finite vertices and the largest viewport.
Every test draws a hand-written frame (vsm_draw_frames) and compares the whole physical image bit for bit, the optional outputs, and -- on a
counting context whose queues did not overflow -- pairs, fragments, big pairs, tiles and clipped pairs with vsm_draw_model.draw, whose
predict the CPU tests hold to the path every frame was written for."""
import numpy as np
import pytest
import torch

import raster_model as RM
import vsm_draw_frames as VF
import vsm_draw_model as DM
from oxylus_amd import lib as L

pytestmark = pytest.mark.gpu

SENTINEL = -7
COUNTS = ("pairs", "fragments", "big_pairs", "tiles", "clipped_pairs")
OVERFLOWS = ("big_pairs_overflowed", "tiles_overflowed", "clipped_pairs_overflowed")


def _draw(r, vf, image=None):
    """Uploads frame `vf` (the index buffer sized exactly to its list) and draws it; returns the context."""
    from oxylus_amd.renderer import ImageAttachment, PreparedFrame, VsmDrawContext

    n, ps, phys, count = vf.shape
    frame = PreparedFrame.create(vf.frame.scene.to("cuda"), with_triangles=False)
    frame.reordered_indices_buffer = vf.indices().cuda()
    r.prepared_frame = frame
    ctx = VsmDrawContext(virtual_page_table=torch.from_numpy(vf.table.view(np.int32).copy()).cuda(), vsm_clipmaps_buffer=torch.from_numpy(vf.clipmaps.copy()).cuda(),
                         vsm_clipmap_dirty_flags_buffer=torch.tensor(vf.flags, dtype=torch.int32, device="cuda"),
                         physical_page_image=ImageAttachment.depth(torch.from_numpy(np.array(vf.image if image is None else image, dtype=np.float32)).cuda()),
                         page_size=ps, page_table_size=n, physical_page_table_size=phys, clipmap_count=count, wide_triangle_index=vf.form,
                         draw_cmd=torch.tensor(vf.cmd, dtype=torch.int64).to(torch.int32).cuda(),
                         draw_commands_buffer=torch.full((count, 5), SENTINEL, dtype=torch.int32, device="cuda"),
                         draw_count_buffer=torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda"),
                         draw_clipmaps_buffer=torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda"))
    r.draw_physical_pages(ctx)
    torch.cuda.synchronize()
    return ctx


def _same_image_and_outputs(ctx, vf, label):
    phys, count = vf.shape[2], vf.shape[3]
    want = vf.model()[0].view(np.uint32)
    got = ctx.physical_page_image.data.view(phys, phys).cpu().numpy().view(np.uint32)
    if not np.array_equal(got, want):
        ys, xs = np.nonzero(got != want)
        raise AssertionError(f"{label}: {len(ys)} texels differ, the first at (x {xs[0]}, y {ys[0]}): got 0x{got[ys[0], xs[0]]:08X}, want 0x{want[ys[0], xs[0]]:08X}")
    wc, wn, wl = DM.build_draw_commands(vf.flags, count, vf.cmd, np.full((count, 5), SENTINEL), np.full(count, SENTINEL))
    u = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    assert np.array_equal(u(ctx.draw_commands_buffer), wc) and int(u(ctx.draw_count_buffer)[0]) == wn and np.array_equal(u(ctx.draw_clipmaps_buffer), wl), label
    return got


def _run(r, vf, label):
    """Draw, compare image and outputs, and hold the counting context's stats to the model's (no queue may overflow)."""
    got = _same_image_and_outputs(_draw(r, vf), vf, label)
    st, want = r.debug_vsm_draw_stats(), vf.model()[1]
    print(label, st)
    assert all(st[k] == 0 for k in OVERFLOWS), (label, st)
    assert {k: st[k] for k in COUNTS} == want, (label, st, want)
    return got, st


@pytest.fixture(scope="module")
def counting():
    """A context of this module's own with the counting kernels on (queues of the default size: 4096 pairs, 8192 tiles for these frames)."""
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    r.debug_set_tuning(L.TUNE_VSM_DRAW_STATS, 1)
    yield r
    r.close()


@pytest.fixture
def capped(counting):
    """Every launch of the draw capped at one block: 4 waves (256 triangles per step of k_vsm_draw_tris, 4 big pairs or tiles per step),
    256 mesh instances per step of k_vsm_draw_rows, 64 queued pairs per step of k_vsm_draw_clipped, 256 bitmap words per step of the prologue."""
    counting.debug_set_tuning(L.TUNE_VSM_DRAW_GRID, 1)
    yield counting
    counting.debug_set_tuning(L.TUNE_VSM_DRAW_GRID, 0)


@pytest.fixture(scope="module")
def tiny_queues():
    """A fresh counting context whose big-pair and clip queues hold 64 entries and whose tile list holds 128."""
    from oxylus_amd.renderer import RendererInstance

    r = RendererInstance(0)
    r.debug_set_tuning(L.TUNE_VSM_DRAW_CAPACITY, VF.CAPACITY)
    r.debug_set_tuning(L.TUNE_VSM_DRAW_STATS, 1)
    yield r
    r.close()


# ---- 1. stride loops -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2], ids=["packed", "wide", "pairs"])
@pytest.mark.parametrize("n", VF.RF.STRIDE_COUNTS)
def test_triangle_and_rows_stride_loops(capped, n, form):
    """k_vsm_draw_tris over 1..5 steps of 256 triangles with full and partial last steps, k_vsm_draw_rows over 320 mesh instances."""
    _, st = _run(capped, VF.stride_frame(n, form), f"{n} triangles, form {form}")
    assert st["pairs"] == n and st["big_pairs"] == 0


def test_clip_queue_stride_loop(capped):
    _, st = _run(capped, VF.clip_stride_frame(), "clip stride")
    assert st["clipped_pairs"] == 136


def test_big_pair_and_tile_stride_loops(capped):
    _, st = _run(capped, VF.big_stride_frame(), "big stride")
    assert st["big_pairs"] >= 9 and st["tiles"] >= 9


def test_prologue_stride_loop_over_bitmap_words(capped):
    """n = 96: 288 words per clipmap for one block of 256 threads."""
    _run(capped, VF.wide_table_frame(), "288 bitmap words")


def test_the_cap_does_not_change_the_image(capped):
    for vf in (VF.stride_frame(1025), VF.big_stride_frame(), VF.wide_table_frame()):
        for cap in (2, 3, 0, 1):
            capped.debug_set_tuning(L.TUNE_VSM_DRAW_GRID, cap)
            _run(capped, vf, f"cap {cap}")


# ---- 2 .. 4, 7 .. 9: one frame, one claim each (what each frame is for: vsm_draw_frames; that it is that: tests/test_vsm_draw_model.py) ----------------
UNCAPPED = sorted(k for k in VF.all_frames() if not k.startswith(("stride-", "overflow-")))


@pytest.mark.parametrize("name", UNCAPPED)
def test_frame(counting, name):
    vf = VF.all_frames()[name]
    got, st = _run(counting, vf, name)
    if name.startswith("bitmap-"):
        assert st["pairs"] == (0 if name.endswith("outside-the-image") else 1)  # the four boxes beside the page hold no drawable page
    if name.startswith("shared-edge-"):
        s = int(name.rsplit("-", 1)[1])
        assert st["fragments"] == s * s
    if name == "threshold-spread-4095-4096":
        assert st["big_pairs"] == 4
    if name == "neg-zero":
        assert (got == VF.NEG_ZERO_BITS).any() and st["fragments"] > 100


# ---- 5. deterministic overflows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles", "big", "clip", "big-and-clip"])
def test_overflow(tiny_queues, name):
    """Queues of 64 pairs and 128 tiles.  tiles: 3 x 50 tiles, the third pair's ballot crosses 128 and its wave walks the rest in place;
    big: 82 big pairs, 12 of them out of the clipper; clip: 70 crossing pairs; big-and-clip: 70 of each.  The overflow passes draw what the
    queues could not hold: same image; the counters run on past the capacities, so they equal the model's totals.  (A pair the overflow pass
    meets again is drawn twice: fragments >=, and pairs too once the clip queue's pass has run.)"""
    vf = VF.overflow_frames()[name]
    _same_image_and_outputs(_draw(tiny_queues, vf), vf, name)
    st, want = tiny_queues.debug_vsm_draw_stats(), vf.model()[1]
    print(name, st)
    cap = VF.CAPACITY
    assert (st["big_pairs"], st["tiles"], st["clipped_pairs"]) == (want["big_pairs"], want["tiles"], want["clipped_pairs"]), (st, want)
    assert st["big_pairs_overflowed"] == max(want["big_pairs"] - cap, 0) and st["tiles_overflowed"] == max(want["tiles"] - 2 * cap, 0), (st, want)
    assert st["clipped_pairs_overflowed"] == max(want["clipped_pairs"] - cap, 0), (st, want)
    assert {"tiles": st["tiles_overflowed"], "big": st["big_pairs_overflowed"], "clip": st["clipped_pairs_overflowed"],
            "big-and-clip": min(st["big_pairs_overflowed"], st["clipped_pairs_overflowed"])}[name] > 0
    assert st["fragments"] >= want["fragments"] > 0
    assert st["pairs"] >= want["pairs"] if st["clipped_pairs_overflowed"] else st["pairs"] == want["pairs"], (st, want)


# ---- 6. the draw command -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 2], ids=["packed", "pairs"])
@pytest.mark.parametrize("cmd", [(15, 0, 0, 0, 0), (7, 1, 0, 0, 0), (8, 1, 0, 0, 0), (315, 1, 0, 0, 0), (9, 1, 0, 0, 0), (15, 1, 7, 0x7FFFFFFF, 0xFFFFFFFE), (15, 3, 3, 1, 1)],
                         ids=["no-instance", "count-7", "count-8", "count-past-the-buffer", "count-9-of-15", "words-2-4", "three-instances"])
def test_draw_command(counting, cmd, form):
    """instanceCount 0 draws nothing (the commands are still written); an index count draws count / 3 triangles, at most what the buffer
    holds (here: exactly the five of the list); words 2..4 are copied to the outputs and change nothing else."""
    vf = VF.command_frame(form, cmd)
    got, st = _run(counting, vf, f"cmd {cmd}")
    drawn = 0 if cmd[1] == 0 else min(cmd[0] // 3, 5)
    assert st["pairs"] == 2 * drawn
    assert np.array_equal(got, VF.command_frame(form, (3 * drawn, 1, 0, 0, 0)).model()[0].view(np.uint32))
    if drawn < 5:  # the list's tail would have drawn
        assert not np.array_equal(got, VF.command_frame(form).model()[0].view(np.uint32))


# ---- 10. the two draws agree where their rules coincide ----------------------------------------------------------------------------------------------
def _written_depth(vf):
    """(mask of written texels, their depth bits, vis per texel) of the frame's visbuffer image by the CPU checkers, and (mask, bits) of
    its shadow image by vsm_draw_model."""
    vd = vf.frame.oracle_image().numpy().view(np.uint64)
    shadow = vf.model()[0].view(np.uint32)
    return (vd != 0, (vd >> np.uint64(32)).astype(np.uint32), (vd & np.uint64(0xFFFFFFFF)).astype(np.uint32)), (shadow != F2_BITS, shadow)


F2_BITS = int(np.float32(2.0).view(np.uint32))


def _assert_agree(main, shadow, vf, label):
    (m_mask, m_bits, m_vis), (s_mask, s_bits) = main, shadow
    assert np.array_equal(m_mask, s_mask), f"{label}: {int((m_mask != s_mask).sum())} texels written by one draw only"
    assert np.array_equal(m_bits[m_mask], s_bits[s_mask]), f"{label}: {int((m_bits != s_bits)[m_mask].sum())} depths differ"
    for i, name in enumerate(VF.AGREEMENT_CLASSES):
        assert int((m_mask & (m_vis == vf.frame.vis(i, 0, 0))).sum()) > 0, (label, name)


def test_the_two_draws_agree_where_their_rules_coincide(counting, renderer, oracle_lib):
    """The same five triangles (vsm_draw_frames.agreement_frame: front-facing, disjoint, depth inside (0, 1), one per path) through
    oxc_draw_visbuffer at 128 x 128 and through oxc_draw_physical_pages with one identity-mapped clipmap of V = 128 under the same
    projection_view: the same texels are written and they hold the same depth bits -- first by the two CPU checkers, then on the device."""
    import test_gpu_raster_paths as RP

    vf = VF.agreement_frame()
    main, shadow = _written_depth(vf)
    # the unclipped four once more by the Python raster model, which does not clip
    rm, setups = vf.frame.model_image(vf.frame.draw[:4])
    four = vf.frame.oracle_image(draw=vf.frame.draw[:4]).numpy().view(np.uint64)
    assert np.array_equal(rm, four)
    assert [RM.predict(t)[0] for t in setups] == [RM.SMALL, RM.RECT32, RM.RECT32, RM.TILES32]
    _assert_agree(main, shadow, vf, "CPU checkers")
    # the device: each draw against its checker (bytes, path counts), then against the other
    got_s, st = _run(counting, vf, "agreement")
    assert (st["pairs"], st["big_pairs"], st["tiles"], st["clipped_pairs"]) == (6, 5, 9 + 20 + 48 + 30, 1), st  # the sliver leaves the clipper as two tiled pieces
    got_m = RP._draw(renderer, vf.frame)
    rs = renderer.debug_raster_stats()
    print("agreement", rs)
    RP._assert_same(got_m, vf.frame.oracle_image(), "agreement")
    assert (rs["clipped"], rs["big"], rs["tiles"], rs["overflowed_segments"]) == (1, 5, 2 + 4 + 4, 0), rs  # boxes of 50 x 70, 128 x 96 and 68 x 96 px in tiles of 64
    vd = got_m.numpy().view(np.uint64)
    _assert_agree((vd != 0, (vd >> np.uint64(32)).astype(np.uint32), (vd & np.uint64(0xFFFFFFFF)).astype(np.uint32)), (got_s != F2_BITS, got_s), vf, "device")
