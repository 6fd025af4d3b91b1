"""Known answers of the VSM page-update checker (tests/vsm_pages_model.py), hand-derived from Shaders/rmvsm.slang and
passes/rmvsm_*.slang, and the boundary of oxc_update_virtual_shadowmap (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np

import vsm_pages_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_pixel_lands_on_its_page():
    hc = VM.hand_case()
    assert VM.texel_length(8, hc["fcw"], hc["vext"]) == np.float32(14.0) / np.float32(1120.0)
    m = VM.mark_visible(hc["depth"], hc["inv_pv"], hc["resolution"], hc["clipmaps"], 8, 3, hc["fcw"], hc["bias"], hc["vext"])
    assert [tuple(int(i) for i in p) for p in np.argwhere(m)] == [hc["page"]]
    out = VM.update(np.zeros((3, 8, 8), np.uint32), hc["depth"], hc["inv_pv"], hc["resolution"], hc["clipmaps"], page_size=16,
                    physical_page_table_size=64, count=3, first_clipmap_width=hc["fcw"], bias=hc["bias"], virtual_extent=hc["vext"])
    assert out["table"][2, 7, 0] == 7 and out["dirty"].tolist() == [[0, 0]] and out["dirty_flags"].tolist() == [0, 0, 1]
    assert out["counters"].tolist() == [1, 1, 16, 1, 0, 0, 0, 0] and out["clear_cmd"].tolist() == [1, 1, 1]


def test_clipmap_index_at_the_thresholds_bias_2():
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    # k - 2 < 0 for k = 0, 1: index >= 2 for every r; T_2 = 1, T_3 = 2, ... T_8 = 64
    r = np.array([0.0, 0.1, down, one, up, 2.0, np.nextafter(np.float32(2), np.float32(3)), 64.0, 65.0, 1e30, np.nan], dtype=np.float32)
    assert VM.clipmap_index(r, 2.0, 10).tolist() == [2, 2, 2, 2, 3, 3, 4, 8, 9, 9, 2]
    assert VM.clipmap_index(r, 2.0, 1).tolist() == [0] * 11  # one clipmap: always 0


def test_clipmap_index_at_the_thresholds_bias_minus_1_5():
    t0 = np.float32(2.0 ** 1.5)  # binary32 nearest to T_0 = 2^1.5 (irrational: never equal)
    below = t0 if float(t0) < 2.0 ** 1.5 else np.nextafter(t0, np.float32(0))
    above = np.nextafter(below, np.float32(10))
    r = np.array([0.0, 0.5, 1.0, below, above, 2.0 ** 2.5 * 1.0001, np.inf, np.nan], dtype=np.float32)
    # ceil(-1.5 + max(log2 r, 0)): negative -> 0; just past 2^1.5 -> 1; past 2^2.5 -> 2; inf -> count - 1; NaN -> log2 = 0 -> 0
    assert VM.clipmap_index(r, -1.5, 10).tolist() == [0, 0, 0, 0, 1, 2, 9, 0]


def test_floor_mod_wraps_negative_offsets():
    assert VM.wrap([1, 0, 7, 0, 5], [-2, -17, 9, 0, -64], 8).tolist() == [7, 7, 0, 0, 5]
    assert VM.wrap(3, -1000003, 64) == (3 - 1000003) % 64


def test_depth_zero_marks_nothing():
    hc = VM.hand_case()
    z = np.zeros_like(hc["depth"])
    assert not VM.mark_visible(z, hc["inv_pv"], hc["resolution"], hc["clipmaps"], 8, 3, hc["fcw"], hc["bias"], hc["vext"]).any()
    # outside the clip space of the clipmap (uv' > 1) and uv' == 1 (virt == n) mark nothing either
    rec = np.frombuffer(hc["clipmaps"], dtype=np.float32).reshape(3, 19).copy()
    rec[2, 12] = 1.0  # x translation: uv' = uv + 0.5
    d = np.zeros((64, 64), np.float32)
    d[10, 40] = 0.5
    assert not VM.mark_visible(d, hc["inv_pv"], hc["resolution"], rec.view(np.uint8).reshape(-1), 8, 3, hc["fcw"], hc["bias"], hc["vext"]).any()


def _table(entries, layers=1, n=8):
    t = np.zeros((layers, n, n), np.uint32)
    for (l, y, x), v in entries.items():
        t[l, y, x] = v
    return t


def test_failed_allocation_leaves_the_entry_unchanged():
    # P = 1: one physical page; three requests.  The first gets page 0, the other two fail: not stored (no AllocationFailed bit)
    t = _table({(0, 0, 1): 0, (0, 2, 0): 0x30000 | VM.INVALIDATED, (0, 5, 5): 0})
    m = np.zeros_like(t, dtype=bool)
    m[0, 0, 1] = m[0, 2, 0] = m[0, 5, 5] = True
    out = VM.resolve(t, m, 16, 16)
    assert t[0, 0, 1] == VM.VISIBLE | VM.DIRTY | VM.BACKED
    assert t[0, 2, 0] == 0x30000 | VM.INVALIDATED | VM.VISIBLE and t[0, 5, 5] == VM.VISIBLE
    assert out["counters"].tolist() == [3, 1, 1, 3, 2, 0, 0, 0]


def test_free_invisible_clears_only_the_backed_bit():
    t = _table({(0, 1, 1): (9 << 16) | VM.BACKED | VM.INVALIDATED})
    VM.resolve(t, np.zeros_like(t, dtype=bool), 16, 64)
    assert t[0, 1, 1] == (9 << 16) | VM.INVALIDATED


def test_invalidation_resets_the_entry_to_8(oracle_lib):
    from oxylus_amd.synth import pack_clipmaps

    # identity clipmap, a unit box at the origin: project_aabb gives uv [0.25, 0.75]^2 -> pages 2..5 of n = 8
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    clip = pack_clipmaps(eye[None], np.array([[1, 0]], np.int32), -10.0).numpy()
    t = _table({(0, 3, 4): (7 << 16) | VM.BACKED, (0, 3, 7): (5 << 16) | VM.BACKED, (0, 0, 0): (6 << 16) | VM.BACKED, (0, 4, 5): VM.VISIBLE})
    mi = np.array([[0, 0, 0, 0, 0]], np.int32)
    mesh = np.zeros(16, np.float32)
    mesh[13:16] = 1.0  # aabb_extent; center 0 -> corners at -0.5 (the `center - extent * 0.5` convention)
    tw = eye.reshape(1, 16)
    assert VM.invalidation_rect(eye, -10.0, mesh[10:13], mesh[13:16], 8) == (2, 2, 5, 5)
    VM.invalidate(t, clip, 1, [0], mi, mesh.view(np.int64), tw, tw)
    # virtual x 2..5 wrap to 3..6 (offset +1): (3, 4) is inside, (3, 7) and (0, 0) are not; an unbacked page is left alone
    assert t[0, 3, 4] == VM.INVALIDATED and t[0, 3, 7] == (5 << 16) | VM.BACKED and t[0, 0, 0] == (6 << 16) | VM.BACKED and t[0, 4, 5] == VM.VISIBLE


def test_request_free_and_dirty_list_orders():
    # two layers of n = 8, P = 2 (4 physical pages); physical page 1 is held by a visible backed page, so the free list is [0, 2, 3]
    t = _table({(1, 0, 0): 0, (0, 7, 7): 0, (0, 0, 5): 0, (1, 6, 2): (1 << 16) | VM.BACKED, (0, 3, 3): 0}, layers=2)
    m = np.zeros_like(t, dtype=bool)
    for p in ((1, 0, 0), (0, 7, 7), (0, 0, 5), (1, 6, 2), (0, 3, 3)):
        m[p] = True
    out = VM.resolve(t, m, 16, 32)
    assert out["free_list"].tolist() == [0, 2, 3]
    # requests in ascending (layer, y, x): (0,0,5), (0,3,3), (0,7,7), (1,0,0) -> pages 0, 2, 3, fail
    assert [tuple(int(v) for v in np.unravel_index(i, t.shape)) for i in out["requests"]] == [(0, 0, 5), (0, 3, 3), (0, 7, 7), (1, 0, 0)]
    assert t[0, 0, 5] >> 16 == 0 and t[0, 3, 3] >> 16 == 2 and t[0, 7, 7] >> 16 == 3 and t[1, 0, 0] == VM.VISIBLE
    assert out["dirty"].tolist() == [[0, 0], [0, 1], [1, 1]] and out["dirty_flags"].tolist() == [1, 0]
    assert out["counters"].tolist() == [4, 3, 3, 4, 1, 0, 0, 0]


def test_context_struct_matches_the_header(tmp_path):
    from oxylus_amd import lib as L

    src = tmp_path / "vsm.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oxcull.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(oxc_vsm_update_context), '
                   'offsetof(oxc_vsm_update_context, inv_projection_view), offsetof(oxc_vsm_update_context, virtual_page_table), '
                   'offsetof(oxc_vsm_update_context, hpb_attachment), offsetof(oxc_vsm_update_context, physical_page_image)); return 0; }\n')
    exe = str(tmp_path / "vsm")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    V = L.VsmUpdateContext
    assert got == [C.sizeof(V), V.inv_projection_view.offset, V.virtual_page_table.offset, V.hpb_attachment.offset, V.physical_page_image.offset]


def test_entry_point_is_exported_and_bound():
    from oxylus_amd import lib as L

    L.build()
    lib = L.load()
    assert "oxc_update_virtual_shadowmap" in L.EXPORTS and hasattr(lib, "oxc_update_virtual_shadowmap")
    assert L.KERNEL_NAMES[15] == "vsm_update"
