"""tests/terrain_brush_model.py, the checker of oxc_apply_terrain_brush, on the CPU: the library's export and the structs' layout against a
compiled probe of the header, answers worked by hand, the golden fixture, a binary64 transcription of the two Slang files, and the branch
counts of the rays and strokes the tests use."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import terrain_brush_frames as BF
import terrain_brush_model as TB
from oxylus_amd import lib as L

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rep = dataclasses.replace
RES, PC = (24, 20), (3, 5)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_export_and_struct_layout(tmp_path, liboxcull):
    """The symbol is exported with its prototype; sizes 96 / 16 / 16 and every offset of the three records and the context equal the header's."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    assert "oxc_apply_terrain_brush" in L.EXPORTS and hasattr(liboxcull, "oxc_apply_terrain_brush")
    mirrors = (L.TerrainBrushParams, L.TerrainBrushHit, L.TerrainRegion, L.TerrainBrushContext)
    assert [C.sizeof(m) for m in mirrors[:3]] == [96, 16, 16]
    prints = ""
    for m in mirrors:
        prints += f'  printf("%zu\\n", sizeof({m._c_name_}));\n' + "".join(f'  printf("%zu\\n", offsetof({m._c_name_}, {n}));\n' for n, _ in m._fields_)
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "oxcull.h"\nint main(void) {\n' + prints + "  return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    numbers = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    want = []
    for m in mirrors:
        want += [C.sizeof(m)] + [getattr(m, n).offset for n, _ in m._fields_]
    assert numbers == want


def test_renderer_context_marshals_every_field():
    from oxylus_amd.renderer import TerrainBrushContext, TerrainBrushParams

    p = TerrainBrushParams.engine((2048, 2048), (64, 64), (1.0, 500.0, 2.0), (0.0, -1.0, 0.0), mode=L.TERRAIN_BRUSH_FLATTEN, flatten_height_world=100.0, layer=2)
    c = TerrainBrushContext(p, None, None, None, None, None, stages=L.TERRAIN_BRUSH_TRACE).c()
    assert c.struct_size == C.sizeof(L.TerrainBrushContext) == 184 and c.stages == 1 and not c.hit.dptr
    q = c.params
    assert q.radius_texels == 64.0 and list(q.world_min) == [-512.0, -512.0] and q.inv_world_size[0] == F(1.0) / F(1024.0) and q.flatten_height == 0.25
    assert q.strength == min(max(F(3.0) * F(1.0 / 60.0), F(0.0)), F(1.0)) and q.mode == 2 and q.layer == 2 and list(q.patch_count) == [64, 64]
    same = BF.params((2048, 2048), (64, 64), (1.0, 500.0, 2.0), (0.0, -1.0, 0.0), radius_world=32.0, mode=TB.FLATTEN, flatten_height_world=100.0, layer=2)
    assert dataclasses.asdict(same) == {k: (tuple(v) if isinstance(v, tuple) else v) for k, v in dataclasses.asdict(p).items()}


# ---- answers worked by hand ----------------------------------------------------------------------------------------------------------------------
def _unit_world(res, **kw):
    """A world where a texel is one unit: world_min 0, world_size = resolution, heights in world units of 1 / 65535 * 65535."""
    return TB.Params(resolution=res, world_min=(0.0, 0.0), world_size=(float(res[0]), float(res[1])), inv_world_size=(float(F(1.0) / F(res[0])), float(F(1.0) / F(res[1]))),
                     patch_count=(2, 2), base_height=0.0, height_scale=64.0, **kw)


def test_flat_map_under_a_vertical_and_a_45_degree_ray():
    """A 16 x 16 map of height 0.25 * 64 = 16 (q = 0x4000 is not a quarter of 65535, so take what the load gives).  Vertical from y = 100 at
    (1.5, 2.5): the span is (0, 1e9), the crossing is step 1, and 24 bisections leave hi within 1953125 / 2^24 of 100 - h above the ground.
    At 45 degrees from (0.5, 100, 2.5) the hit lies at x = 0.5 + (100 - h), clipped by nothing.  radius 3: both origins clamp at 0."""
    hm = np.full((16, 16), 0x4000, np.uint16)
    h = float(TB.load_unorm16(np.uint16(0x4000)) * F(64.0))
    B = _unit_world((16, 16), ray_origin=(1.5, 100.0, 2.5), ray_direction=(0.0, -2.0, 0.0), radius_texels=3.0)
    info = {}
    hit, region = TB.trace(B, hm, info=info)
    wp = hit[:3].view(np.float32)
    assert info["step"] == 1 and info["span"] == (0.0, F(1e9)) and hit[3] == 1
    assert wp[0] == 1.5 and wp[2] == 2.5 and 0 <= h - wp[1] <= 1953125.0 / 2 ** 24 + 1e-5
    assert region.tolist() == [0, 0, 0, 0]  # floor(1.5 - 4) < 0
    B45 = rep(B, ray_origin=(0.5, 20.0, 2.5), ray_direction=(1.0, -1.0, 0.0))
    hit, region = TB.trace(B45, hm, info=info)
    wp = hit[:3].view(np.float32)
    # span: x from 0.5 to 16 -> t in [0, 15.5 * sqrt 2]; steps of 15.5 sqrt 2 / 512 ~ 0.0428, bisected 24 times
    assert hit[3] == 1 and abs(wp[0] - (0.5 + 20.0 - h)) < 1e-4 and abs(wp[1] - h) < 1e-4 and wp[2] == 2.5
    assert region.tolist() == [0, 0, 0, 0]  # centre (4.5, 2.5) - 4 = (0.5, -1.5)
    far = rep(B45, ray_origin=(8.5, 20.0, 9.5))
    hit, region = TB.trace(far, hm)
    assert region.tolist() == [8, 5, 1, 0]  # centre (12.5, 9.5) - 4 = (8.5, 5.5); * 2 / 16 = (1.06, 0.69)


def test_clip_to_footprint_by_hand():
    B = _unit_world((16, 16))
    assert TB.clip_to_footprint(B, (-4.0, 0, 3.0), (1.0, 0.0, 0.0)) == (4.0, 20.0)            # x enters at 4, leaves at 20; z parallel and inside
    assert TB.clip_to_footprint(B, (-4.0, 0, 3.0), (-1.0, 0.0, 0.0)) == (0.0, -4.0)           # pointing away: near 0 > far -4
    assert TB.clip_to_footprint(B, (3.0, 0, 17.0), (1.0, 0.0, 0.0)) == (1.0, 0.0)             # parallel to z and outside it
    assert TB.clip_to_footprint(B, (3.0, 0, 5.0), (0.0, -1.0, 0.0)) == (0.0, F(1e9))          # parallel to both and inside
    assert TB.clip_to_footprint(B, (-2.0, 0, -6.0), (0.5, 0.0, 0.5)) == (12.0, 36.0)          # x: [4, 36], z: [12, 44]
    counts = {}
    TB.trace(rep(B, ray_origin=(3.0, 5.0, 17.0), ray_direction=(1.0, 0.0, 0.0)), np.zeros((16, 16), np.uint16), counts)
    TB.trace(rep(B, ray_origin=(-4.0, 5.0, 3.0), ray_direction=(-1.0, 0.0, 0.0)), np.zeros((16, 16), np.uint16), counts)
    assert counts == {"miss_parallel": 1, "miss_clip": 1}


def test_falloff_by_hand():
    """distance 0: t = 1, smoothed = 1 * (1 * (6 - 15) + 10) = 1, pow 1;  radius / 2: t = 0.5, smoothed = 0.125 * (0.5 * -12 + 10) = 0.5, and
    with falloff 2 it is 0.25;  radius: t = 0, the pow rule's zero base gives 0.  A radius of 0 gives 0 everywhere."""
    B = TB.Params(radius_texels=8.0, falloff=1.0)
    assert TB.falloff_of(B, [0.0, 4.0, 8.0, 9.0]).tolist() == [1.0, 0.5, 0.0, 0.0]
    assert TB.falloff_of(rep(B, falloff=2.0), [0.0, 4.0, 8.0]).tolist() == [1.0, 0.25, 0.0]
    assert TB.falloff_of(rep(B, falloff=-5.0), [4.0])[0] == TB.falloff_of(rep(B, falloff=1e-3), [4.0])[0] > 0.999
    assert TB.falloff_of(rep(B, radius_texels=0.0), [0.0]).tolist() == [0.0]


def test_one_texel_of_each_mode():
    """A hit at the centre of texel (2, 2) of a 5 x 5 map with radius 0.5: footprint 3 x 3 threads' worth, and only texel (2, 2) has distance
    0 < radius: falloff 1, amount = strength = 0.5."""
    hm = ((np.arange(25, dtype=np.uint32) ** 2) * 100).astype(np.uint16).reshape(5, 5)  # not linear: its 5 x 5 mean is not the centre
    he = np.full((5, 5), 0.25, np.float32)
    se = np.full((5, 5), 0x80402000, np.uint32)
    hit = np.concatenate([np.array([2.5, 0.0, 2.5], np.float32).view(np.uint32), [1]]).astype(np.uint32)
    B = _unit_world((5, 5), radius_texels=0.5, strength=0.5, flatten_height=0.75)
    l = TB.load_unorm16
    only = lambda out: (np.argwhere(out != he).tolist(), out[2, 2])  # noqa: E731
    assert only(TB.apply(rep(B, mode=TB.RAISE), hit, hm, he, se)[0]) == ([[2, 2]], F(0.75))
    total = F(0.0)
    for v in hm.reshape(-1):
        total = total + l(v)
    assert only(TB.apply(rep(B, mode=TB.SMOOTH), hit, hm, he, se)[0]) == ([[2, 2]], F(0.25) + (total / F(25.0) - l(hm[2, 2])) * F(0.5))
    assert only(TB.apply(rep(B, mode=TB.FLATTEN), hit, hm, he, se)[0]) == ([[2, 2]], F(0.25) + (F(0.75) - l(hm[2, 2])) * F(0.5))
    from terrain_maps_model import noised
    assert only(TB.apply(rep(B, mode=TB.NOISE), hit, hm, he, se)[0]) == ([[2, 2]], F(0.25) + noised(F(2.0) * F(0.05), F(2.0) * F(0.05), 0)[0] * F(0.5))
    assert TB.apply(rep(B, mode=TB.RAISE, strength=4.0), hit, hm, he, se)[0][2, 2] == 1.0 and TB.apply(rep(B, mode=TB.RAISE, strength=-4.0), hit, hm, he, se)[0][2, 2] == -1.0
    # PaintLayer 2 at t = 0.5 over (0x00, 0x20, 0x40, 0x80): (0, (32 + 223 * .5) -> 143.5 -> 144 (the lerp rounds up), 32, (128 + 127 * .5) -> 192)
    painted = TB.apply(rep(B, mode=TB.PAINT_LAYER, layer=2), hit, hm, he, se)[1]
    assert np.argwhere(painted != se).tolist() == [[2, 2]] and painted[2, 2] in (0xC0209000, 0xC0208F00) and (painted[2, 2] >> 16) & 0xFF == 0x20
    assert TB.apply(rep(B, mode=TB.PAINT_LAYER, layer=7, strength=3.0), hit, hm, he, se)[1][2, 2] == 0xFF000000
    miss = hit.copy()
    miss[3] = 0
    assert (TB.apply(rep(B, mode=TB.RAISE), miss, hm, he, se)[0] == he).all()


# ---- the golden fixture ----------------------------------------------------------------------------------------------------------------------------
def test_golden_fixture_pins_the_checker():
    """tests/golden/terrain_brush_24x20.npz (python tests/terrain_brush_frames.py): the inputs and the expected records and edit images."""
    from gpu_passes import same

    stored = np.load(BF.GOLDEN)
    B, images = BF.golden_case()
    for name in BF.IMAGES:
        same(images[name], stored["in_" + name], name)
    out = BF.want(B, images)
    for name in ("hit", "region", "height_edit", "splat_edit"):
        same(out[name], stored["out_" + name], name)
    same(BF.want(rep(B, mode=TB.PAINT_LAYER, layer=2), images)["splat_edit"], stored["out_splat_edit_paint"], "paint")
    assert out["hit"][3] == 1 and (out["height_edit"] != images["height_edit"]).any()


# ---- the checker against a binary64 transcription -------------------------------------------------------------------------------------------------
def _rays():
    """Every ray of the set: (name, heightmap kind, params).  Chosen so that the binary64 march crosses at the checker's step: the seam rays
    cross midway between two steps, the others meet the ground at an angle."""
    rays = [(f"step {k}", "flat", BF.params(RES, PC, *BF.ray_crossing_at_step(k), radius_texels=2.5, strength=0.5)) for k in (1, 255, 256, 257, 511, 512)]
    rays += [("ridge", "ridge", BF.params(RES, PC, (-500.0, 300.0, 0.0), (1.0, -0.27, 0.0), radius_texels=2.5, strength=0.5)),
             ("ramp", "ramp", BF.params(RES, PC, (-300.0, 420.0, -150.0), (0.6, -0.7, 0.35), radius_texels=2.5, strength=0.75)),
             ("pit", "pit", BF.params(RES, PC, (-20.0, 450.0, 30.0), (0.05, -1.0, -0.07), radius_texels=6.0, strength=0.4)),
             ("under", "ramp", BF.params(RES, PC, (0.0, -50.0, 0.0), (0.3, -1.0, 0.1), radius_texels=2.5)),
             ("outside", "ramp", BF.params(RES, PC, (-900.0, 500.0, -900.0), (-1.0, -1.0, 0.5), radius_texels=2.5)),
             ("parallel", "ramp", BF.params(RES, PC, (0.0, 500.0, 900.0), (1.0, -1.0, 0.0), radius_texels=2.5))]
    return rays


def _trace64(B, hm):
    """terrain_brush_trace.slang statement by statement in binary64 -> (step or 0, world_position)."""
    d = np.asarray(B.ray_direction, np.float64)
    d = d / np.sqrt((d * d).sum())
    o = np.asarray(B.ray_origin, np.float64)
    W, H = B.resolution
    t64 = hm.astype(np.float64) / 65535.0

    def sample(x, z):
        u, v = (x - B.world_min[0]) * B.inv_world_size[0], (z - B.world_min[1]) * B.inv_world_size[1]
        gx, gy = u * W - 0.5, v * H - 0.5
        ix, iy = int(np.floor(gx)), int(np.floor(gy))
        fx, fy = gx - ix, gy - iy
        c = lambda i, n: min(max(i, 0), n - 1)  # noqa: E731
        top = t64[c(iy, H), c(ix, W)] * (1 - fx) + t64[c(iy, H), c(ix + 1, W)] * fx
        bottom = t64[c(iy + 1, H), c(ix, W)] * (1 - fx) + t64[c(iy + 1, H), c(ix + 1, W)] * fx
        return B.base_height + (top * (1 - fy) + bottom * fy) * B.height_scale

    near, far = 0.0, 1e9
    for oo, dd, lo, size in ((o[0], d[0], B.world_min[0], B.world_size[0]), (o[2], d[2], B.world_min[1], B.world_size[1])):
        hi = lo + size
        if abs(dd) < 1e-6:
            if oo < lo or oo > hi:
                return 0, None
            continue
        t0, t1 = (lo - oo) / dd, (hi - oo) / dd
        near, far = max(near, min(t0, t1)), min(far, max(t0, t1))
    if not near <= far:
        return 0, None
    step = (far - near) / 512.0
    gap = lambda t: (o[1] + d[1] * t) - sample(o[0] + d[0] * t, o[2] + d[2] * t)  # noqa: E731
    previous_t, previous_gap = near, gap(near)
    for i in range(1, 513):
        t = near + step * i
        g = gap(t)
        if g <= 0 and previous_gap > 0:
            lo, hi = previous_t, t
            for _ in range(24):
                mid = (lo + hi) * 0.5
                lo, hi = (mid, hi) if gap(mid) > 0 else (lo, mid)
            return i, o + d * hi
        previous_t, previous_gap = t, g
    return 0, None


def _apply64(B, wp, hm, he, se):
    """terrain_brush_apply.slang in binary64 for every texel of the map -> (height_edit, splat channels [H, W, 4] before the unorm store)."""
    W, H = B.resolution
    cx, cy = (wp[0] - B.world_min[0]) * B.inv_world_size[0] * W, (wp[2] - B.world_min[1]) * B.inv_world_size[1] * H
    y, x = np.mgrid[0:H, 0:W]
    radius = int(np.ceil(B.radius_texels))
    inside = (np.abs(x - (np.floor(cx) - radius) - radius) <= radius) & (np.abs(y - (np.floor(cy) - radius) - radius) <= radius)
    t = np.clip(1 - np.hypot(x + 0.5 - cx, y + 0.5 - cy) / B.radius_texels, 0, 1)
    falloff = np.where(inside, (t * t * t * (t * (t * 6 - 15) + 10)) ** max(B.falloff, 1e-3), 0.0)
    amount = falloff * B.strength
    h = hm.astype(np.float64) / 65535.0
    pad = np.pad(h, 2, mode="edge")
    smooth = sum(pad[2 + oy:2 + oy + H, 2 + ox:2 + ox + W] for oy in range(-2, 3) for ox in range(-2, 3)) / 25.0
    from terrain_maps_model import noised
    delta = {TB.RAISE: amount, TB.SMOOTH: (smooth - h) * amount, TB.FLATTEN: (B.flatten_height - h) * amount,
             TB.NOISE: noised((x * F(0.05)).astype(np.float32), (y * F(0.05)).astype(np.float32), 0)[0].astype(np.float64) * amount}.get(B.mode, amount)
    out_h = np.where(falloff > 0, np.clip(he.astype(np.float64) + delta, -1, 1), he)
    p = np.stack([((se >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.float64) / 255.0 for c in range(4)], -1)
    target = np.array([float(B.layer == 1), float(B.layer == 2), float(B.layer == 3), 1.0])
    out_s = np.where((falloff > 0)[..., None], p + (target - p) * np.clip(amount, 0, 1)[..., None], p)
    return out_h, out_s


# the largest differences measured over the ray set; asserted at four times them
MEASURED = {"position": 1.76e-5, "height_edit": 2.2e-7, "splat": 0.0}  # splat: beyond the half step of the unorm8 store


def test_checker_against_a_binary64_transcription():
    """Every ray of the set: the transcription's crossing step equals the checker's (no ray is left out); the hit positions, and for every
    mode the edit values of the hits, differ by no more than four times what was measured.  The strokes use the checker's hit as the centre,
    so the comparison is of the apply rules alone; the splat channels are compared before the unorm8 store, the checker's after it (half a
    step of 1 / 255 is allowed on top)."""
    worst = {"position": 0.0, "height_edit": 0.0, "splat": 0.0}
    for name, kind, B in _rays():
        images = BF.initial(RES, kind)
        info = {}
        out = BF.want(B, images, TB.TRACE, info=info)
        step64, wp64 = _trace64(B, images["heightmap"])
        assert step64 == info["step"], f"{name}: binary64 crosses at step {step64}, the checker at {info['step']}"
        if not step64:
            continue
        wp = out["hit"][:3].view(np.float32).astype(np.float64)
        worst["position"] = max(worst["position"], np.abs(wp - wp64).max())
        for mode in range(5):
            M = rep(B, mode=mode, layer=2, flatten_height=0.6)
            he, se = TB.apply(M, out["hit"], images["heightmap"], images["height_edit"], images["splat_edit"])
            he64, se64 = _apply64(M, wp, images["heightmap"], images["height_edit"], images["splat_edit"])
            if mode == TB.PAINT_LAYER:
                got = np.stack([((se >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.float64) / 255.0 for c in range(4)], -1)
                worst["splat"] = max(worst["splat"], max(0.0, np.abs(got - se64).max() - 0.5 / 255.0))
            else:
                worst["height_edit"] = max(worst["height_edit"], np.abs(he - he64).max())
    print("largest differences:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k in worst:
        assert worst[k] <= 4 * MEASURED[k], (k, worst[k])


# ---- non-degeneracy --------------------------------------------------------------------------------------------------------------------------------
def test_every_branch_is_taken_over_the_test_set():
    counts = {}
    for name, kind, B in _rays():
        images = BF.initial(RES, kind)
        for mode in range(5):
            BF.want(rep(B, mode=mode, layer=1), images, counts=counts)
    for name in TB.COUNTS:
        assert counts.get(name, 0) > 0, name
    assert set(counts["hit_step"]) >= {1, 255, 256, 257, 511, 512}
