"""The case table of tests/test_gpu_pixel_pass_edges.py -- the extents from 1 x 1 to 129 x 65 at which the tiles, clamps and level counts of
oxc_generate_ambient_occlusion, oxc_contact_shadows and oxc_resolve_shadowmap degenerate -- with its seeded inputs, and the proof, made with
the three checkers alone (no GPU needed), that no case of it passes vacuously: every mip level is sampled at every extent, rays are cut at
the border and clamped at all four sides, every outcome class occurs, and no generated input holds a poison pattern of the guard bands."""
import functools

import numpy as np
import pytest

import ambient_occlusion_model as AM
import contact_shadows_model as CM
import vsm_resolve_model as RM
from test_ambient_occlusion_model import PROJ, hilbert
from test_contact_shadows_model import I16, class_counts

F = np.float32

# below one 8 x 8 wave tile; exactly one and one-plus-one wave tile, 16 x 16 block and 32 x 32 prefilter block in each axis separately; strips
# one texel wide or high that span several tiles; every combination of upper prefilter levels collapsed to max(1, dim >> k)
EXTENTS = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (8, 8), (9, 7), (15, 17), (16, 16), (17, 9), (31, 33), (32, 32), (33, 31), (47, 1), (1, 47),
           (64, 3), (129, 65)]
EXTENT_IDS = [f"{w}x{h}" for w, h in EXTENTS]

# ---- the poison of the guard bands ----------------------------------------------------------------------------------------------------------
NAN32 = 0x7FC00000   # around float inputs: a read changes the result
NAN16 = 0x7E00       # around the normals
HILBERT_POISON = 0xFFFF  # around the Hilbert table (its entries are 0..4095)
OUT32 = 0x7FC00BAD   # around 32-bit outputs and between the prefiltered levels: a NaN as a float, no edge word the checker produces nearby
OUT16 = 0x7EAD       # around the half outputs: a NaN half


def holds(a, bits, dtype) -> bool:
    return bool((np.ascontiguousarray(a).view(dtype) == dtype(bits)).any())


# ---- ambient occlusion ----------------------------------------------------------------------------------------------------------------------
AO_FAR = 100.0
AO_SKY_DEPTH = F(0.005)  # linear 200 under PROJ (linear = 1 / depth): beyond far * 0.999
AO_WIDE = dict(slice_count=3, samples_per_slice_side=8, effect_radius=400.0)  # the sample distances reach all five levels at every extent
AO_RESOLUTIONS = [((33, 31), (40.0, 25.0)), ((33, 31), (33.5, 30.25))]  # resolution is a float argument of its own


def ao_seed(W, H):
    return 1000 * W + H


@functools.lru_cache(maxsize=None)
def ao_inputs(W, H):
    """(depth float32 [H, W], normal uint16 [H, W, 4]): a seeded device depth in (0.05, 0.95) with about one texel in twelve sky (none in an
    image of fewer than four texels; one non-sky texel always stays), and view-space normals of mixed directions that face the camera."""
    rng = np.random.default_rng(ao_seed(W, H))
    depth = rng.uniform(0.05, 0.95, (H, W)).astype(np.float32)
    if W * H >= 4:
        sky = rng.permutation(W * H)[:max(1, W * H // 12)]
        depth.reshape(-1)[sky] = AO_SKY_DEPTH
    n = np.stack([rng.uniform(-1, 1, (H, W)), rng.uniform(-1, 1, (H, W)), rng.uniform(0.15, 1, (H, W))], axis=-1)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    depth.setflags(write=False)
    normal = RM.encode_normal(n)
    normal.setflags(write=False)
    return depth, normal


def ao_want(W, H, resolution=None, stats=None, **kw):
    depth, normal = ao_inputs(W, H)
    return AM.generate(depth, normal, hilbert(), I16, PROJ, (W, H) if resolution is None else resolution, AO_FAR, stats=stats, **kw)


@functools.lru_cache(maxsize=None)
def ao_wide_counters(W, H):
    st = {}
    ao_want(W, H, stats=st, **AO_WIDE)
    c = AM.counters(st)
    c["sky_pixels"] = W * H - c["non_sky_pixels"]
    return c


@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
def test_ambient_occlusion_case_samples_every_level(extent):
    """The radius-400 run of every extent: samples counted at each of the five levels and at fractional levels, a non-sky pixel, and a sky
    pixel from 64 texels upwards."""
    c = ao_wide_counters(*extent)
    print(extent, c)
    for k in range(5):
        assert c[f"mip{k}"] > 0, (extent, k, c)
    assert c["fractional"] > 0 and c["non_sky_pixels"] >= 1, (extent, c)
    if extent[0] * extent[1] >= 64:
        assert c["sky_pixels"] >= 1, (extent, c)


def test_ambient_occlusion_sweep_is_not_degenerate():
    total = {}
    for W, H in EXTENTS:
        for k, v in ao_wide_counters(W, H).items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert total["result_partial"] > 1000 and total["sign_minus"] > 0 and total["sign_plus"] > 0, total


def test_ambient_occlusion_resolution_cases_differ_from_the_extent_run():
    """resolution != extent changes the image: the two cases cannot pass by ignoring the argument."""
    for (W, H), res in AO_RESOLUTIONS:
        a, b = ao_want(W, H, **AO_WIDE), ao_want(W, H, resolution=res, **AO_WIDE)
        assert (a["noisy_occlusion"] != b["noisy_occlusion"]).sum() > W * H // 4, res
        assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(a["levels"], b["levels"]))  # the prefilter does not read it


def test_ambient_occlusion_inputs_hold_no_poison():
    assert not holds(hilbert(), HILBERT_POISON, np.uint16)
    for W, H in EXTENTS:
        depth, normal = ao_inputs(W, H)
        assert not holds(depth, NAN32, np.uint32) and np.isfinite(depth).all() and not holds(normal, NAN16, np.uint16), (W, H)


# ---- contact shadows ------------------------------------------------------------------------------------------------------------------------
CS_STEPS = (1, 2, 64)
CS_SUNS = ((0.7, 0.6, 0.3), (-0.7, 0.6, 0.3), (0.7, -0.6, 0.3), (-0.7, -0.6, 0.3))  # one per quadrant of screen space
CS_SETTINGS = dict(thickness=8.0, shadow_length=4.0)  # rays of four units through surfaces 5 .. 30 units away: a quarter of the image wide
CS_NEAR = 0.1
# the classes test_contact_shadows_model.FLOORS names, and a hit that writes exactly 1.0
CS_CLASSES = ("sky", "miss", "hit_zero", "hit_partial", "hit_one", "rejected", "n_lower", "n_between", "n_upper", "end_clip")


def cs_cameras():
    """{name: (inv_projection_view, view, projection, near_clip)}: the 60 degree reversed-Z camera at the origin, and the rotated one."""
    from oxylus_amd.synth import perspective_reversed_z
    from test_gpu_contact_shadows import rotated_camera

    proj = perspective_reversed_z(60.0, 1.0, CS_NEAR, 1000.0).numpy()
    inv = np.linalg.inv(proj.astype(np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    return {"identity": (inv, I16.copy(), proj, CS_NEAR), "rotated": rotated_camera()}


@functools.lru_cache(maxsize=None)
def cs_depth(W, H):
    """A seeded reversed-Z depth of surfaces 5 .. 30 units away (depth = near / distance), about one texel in twelve sky (0.0)."""
    rng = np.random.default_rng(7000 + 1000 * W + H)
    depth = (F(CS_NEAR) / rng.uniform(5.0, 30.0, (H, W)).astype(np.float32)).astype(np.float32)
    if W * H >= 4:
        depth.reshape(-1)[rng.permutation(W * H)[:max(1, W * H // 12)]] = 0.0
    depth.setflags(write=False)
    return depth


def cs_runs():
    """(camera name, camera, steps, sun) of every run of one extent."""
    return [(name, cam, steps, sun) for name, cam in cs_cameras().items() for steps in CS_STEPS for sun in CS_SUNS]


@functools.lru_cache(maxsize=None)
def cs_extent_counts(W, H):
    total = {"left": 0, "right": 0, "top": 0, "bottom": 0}
    for _, (inv, view, proj, near), steps, sun in cs_runs():
        st = {}
        CM.contact_shadows(cs_depth(W, H), inv, view, proj, near, sun, steps=steps, stats=st, **CS_SETTINGS)
        for k, v in {**class_counts(st), **st["clamped_taps"]}.items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("extent", EXTENTS, ids=EXTENT_IDS)
def test_contact_shadows_case_clamps_at_all_four_sides(extent):
    """Over the runs of one extent (two cameras, three step counts, four suns): taps whose footprint is clamped at the left, right, top and
    bottom border, and from 15 x 15 upwards rays cut at the image border."""
    c = cs_extent_counts(*extent)
    print(extent, c)
    assert c["non_sky_pixels"] >= 1
    for side in ("left", "right", "top", "bottom"):
        assert c[side] > 0, (extent, side, c)
    if min(extent) >= 15:
        assert c["end_clip"] > 0, (extent, c)


def test_contact_shadows_sweep_is_not_degenerate():
    """Every outcome class occurs in the sweep: the ones the floors of tests/test_contact_shadows_model.py name and a hit that writes
    exactly 1.0.  (A moved start needs a pixel outside the clip volume; no image produces one, and it is not asked for there either.)"""
    total = {}
    for W, H in EXTENTS:
        for k, v in cs_extent_counts(W, H).items():
            total[k] = total.get(k, 0) + v
    print(total)
    for name in CS_CLASSES:
        assert total[name] > 0, (name, total)


def test_contact_shadows_inputs_hold_no_poison():
    for W, H in EXTENTS:
        assert not holds(cs_depth(W, H), NAN32, np.uint32) and np.isfinite(cs_depth(W, H)).all(), (W, H)


# ---- shadow resolve -------------------------------------------------------------------------------------------------------------------------
RESOLVE_SOURCE = 128  # Frame(renderer, 128, 128, seed=67) of tests/test_gpu_vsm_resolve.py


RESOLVE_FIRST_ROW = 32  # the rows above hold mostly sky: the horizon crosses the middle row, which a 1-high strip would otherwise land on


def resample_index(dim, first=0, source=RESOLVE_SOURCE):
    """Nearest neighbour: the source row / column in [first, source) under the centre of each of `dim` texels."""
    span = source - first
    return first + np.minimum(((np.arange(dim) * 2 + 1) * span) // (2 * dim), span - 1)


def resample(image, W, H):
    """[source, source, ...] -> [H, W, ...] by nearest neighbour, from the rows RESOLVE_FIRST_ROW .. source - 1 and every column."""
    return np.ascontiguousarray(np.asarray(image)[resample_index(H, RESOLVE_FIRST_ROW)][:, resample_index(W)])


def resolve_counts(st, got):
    oc = st["outcome"]
    c = {name: int((oc == k).sum()) for name, k in (("sky", RM.SKY), ("hard", RM.HARD), ("no_blocker", RM.NO_BLOCKER), ("all_blockers", RM.ALL_BLOCKERS),
                                                    ("pcf", RM.PCF))}
    c.update(non_sky=int((oc != RM.SKY).sum()), lit=int(((oc != RM.SKY) & (got == 1.0)).sum()), shadowed=int((got == 0.0).sum()),
             partial=int(((got > 0.0) & (got < 1.0)).sum()), taps=st["taps"], misses=st["misses"], fallback_minus=st["fallback_minus"],
             fallback_plus=st["fallback_plus"])
    return c


def assert_resolve_sweep_is_not_degenerate(per_extent: dict):
    """per_extent: {(W, H): resolve_counts}.  A non-sky pixel at every extent; over the sweep fully lit, fully shadowed and partial pixels
    and a tap served by a neighbouring clipmap."""
    total = {}
    for extent, c in per_extent.items():
        assert c["non_sky"] >= 1, (extent, c)
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert total["lit"] > 0 and total["shadowed"] > 0 and total["partial"] > 0 and total["fallback_minus"] + total["fallback_plus"] > 0, total
    return total


def resolve_frame_from_the_models():
    """The frame of tests/test_gpu_pixel_pass_edges.py -- Frame(renderer, 128, 128, seed=67, evict=True) of tests/test_gpu_vsm_resolve.py --
    made without a GPU: the oracle draws the depth, tests/vsm_pages_model.py fills the page table, tests/vsm_draw_model.py draws every
    triangle into the physical pages, and a third of the entries lose their Backed bit by the Frame's rule."""
    import torch

    import oracle
    import vsm_draw_model as DM
    import vsm_pages_model as VP
    from oxylus_amd.synth import normals_from_depth, pack_clipmaps, virtual_shadow_matrices
    from test_gpu_vsm_resolve import LIGHT, MAX_SHADOW_DIST, REFERENCE, Z_LENGTH, occluder_scene

    S, count, n, ps, phys = RESOLVE_SOURCE, REFERENCE["clipmap_count"], REFERENCE["page_table_size"], REFERENCE["page_size"], REFERENCE["physical_page_table_size"]
    s = occluder_scene(67)
    ml = s.meshlet_instances[:, 1].long()
    idx = torch.tensor([(i << 8) | c for i, m in enumerate(ml.tolist()) for c in range(3 * int(s.meshlets[m, 3]))], dtype=torch.int64).to(torch.int32)
    vd = torch.zeros((S, S), dtype=torch.int64)
    pv = [float(x) for x in s.camera["projection_view"]]
    oracle.draw_visbuffer(s, s.meshlet_instances, idx, pv, S, S, vd)
    depth = oracle.resolve_visbuffer(vd)[0].numpy()
    inv = np.linalg.inv(np.asarray(pv, np.float64).reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    mats, offs, zn = virtual_shadow_matrices(list(s.camera["position"]), LIGHT, MAX_SHADOW_DIST, 10.0, count, page_table_size=n)
    clip = pack_clipmaps(mats, offs, zn).numpy()
    up = VP.update(np.zeros((count, n, n), np.uint32), depth, inv, (S, S), clip, page_size=ps, physical_page_table_size=phys, count=count,
                   first_clipmap_width=10.0, virtual_extent=float(n * ps))
    image = DM.draw(VP.physical_image(np.zeros((phys, phys), np.float32), up["dirty"], ps), s, s.meshlet_instances.numpy(), idx.numpy(),
                    [idx.numel(), 1, 0, 0, 0], up["table"], clip, up["dirty_flags"], **REFERENCE)
    c, y, x = np.mgrid[0:count, 0:n, 0:n]
    table = up["table"] & np.where((7 * x + 13 * y + c) % 3 == 0, ~np.uint32(4), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    normal = normals_from_depth(torch.from_numpy(depth), inv, s.camera["position"]).numpy()
    return dict(depth=depth, normal=normal, table=table, clipmaps=clip, physical=image, inv=inv, light=LIGHT, z_length=Z_LENGTH,
                kw=dict(first_clipmap_width=10.0, virtual_extent=float(n * ps), **REFERENCE))


def test_resolve_sweep_is_not_degenerate():
    """The resolve checker over every extent of the sweep on the models' frame: a non-sky pixel at every extent, fully lit, fully shadowed
    and partial pixels and taps served by both neighbouring clipmaps over the sweep; no resampled input holds the poison."""
    f = resolve_frame_from_the_models()
    per = {}
    for W, H in EXTENTS:
        depth, normal = resample(f["depth"], W, H), resample(f["normal"], W, H)
        assert depth.shape == (H, W) and normal.shape == (H, W, 4)
        assert not holds(depth, NAN32, np.uint32) and np.isfinite(depth).all() and not holds(normal, NAN16, np.uint16), (W, H)
        st = {}
        got = RM.resolve(depth, normal, f["table"], f["clipmaps"], f["physical"], f["inv"], (W, H), f["light"], f["z_length"], stats=st, **f["kw"])
        per[(W, H)] = resolve_counts(st, got)
    total = assert_resolve_sweep_is_not_degenerate(per)
    assert total["fallback_minus"] > 0 and total["fallback_plus"] > 0 and total["misses"] > 0, total
