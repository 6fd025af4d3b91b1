"""The frames of the debug view tests: hand-made visbuffer, depth, overdraw, G-buffer and ambient-occlusion images with a small record
chain, the checker's call over them and the GPU call between guard bands.  The rules come from debug_view_model, the guard bands from
gpu_passes.  `python tests/debug_view_frames.py` writes the golden fixture tests/golden/debug_view_17x9.npz: the 17 x 9 frame's inputs and
the fourteen main views' outputs."""
import dataclasses
import os
import types

import numpy as np

import debug_view_model as DV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debug_view_17x9.npz")
POISON32, POISON16 = 0xFFFFFFFB, 0xFFFB
FILL16 = 0xFFFB  # the output's pre-fill: a NaN half no view stores (a NaN is stored as 0x7E00)
EXTENTS = [(1, 1), (2, 1), (15, 17), (16, 16), (17, 9), (33, 19), (129, 65)]
TERRAIN_TEXEL = 0xFFFFFE00
IMAGES = ("vis", "depth", "overdraw", "albedo", "normal", "emissive", "mr_occlusion", "ao")
RECORDS = ("meshlet_instances", "mesh_instances", "meshes")
READS = {DV.OVERDRAW: "overdraw", DV.ALBEDO: "albedo", DV.NORMAL: "normal", DV.GEOMETRIC_NORMAL: "normal", DV.EMISSIVE: "emissive", DV.METALLIC: "mr_occlusion",
         DV.ROUGHNESS: "mr_occlusion", DV.BAKED_OCCLUSION: "mr_occlusion", DV.GTAO: "ao"}


@dataclasses.dataclass
class Frame:
    vis: np.ndarray        # uint32 [H, W]
    depth: np.ndarray      # float32 [H, W]
    overdraw: np.ndarray   # uint32 [H, W]
    albedo: np.ndarray     # uint32 [H, W]
    normal: np.ndarray     # uint16 [H, W, 4]
    emissive: np.ndarray   # uint32 [H, W]
    mr_occlusion: np.ndarray        # uint32 [H, W]
    ao: np.ndarray         # uint16 [H, W]
    meshlet_instances: np.ndarray  # uint32 [N, 2]
    mesh_instances: np.ndarray     # uint32 [M, 5]
    meshes: np.ndarray             # uint32 [K, 16]: GPU::Mesh, lod_count in word 7
    meshlet_instance_count: int
    heatmap_scale: float = 10.0

    @property
    def extent(self):
        return self.vis.shape[1], self.vis.shape[0]


def record_chain(seed=5, n=12, m=5, k=3):
    """n meshlet instances over m mesh instances over k meshes with 1, 3 and 7 LODs; every material, mesh and LOD index occurs."""
    rng = np.random.default_rng(seed)
    mli = np.stack([np.arange(n) % m, rng.integers(0, 9, n)], axis=-1).astype(np.uint32)
    mi = np.zeros((m, 5), np.uint32)
    mi[:, 0] = np.arange(m) % k                     # mesh_index
    mi[:, 2] = (np.arange(m) * 7 + 2) % 11          # material_index
    mi[:, 3] = np.arange(m)
    meshes = rng.integers(0, 2 ** 32, (k, 16), dtype=np.uint64).astype(np.uint32)  # every word but lod_count is noise the view must not read
    meshes[:, 7] = (1, 3, 7)[:k]
    mi[:, 1] = np.arange(m) % np.maximum(meshes[mi[:, 0], 7], 1)  # lod_index below its mesh's lod_count
    return mli, mi, meshes


def frame(extent=(17, 9), seed=3, empty=0.2, terrain=0.1, n=12) -> Frame:
    """Random texels of n meshlet instances with `empty` ~0u and `terrain` terrain texels, depths in (0, 1), random words in every image."""
    W, H = extent
    rng = np.random.default_rng(seed + 1000 * W + H)
    u32 = lambda: rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)  # noqa: E731
    vis = ((rng.integers(0, n, (H, W)).astype(np.uint32) << np.uint32(8)) | rng.integers(0, 64, (H, W)).astype(np.uint32)).astype(np.uint32)
    # ~0u in the upper right corner and a few single texels, terrain in the lower left corner: a missing neighbour is a depth edge of its own
    # (the outline there is far above 1), so the empty texels are kept together
    y, x = np.mgrid[0:H, 0:W]
    vis[(x >= W - max(1, int(W * empty))) & (y < max(1, H // 3))] = DV.EMPTY
    vis[(x < max(1, int(W * terrain * 2))) & (y >= H - max(1, H // 3))] = TERRAIN_TEXEL | 3
    vis[rng.random((H, W)) < 0.02] = DV.EMPTY
    # a slope whose outline stays below 1, and one step across the middle column whose outline is far above it
    depth = (np.float32(0.3) + np.float32(0.002) * x.astype(np.float32) + np.float32(0.0013) * y.astype(np.float32) + np.float32(0.3) * (x >= W // 2)).astype(np.float32)
    normal = np.float16(rng.uniform(-1, 1, (H, W, 4))).view(np.uint16)
    ao = np.float16(rng.random((H, W))).view(np.uint16)
    mli, mi, meshes = record_chain(n=n)
    return Frame(vis, depth, rng.integers(0, 40, (H, W)).astype(np.uint32), u32(), normal, u32(), u32(), ao, mli, mi, meshes, n)


def golden_frame() -> Frame:
    return frame((17, 9))


def model_inputs(f: Frame, view) -> dict:
    """The checker's keyword arguments: only what `view` reads."""
    kw = {}
    if view == DV.OVERDRAW:
        kw["heatmap_scale"] = f.heatmap_scale
    if view in READS:
        kw[READS[view]] = getattr(f, READS[view])
    if view in DV.RECORD_VIEWS:
        kw.update(meshlet_instance_count=f.meshlet_instance_count, meshlet_instances=f.meshlet_instances, mesh_instances=f.mesh_instances, meshes=f.meshes)
    return kw


def want(f: Frame, view, clear=True, init=None, stats=None) -> np.ndarray:
    return DV.debug_view(view, f.vis, f.depth, clear=clear, init=init, stats=stats, **model_inputs(f, view))


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------------
def read_by(view) -> tuple:
    names = ("depth",) if view == DV.RMVSM else ("vis", "depth")
    names += (READS[view],) if view in READS else ()
    return names + (RECORDS if view in DV.RECORD_VIEWS else ())


def guards(f: Frame, view, poisoned_rest=False) -> dict:
    """Guarded tensors of what `view` reads -- with `poisoned_rest` also of every other input, holding poison only -- and of the output."""
    import torch

    from gpu_passes import Guard

    W, H = f.extent
    gs = {}
    for name in IMAGES + RECORDS:
        a = getattr(f, name)
        mine = name in read_by(view)
        if not mine and not poisoned_rest:
            continue
        if a.dtype == np.uint16:
            row, align = (W * 4, 8) if a.ndim == 3 else (W, 2)
            data = a if mine else np.full(a.shape, POISON16, np.uint16)
            gs[name] = Guard(name, a.shape, torch.int16, row, POISON16, align, data=data)
        else:
            row = W if name in IMAGES else a.shape[1]
            data = a if mine else np.full(a.shape, POISON32, np.uint32).view(a.dtype)
            gs[name] = Guard(name, a.shape, torch.float32 if a.dtype == np.float32 else torch.int32, row, POISON32, 8 if name == "meshes" else 4, data=data)
    gs["debug"] = Guard("debug", (H, W, 4), torch.int16, W * 4, POISON16, 8, fill=FILL16)
    return gs


def prepared_frame(gs: dict, f: Frame):
    """A PreparedFrame over the guarded record buffers; what the view does not read stays null."""
    from oxylus_amd.renderer import PreparedFrame

    t = lambda name: gs[name].tensor if name in gs else None  # noqa: E731
    scene = types.SimpleNamespace(n_mesh_instances=len(f.mesh_instances), meshes=t("meshes"), transforms=None, mesh_instances=t("mesh_instances"))
    return PreparedFrame(scene, f.meshlet_instance_count, t("meshlet_instances"), None, None, None)


def context(f: Frame, gs: dict, view, clear=True, **replace):
    from oxylus_amd.renderer import DebugViewContext, ImageAttachment

    t = lambda name: gs[name].tensor if name in gs else None  # noqa: E731
    c = DebugViewContext(int(view), ImageAttachment.depth(t("depth")), t("debug"), visbuffer_attachment=t("vis"), clear=clear, heatmap_scale=f.heatmap_scale,
                         meshlet_instance_count=f.meshlet_instance_count, overdraw_attachment=t("overdraw"), albedo_attachment=t("albedo"),
                         normal_attachment=t("normal"), emissive_attachment=t("emissive"), metallic_roughness_occlusion_attachment=t("mr_occlusion"),
                         ambient_occlusion_attachment=t("ao"))
    return dataclasses.replace(c, **replace)


def got_of(gs, f: Frame) -> np.ndarray:
    W, H = f.extent
    return gs["debug"].bits()[1].reshape(H, W, 4).copy()


def check_unwritten(gs, f: Frame, label):
    """Nothing written: the output holds its pre-fill, every band its poison."""
    for g in gs.values():
        g.check(label)
    assert (got_of(gs, f) == FILL16).all(), f"{label}: written after a refusal"


def run(r, f: Frame, view, label, clear=True, poisoned_rest=False, stats=None) -> np.ndarray:
    """One oxc_apply_debug_view between guard bands: every word of the output equal to the checker's (a discarded pixel keeping the pre-fill
    without `clear`), every input unchanged, the bands untouched.  Returns the output."""
    import torch

    from gpu_passes import same

    W, H = f.extent
    gs = guards(f, view, poisoned_rest)
    r.prepared_frame = prepared_frame(gs, f) if view in DV.RECORD_VIEWS or poisoned_rest else None
    r.apply_debug_view(context(f, gs, view, clear))
    torch.cuda.synchronize()
    for g in gs.values():
        g.check(label)
    got = got_of(gs, f)
    same(got, want(f, view, clear, np.full((H, W, 4), FILL16, np.uint16), stats), label)
    for name in read_by(view):
        a = getattr(f, name)
        same(gs[name].bits()[1], np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.uint16 else np.uint32).reshape(-1), f"{label}: input {name}")
    return got


# ---- the RMVSM view ---------------------------------------------------------------------------------------------------------------------------
SMALL = dict(page_size=16, page_table_size=8, physical_page_table_size=64, clipmap_count=3)
SECOND = dict(page_size=64, page_table_size=16, physical_page_table_size=512, clipmap_count=4)


@dataclasses.dataclass
class VsmFrame:
    depth: np.ndarray     # float32 [H, W]
    table: np.ndarray     # uint32 [count, n, n]
    clipmaps: np.ndarray  # uint8 [count * 76]
    inv_pv: np.ndarray    # float32 [16]
    shape: dict
    first_clipmap_width: float
    bias: float = -1.5

    @property
    def extent(self):
        return self.depth.shape[1], self.depth.shape[0]

    @property
    def settings(self):
        W, H = self.extent
        return dict(first_clipmap_width=self.first_clipmap_width, virtual_extent=float(self.shape["page_table_size"] * self.shape["page_size"]), **self.shape), (W, H)


def vsm_frame(extent=(17, 9), shape=SMALL, seed=9, widths=(2.0, 4.0, 8.0, 16.0), sky=0.15, nan_clipmap=None, depth=None) -> VsmFrame:
    """A camera whose unprojection is (ndc.xy / depth, 1): the footprint, and with it the clipmap, changes with the depth, and small depths land
    outside the orthographic clipmaps of `widths`.  Every page-table entry has random flag bits.  `nan_clipmap`: that clipmap's matrix is all
    zero, so its clip_uv is 0 / 0."""
    import vsm_resolve_model as RM

    W, H = extent
    count, n = shape["clipmap_count"], shape["page_table_size"]
    rng = np.random.default_rng(seed + 1000 * W + H)
    if depth is None:
        depth = (np.float32(0.25) + np.float32(0.75) * rng.random((H, W)).astype(np.float32)).astype(np.float32)
        depth[rng.random((H, W)) < sky] = 0.0
    table = (rng.integers(0, 8, (count, n, n)).astype(np.uint32) | (rng.integers(0, 16, (count, n, n)).astype(np.uint32) << np.uint32(16))).astype(np.uint32)
    clipmaps = RM.ortho_clipmaps(count, widths[:count], offsets=rng.integers(-20, 20, (count, 2)).astype(np.int32))
    if nan_clipmap is not None:
        clipmaps.view(np.float32).reshape(count, 19)[nan_clipmap, :16] = 0.0
    inv_pv = np.zeros(16, np.float32)
    inv_pv[0] = inv_pv[5] = 1.0   # x, y
    inv_pv[14] = 1.0              # z = 1
    inv_pv[11] = 1.0              # w = depth
    # thresholds 2^1.5 and 2^2.5 inside the footprint's range over depths 0.25 .. 1
    fcw = (2.0 / W) / 2.0 * (n * shape["page_size"]) / (2.0 * (n - 1) / n)
    return VsmFrame(np.ascontiguousarray(depth, np.float32), table, clipmaps, inv_pv, dict(shape), float(np.float32(fcw)))


def vsm_want(f: VsmFrame, stats=None) -> np.ndarray:
    settings, resolution = f.settings
    return DV.rmvsm(f.depth, f.table, f.clipmaps, f.inv_pv, resolution, bias=f.bias, stats=stats, **settings)


def vsm_guards(f: VsmFrame) -> dict:
    import torch

    from gpu_passes import Guard

    W, H = f.extent
    n = f.shape["page_table_size"]
    return {"depth": Guard("depth", (H, W), torch.float32, W, POISON32, 4, data=f.depth),
            "table": Guard("table", f.table.shape, torch.int32, n, POISON32, 4, data=f.table),
            "clipmaps": Guard("clipmaps", (len(f.clipmaps) // 4,), torch.int32, 19, POISON32, 4, data=f.clipmaps.view(np.uint32)),
            "debug": Guard("debug", (H, W, 4), torch.int16, W * 4, POISON16, 8, fill=FILL16)}


def vsm_context(f: VsmFrame, gs: dict, **replace):
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import DebugViewContext, ImageAttachment

    settings, resolution = f.settings
    c = DebugViewContext(L.DEBUG_VIEW_RMVSM, ImageAttachment.depth(gs["depth"].tensor), gs["debug"].tensor, vsm_clipmaps_buffer=gs["clipmaps"].tensor,
                         virtual_page_table=gs["table"].tensor, inv_projection_view=tuple(float(x) for x in f.inv_pv), resolution=tuple(float(x) for x in resolution),
                         clipmap_selection_bias=f.bias, **settings)
    return dataclasses.replace(c, **replace)


def run_vsm(r, f: VsmFrame, label, stats=None) -> np.ndarray:
    """One RMVSM call between guard bands: every word equal to the checker's (no pixel keeps the pre-fill), inputs and bands untouched."""
    import torch

    from gpu_passes import same

    W, H = f.extent
    gs = vsm_guards(f)
    r.prepared_frame = None
    r.apply_debug_view(vsm_context(f, gs))
    torch.cuda.synchronize()
    w = vsm_want(f, stats)
    for g in gs.values():
        g.check(label, w if g.name == "debug" else None)
    got = gs["debug"].bits()[1].reshape(H, W, 4).copy()
    same(got, w, label)
    return got


if __name__ == "__main__":
    f = golden_frame()
    stored = {"in_" + name: getattr(f, name) for name in IMAGES + RECORDS}
    stored["meshlet_instance_count"] = np.uint32(f.meshlet_instance_count)
    stored["heatmap_scale"] = np.float32(f.heatmap_scale)
    stored.update({"out_" + DV.NAMES[view]: want(f, view) for view in DV.MAIN_VIEWS})
    np.savez_compressed(GOLDEN, **stored)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
