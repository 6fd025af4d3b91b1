"""Frames of oxc_decode_visbuffer_textured: images with mip chains built in numpy, sampler tables, quad meshes with texcoords under several
materials, hand-made visbuffers over them (the decode does not ask whether a pixel lies inside its triangle, so a texel may name any
triangle of the scene), the checker's answer and the GPU call, plain or between guard bands.  Run as a script it writes
tests/golden/textured_decode_17x9.npz: the inputs of one frame and the checker's four images and counters."""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import torch

import textured_decode_model as TM
from scenes import build_scene

F = np.float32
PRESETS = ("LinearRepeated", "LinearClamped", "NearestRepeated", "NearestClamped", "LinearRepeatedAnisotropy")
PRESET_RECORDS = {"LinearRepeated": (1, 0, 1), "LinearClamped": (1, 1, 1), "NearestRepeated": (0, 0, 0), "NearestClamped": (0, 1, 0),
                  "LinearRepeatedAnisotropy": (1, 0, 1)}
SIZES = ((1, 1, 1), (2, 2, 2), (5, 3, 3), (16, 16, 5))  # (width, height, levels): the last level of each is 1 x 1
ALL_IMAGES = 31
CAMERA = (0.25, -0.5, 1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textured_decode_17x9.npz")


# ---- images -------------------------------------------------------------------------------------------------------------------------------------
def chain(width: int, height: int, levels: int, fmt: int, seed: int) -> dict:
    """A mip chain of random bytes: every level differs from a box filter of the one below, so the level a pixel reads shows in its result."""
    rng = np.random.default_rng(seed)
    per = 2 if fmt == TM.RG8 else 4
    return dict(width=width, height=height, format=fmt,
                levels=[rng.integers(0, 256, (max(1, height >> k), max(1, width >> k), per), dtype=np.uint8) for k in range(levels)])


def image_set(fmt: int, seed: int = 7) -> list:
    """The four sizes of SIZES in one format."""
    return [chain(w, h, n, fmt, seed + i) for i, (w, h, n) in enumerate(SIZES)]


def five_images(seed: int = 11) -> list:
    """One 16 x 16 image with 5 levels per kind: albedo sRGB, normal Unorm, emissive sRGB, metallic-roughness Unorm, occlusion Unorm."""
    return [chain(16, 16, 5, fmt, seed + i) for i, fmt in enumerate((TM.SRGB, TM.UNORM, TM.SRGB, TM.UNORM, TM.UNORM))]


# ---- meshes, materials, scenes --------------------------------------------------------------------------------------------------------------------
QUAD_UV = ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0))


def quad_mesh(uv=QUAD_UV, z=-4.0, half=3.0):
    """(positions, triangles, smooth normals, texcoords): a quad in front of the identity-view camera that fills the view; `uv` None: no
    texcoord stream."""
    pos = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], dtype=np.float32)
    nrm = np.array([[-0.5, -0.5, 0.7], [0.5, -0.5, 0.7], [0.5, 0.5, 0.7], [-0.5, 0.5, 0.7]], dtype=np.float32)
    return pos, np.array([[0, 1, 2], [0, 2, 3]]), nrm, None if uv is None else np.asarray(uv)


def half_bits(a) -> np.ndarray:
    """float -> binary16 bits; an integer array is the bits themselves."""
    a = np.asarray(a)
    if np.issubdtype(a.dtype, np.integer):
        return a.astype(np.uint16)
    with np.errstate(all="ignore"):
        return a.astype(np.float32).astype(np.float16).view(np.uint16)


def materials(flags, image_indices=None, sampler_index=None, uv_size=None, uv_offset=None):
    """One material per entry of `flags`, factors that differ per material and per channel and are not 1."""
    from oxylus_amd.synth import pack_materials

    n = len(flags)
    k = np.arange(n, dtype=np.float32)[:, None]
    albedo = 0.35 + 0.6 * np.abs(np.sin(k * 1.7 + np.arange(4, dtype=np.float32)[None, :]))
    emissive = 0.25 + 1.5 * np.abs(np.cos(k * 0.9 + np.arange(3, dtype=np.float32)[None, :]))
    return pack_materials(albedo, emissive, roughness=0.3 + 0.6 * np.abs(np.sin(k[:, 0] + 1.0)), metallic=0.2 + 0.7 * np.abs(np.cos(k[:, 0] * 2.0)), flags=flags,
                          sampler_index=np.zeros(n) if sampler_index is None else sampler_index,
                          image_indices=np.tile(np.arange(5), (n, 1)) if image_indices is None else image_indices,
                          uv_size=np.ones((n, 2), np.float32) if uv_size is None else uv_size, uv_offset=np.zeros((n, 2), np.float32) if uv_offset is None else uv_offset)


def rebind(s, meshes):
    """Scene.bind() points every mesh at the one texcoord stream; a mesh built without texcoords gets its null pointer back."""
    s.bind()
    for i, m in enumerate(meshes):
        if m[3] is None:
            s.meshes[i, 2] = 0
    return s


def scene(meshes, instances, mats):
    """build_scene with texcoords: `meshes` = [(positions, triangles, normals, texcoords [V, 2] floats / half bits or None)]."""
    s, _ = build_scene([m[:3] for m in meshes], instances, mats)
    uv = [np.zeros((len(m[0]), 2), np.uint16) if m[3] is None else half_bits(m[3]).reshape(-1, 2) for m in meshes]
    s.texcoords = torch.from_numpy(np.concatenate(uv).view(np.int16).copy())
    return rebind(s, meshes)


WORLDS = {"identity": np.eye(4), "shear": np.array([[1.0, 0.25, 0.0, 0.25], [0.0, 0.5, 0.0, -0.5], [0.0, 0.0, 2.0, 4.0], [0.0, 0.0, 0.0, 1.0]])}


def view_matrix(tilt=0.0, scale=1.0):
    """A world matrix for the quad: scaled about its centre and tilted about the x axis there, so that uv gradients differ along the image."""
    c, s = np.cos(tilt), np.sin(tilt)
    to, back = np.eye(4), np.eye(4)
    to[2, 3], back[2, 3] = 4.0, -4.0
    rot = np.eye(4)
    rot[1, 1], rot[1, 2], rot[2, 1], rot[2, 2] = c, -s, s, c
    return back @ rot @ np.diag([scale, scale, scale, 1.0]) @ to


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Frame:
    cpu: object
    meshes: list
    vis: np.ndarray         # uint32 [H, W]
    depth: np.ndarray       # float32 [H, W]
    images: list            # model images (dict or None)
    samplers: list          # (filter, address, mip_filter)
    camera_position: tuple = CAMERA
    clear: bool = True

    @property
    def W(self):
        return self.vis.shape[1]

    @property
    def H(self):
        return self.vis.shape[0]


def assign(W: int, H: int, instances: int, mode: str = "bands", holes: bool = True) -> np.ndarray:
    """A visbuffer over `instances` one-meshlet quads: the triangle by the side of the image diagonal, the instance by `mode` -- "bands":
    16-pixel columns (every wave uniform), "pixels": a different instance in every pixel of a tile (needs >= 64), "mixed": bands in the
    upper half, pixels below.  `holes`: the first pixel of every third row is ~0u."""
    ys, xs = np.mgrid[0:H, 0:W]
    bands, pixels = (xs // 16) % instances, ((ys % 8) * 8 + xs % 8 + ys // 8 + xs // 8) % instances
    inst = {"bands": bands, "pixels": pixels, "mixed": np.where(ys < max(1, (H // 16) * 8), bands, pixels)}[mode]
    tri = (xs * H < ys * W).astype(np.uint32)
    vis = (inst.astype(np.uint32) << np.uint32(8)) | tri
    if holes and W * H > 2:
        vis[::3, 0] = 0xFFFFFFFF
    return vis


def frame(W: int, H: int, flags, mode="bands", images=None, samplers=(PRESET_RECORDS["LinearRepeated"],), meshes=None, worlds=None, mesh_of=None, clear=True,
          holes=True, **material_kw) -> Frame:
    """`len(flags)` instances, instance i with material i; mesh_of[i] names its mesh (default 0), worlds[i] its world matrix."""
    n = len(flags)
    meshes = [quad_mesh()] if meshes is None else meshes
    worlds = [view_matrix(0.35 + 0.01 * i, 1.0 + 0.03 * i) for i in range(n)] if worlds is None else worlds
    inst = [(0 if mesh_of is None else mesh_of[i], worlds[i], i) for i in range(n)]
    s = scene(meshes, inst, materials(flags, **material_kw))
    vis = assign(W, H, n, mode, holes)
    return Frame(s, meshes, vis, np.full((H, W), 0.5, np.float32), five_images() if images is None else images, list(samplers), clear=clear)


def exact_frame(W: int, H: int, flags, **kw) -> Frame:
    """`frame` over a quad whose corners project to the corners of the image with w = 1 under a matrix that passes x and y through: every
    quantity of steps 4 and 10 is a power of two or a pixel centre, so uv advances exactly 1 / W and 1 / H a pixel."""
    pos = np.array([[-1.0, -1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, 1.0]], dtype=np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (4, 1))
    f = frame(W, H, flags, meshes=[(pos, np.array([[0, 1, 2], [0, 2, 3]]), nrm, np.asarray(QUAD_UV))], worlds=[np.eye(4)] * len(flags), **kw)
    pv = np.zeros(16, np.float32)
    pv[0] = pv[5] = pv[11] = 1.0  # clip = (x, y, 0.25, z)
    pv[14] = 0.25
    f.cpu.camera = dict(f.cpu.camera, projection_view=[float(v) for v in pv])
    return f


def want(f: Frame, stats=None, init=None) -> dict:
    return TM.decode(f.cpu, f.cpu.meshlet_instances, f.vis, f.depth, f.cpu.camera["projection_view"], f.cpu.materials.numpy(), f.cpu.materials.numel() // 56,
                     clear=f.clear, init=init, stats=stats, camera_position=f.camera_position, images=f.images, samplers=f.samplers)


# ---- the GPU call ---------------------------------------------------------------------------------------------------------------------------------
POISON = {"albedo": 0xFFFFFFFB, "normal": 0xFFFB, "emissive": 0xFFFFFFFB, "mro": 0xFFFFFFFB}


def upload_images(images, offset=0):
    """(records, keep): model images as oxc_material_image records; None becomes an all-zero record.  `offset`: bytes in front of each
    image's texels inside its allocation (a multiple of 4), so the base takes every 4-byte alignment."""
    from oxylus_amd.renderer import pack_material_images

    real = [(im["levels"], im["format"] if im["format"] <= 2 else 0) for im in images if im is not None and im["levels"]]
    rec, keep = pack_material_images(real)
    rec = rec.cpu().numpy().reshape(-1, 144)
    out = np.zeros((len(images), 144), np.uint8)
    j, unread = 0, []
    for i, im in enumerate(images):
        if im is not None and im["levels"]:
            out[i] = rec[j]
            out[i].view(np.uint32)[[2, 3, 5]] = (im["width"], im["height"], im["format"])  # as the model image states them: a frame may misstate them
            j += 1
        elif im is not None:  # a record with levels == 0 over texels that must not be read: a live allocation of poison, so a read shows as a wrong word
            poison = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
            unread.append(poison)
            out[i].view(np.uint64)[0] = poison.data_ptr()
            out[i].view(np.uint32)[2:6] = (im["width"], im["height"], 0, im["format"])
    if offset:
        moved = []
        for i, t in enumerate(keep):
            big = torch.full((t.numel() + 64 + offset,), 0xA5, dtype=torch.uint8, device=t.device)
            base = -big.data_ptr() % 64 + offset  # 64-byte aligned, then `offset`
            big[base:base + t.numel()] = t
            moved.append(big)
            row = [k for k, im in enumerate(images) if im is not None and im["levels"]][i]
            out[row].view(np.uint64)[0] = big.data_ptr() + base
        keep = moved
    return torch.from_numpy(out.reshape(-1).copy()).cuda(), keep + unread


def contexts(r, f: Frame, guards=None, image_offset=0):
    """(decode context, images context, gpu scene, keep) for `f`; sets r.prepared_frame.  `guards`: {name: Guard} for the four outputs."""
    from oxylus_amd.renderer import MaterialImagesContext, PreparedFrame, VisbufferDecodeContext, pack_material_samplers

    gpu = rebind(f.cpu.to("cuda"), f.meshes)
    r.prepared_frame = PreparedFrame.create(gpu)
    vis = torch.from_numpy(f.vis.view(np.int32).copy()).cuda()
    depth = torch.from_numpy(f.depth.copy()).cuda()
    ctx = VisbufferDecodeContext.create(vis, depth, f.cpu.camera["projection_view"], gpu.n_meshlet_instances, gpu.materials, clear=f.clear)
    if guards:
        ctx.albedo_attachment, ctx.normal_attachment = guards["albedo"].tensor, guards["normal"].tensor
        ctx.emissive_attachment, ctx.metallic_roughness_occlusion_attachment = guards["emissive"].tensor, guards["mro"].tensor
    else:
        for t in (ctx.albedo_attachment, ctx.normal_attachment, ctx.emissive_attachment, ctx.metallic_roughness_occlusion_attachment):
            t.fill_(-5)
    rec, keep = upload_images(f.images, image_offset) if f.images else (None, [])
    smp = pack_material_samplers(f.samplers) if f.samplers else None
    return ctx, MaterialImagesContext.create(f.camera_position, rec, smp), gpu, keep


def init_images(f: Frame) -> dict:
    return {"albedo": np.full((f.H, f.W), POISON["albedo"], np.uint32), "normal": np.full((f.H, f.W, 4), POISON["normal"], np.uint16),
            "emissive": np.full((f.H, f.W), POISON["emissive"], np.uint32), "mro": np.full((f.H, f.W), POISON["mro"], np.uint32)}


def counted(r, ctx, images):
    from oxylus_amd import lib as L

    r.debug_set_tuning(L.TUNE_VISBUFFER_DECODE_TEXTURED_STATS, 1)
    try:
        r.decode_visbuffer_textured(ctx, images)
        return r.debug_visbuffer_decode_textured_stats()
    finally:
        r.debug_set_tuning(L.TUNE_VISBUFFER_DECODE_TEXTURED_STATS, 0)


def check(r, f: Frame, label="", **kw) -> dict:
    """One counting call and one plain call of `f`: every word of the four images and every counter equal the checker's.  Returns the
    checker's stats."""
    from gpu_passes import decode_got_of, same

    ctx, images, _gpu, _keep = contexts(r, f, **kw)
    st = {}
    expected = want(f, st, init_images(f))
    dev = counted(r, ctx, images)
    same(decode_got_of(ctx), expected, f"{label}: counting")
    assert dev == TM.counters(st), (label, dev, TM.counters(st))
    for t in (ctx.albedo_attachment, ctx.normal_attachment, ctx.emissive_attachment, ctx.metallic_roughness_occlusion_attachment):
        t.fill_(-5)
    r.decode_visbuffer_textured(ctx, images)
    same(decode_got_of(ctx), expected, f"{label}: plain")
    return st


# ---- the golden frame -----------------------------------------------------------------------------------------------------------------------------
def golden_frame() -> Frame:
    flags = [ALL_IMAGES, ALL_IMAGES | TM.FLIP_Y, 1 | 2 | TM.TWO_COMPONENT, 0]
    images = five_images() + [chain(5, 3, 3, TM.RG8, 23)]
    idx = np.tile(np.arange(5), (4, 1))
    idx[2, 1] = 5
    return frame(17, 9, flags, mode="pixels", images=images, samplers=[PRESET_RECORDS[p] for p in PRESETS], image_indices=idx, sampler_index=[0, 1, 2, 3],
                 uv_size=[[1.0, 1.0], [2.5, 0.75], [4.0, 4.0], [1.0, 1.0]], uv_offset=[[0.0, 0.0], [-0.25, 0.5], [0.125, 0.0], [0.0, 0.0]])


def main():
    f = golden_frame()
    st = {}
    img = want(f, st)
    np.savez_compressed(GOLDEN, vis=f.vis, **{"want_" + k: v for k, v in img.items()}, counters=np.array([TM.counters(st)[k] for k in TM.COUNTER_NAMES], np.int64))
    print(GOLDEN, TM.counters(st))


if __name__ == "__main__":
    main()
