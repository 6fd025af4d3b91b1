"""What the terrain-draw tests share: the 24 x 20 baked heightmap of terrain_maps_frames (through terrain_decode_frames), terrains with the
patch grids 1 x 1, 3 x 2 and 8 x 8 over it, the cameras (straight down, oblique, grazing just above the surface, just below it), patch
lists with their indirect commands, one GPU call between guard bands and the checker's answer to it.  Numpy only until `run` is called;
the rules come from terrain_draw_model.  `python tests/terrain_draw_frames.py` writes the golden fixture
tests/golden/terrain_draw_33x19.npz (inputs and expected outputs only)."""
import dataclasses
import os

import numpy as np

import terrain_decode_frames as DF
import terrain_draw_model as TM

F = np.float32
POISON32 = 0xFFFFFFFB
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_draw_33x19.npz")
NEAR, SCALE = 0.5, 2.0
EXTENTS = ((1, 1), (17, 9), (33, 19), (129, 65))
GRIDS = ((1, 1), (3, 2), (8, 8))
OUTPUTS = ("visdepth", "depth", "vis")


def heightmap() -> np.ndarray:
    return DF.baked_maps()["heightmap"]


def terrain(patch_count=(3, 2), target_edge_pixels=16.0, max_tessellation=64.0, **kw):
    return dataclasses.replace(DF.terrain(**kw), patch_count=tuple(patch_count), target_edge_pixels=float(target_edge_pixels), max_tessellation=float(max_tessellation))


def look_at(H, eye, target, up_hint=(0.0, 1.0, 0.0), scale=SCALE, near=NEAR) -> TM.Camera:
    """A right-handed camera at `eye` looking at `target`, +y of the image down (Vulkan), reverse-Z with an infinite far plane (ndc.z =
    near / distance), the same field of view on both axes: projection_view as binary32 [16], column-major.  Straight down with up_hint
    (0, 0, -1) it is terrain_decode_frames.camera."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, np.asarray(up_hint, np.float64))
    r /= np.linalg.norm(r)
    up = np.cross(r, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = r, -up, -f  # view z negative ahead of the eye; the image's y runs against `up`
    view[:3, 3] = -view[:3, :3] @ eye
    proj = np.array([[scale, 0, 0, 0], [0, scale, 0, 0], [0, 0, 0, near], [0, 0, -1, 0]], np.float64)
    pv = (proj @ view).T.reshape(-1).astype(np.float32)
    return TM.Camera(pv, tuple(float(F(v)) for v in eye), float(F(near)), float(F(H * 0.5 * scale)))


def camera(name: str, W, H) -> TM.Camera:
    """down: the whole map and past its edges;  ground: straight down from low enough that only ground is in view;  oblique: only ground,
    seen at an angle;  grazing: a few units above the highest ground, looking along it (the clipper, big boxes);  below: under the surface,
    looking up at its back."""
    if name == "down":
        return look_at(H, (0.0, DF.CAMERA_HEIGHT, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    if name == "ground":
        return look_at(H, (30.0, 900.0, -20.0), (30.0, 0.0, -20.0), (0.0, 0.0, -1.0))
    if name == "oblique":
        return look_at(H, (-100.0, 500.0, -120.0), (40.0, 0.0, 30.0))
    if name == "grazing":
        return look_at(H, (-300.0, 420.0, -200.0), (400.0, 330.0, 300.0))
    assert name == "below"
    return look_at(H, (10.0, -50.0, 20.0), (40.0, 400.0, 60.0), (0.0, 0.0, 1.0))


def all_patches(T):
    n = int(T.patch_count[0]) * int(T.patch_count[1])
    return np.arange(n, dtype=np.uint32), np.array([4, n, 0, 0], np.uint32)


@dataclasses.dataclass
class Frame:
    T: object
    cam: TM.Camera
    W: int
    H: int
    heightmap: np.ndarray
    visible: np.ndarray   # uint32 [n]
    draw_cmd: np.ndarray  # uint32 [4]
    clear: bool = True
    before: np.ndarray = None  # uint64 [H, W]: the image before the call


def frame(extent=(33, 19), grid=(3, 2), cam="down", visible=None, draw_cmd=None, clear=True, before=None, hm=None, **terrain_kw) -> Frame:
    W, H = extent
    T = terrain(grid, **terrain_kw)
    v, c = all_patches(T)
    before = np.full((H, W), 0x3F00000012345678, np.uint64) if before is None else before  # depth 0.5 of a mesh texel everywhere
    return Frame(T, camera(cam, W, H) if isinstance(cam, str) else cam, W, H, heightmap() if hm is None else hm, v if visible is None else np.asarray(visible, np.uint32),
                 c if draw_cmd is None else np.asarray(draw_cmd, np.uint32), clear, before)


def want(f: Frame, counts=None) -> dict:
    img = TM.draw(f.T, f.heightmap, f.cam, f.visible, f.draw_cmd, f.W, f.H, image=f.before, clear=f.clear, counts=counts)
    depth, vis = TM.resolve(img)
    return {"visdepth": img, "depth": depth, "vis": vis}


def golden_frame() -> Frame:
    """The fixture: 33 x 19 pixels, the 3 x 2 grid seen obliquely, mixed factors."""
    return frame((33, 19), (3, 2), "oblique", target_edge_pixels=4.0)


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------------------
def guards(f: Frame) -> dict:
    import torch

    from gpu_passes import Guard

    W, H = f.W, f.H
    hm = f.heightmap
    return {
        "heightmap": Guard("heightmap", hm.shape, torch.int16, hm.shape[1], 0xFFFB, 2, data=hm),
        "visible": Guard("visible", (max(len(f.visible), 1),), torch.int32, 4, POISON32, 4, data=f.visible if len(f.visible) else np.zeros(1, np.uint32)),
        "draw_cmd": Guard("draw_cmd", (4,), torch.int32, 4, POISON32, 4, data=f.draw_cmd),
        "visdepth": Guard("visdepth", (H, 2 * W), torch.int32, 2 * W, POISON32, 8, data=f.before.view(np.uint32).reshape(H, 2 * W)),
        "depth": Guard("depth", (H, W), torch.float32, W, POISON32, 4, fill=0x7FC12345),
        "vis": Guard("vis", (H, W), torch.int32, W, POISON32, 4, fill=0x7FC12345),
    }


def context(f: Frame, gs: dict, resolves=True, **replace):
    import torch

    from oxylus_amd.renderer import ImageAttachment, TerrainDrawContext

    vd = gs["visdepth"].tensor.view(torch.int64).view(f.H, f.W)
    vis = gs["visible"].tensor  # (an empty list is one unused entry: the buffer may not be null)
    c = TerrainDrawContext(vd, [float(x) for x in f.cam.projection_view], f.cam.position, f.cam.near_clip, f.cam.projection_scale, DF.renderer_terrain(f.T),
                           (f.heightmap.shape[1], f.heightmap.shape[0]), gs["heightmap"].tensor, vis, gs["draw_cmd"].tensor, f.clear,
                           ImageAttachment.depth(gs["depth"].tensor) if resolves else None, gs["vis"].tensor if resolves else None)
    return dataclasses.replace(c, **replace)


def got_of(gs, f: Frame) -> dict:
    return {"visdepth": gs["visdepth"].bits()[1].view(np.uint64).reshape(f.H, f.W).copy(), "depth": gs["depth"].bits()[1].view(np.float32).reshape(f.H, f.W).copy(),
            "vis": gs["vis"].bits()[1].reshape(f.H, f.W).copy()}


def check_unwritten(gs, f: Frame, label):
    """Nothing written: the image holds its earlier bytes, the resolves their pre-fill, every band its poison."""
    from gpu_passes import same

    for g in gs.values():
        g.check(label)
    got = got_of(gs, f)
    same(got["visdepth"], f.before, f"{label}: visdepth written after a refusal")
    assert (got["vis"] == 0x7FC12345).all() and (got["depth"].view(np.uint32) == 0x7FC12345).all(), f"{label}: a resolve written after a refusal"


def run(r, f: Frame, label, counts=None, stats=True) -> dict:
    """One oxc_draw_terrain between guard bands: every word of visdepth, depth and vis and every counter equal to the checker's, every input
    unchanged, the bands untouched.  With `stats` the call runs the counting instantiations and the fragment counter is compared too; without,
    the plain kernels run and that counter stays 0.  Returns the outputs."""
    import torch

    from gpu_passes import same

    from oxylus_amd import lib as L

    counts = {} if counts is None else counts
    gs = guards(f)
    r.debug_set_tuning(L.TUNE_TERRAIN_DRAW_STATS, 1 if stats else 0)  # with `stats` the counting instantiations run: the fragment counter
    try:
        r.draw_terrain_for_visbuffer(context(f, gs))
    finally:
        r.debug_set_tuning(L.TUNE_TERRAIN_DRAW_STATS, 0)
    torch.cuda.synchronize()
    for g in gs.values():
        g.check(label)
    got, w = got_of(gs, f), want(f, counts)
    same(got, w, label)
    for name, a in (("heightmap", f.heightmap.view(np.uint16)), ("draw_cmd", f.draw_cmd)) + ((("visible", f.visible),) if len(f.visible) else ()):
        same(gs[name].bits()[1], np.ascontiguousarray(a).reshape(-1), f"{label}: input {name}")
    s = r.debug_terrain_draw_stats()
    assert {k: s[k] for k in TM.STATS} == {k: counts[k] for k in TM.STATS}, (label, s, counts)
    assert s["fragments"] == (counts["fragments"] if stats else 0), (label, s["fragments"], counts["fragments"])
    return got


if __name__ == "__main__":
    f = golden_frame()
    stored = {"heightmap": f.heightmap, "visible": f.visible, "draw_cmd": f.draw_cmd, "before": f.before, "pv": f.cam.projection_view,
              "camera": np.array(list(f.cam.position) + [f.cam.near_clip, f.cam.projection_scale], np.float32)}
    stored.update({"out_" + k: v for k, v in want(f).items()})
    np.savez_compressed(GOLDEN, **stored)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
