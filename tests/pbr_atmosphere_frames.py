"""What the tests of oxc_apply_pbr_atmosphere share: the small Atmosphere records, the random sky images, the sun that looks straight at one
empty pixel, and one GPU call between guard bands.  Numpy only until `run` or `context` is called; the rule is pbr_atmosphere_model's, the
G-buffer scenes.synthetic_inputs', the guard bands gpu_passes'."""
import dataclasses

import numpy as np

import atmosphere_frames as AF
import pbr_atmosphere_model as AP
import sky_ibl_frames as SF
from pbr_apply_model import HAS_CONTACT_SHADOWS, HAS_DIRECTIONAL_LIGHT, TRANSPARENT_BACKGROUND
from scenes import CAMERA, INV_PV, PBR_SUN, SUN_INTENSITY, synthetic_inputs

F = np.float32
FILL_U32, FILL_U16 = 0xFFFFFFFB, 0xFFFB
ALL_READ = HAS_DIRECTIONAL_LIGHT | HAS_CONTACT_SHADOWS
TWO_LIGHTS = [dict(kind=1, position=(0.2, 0.1, 1.5), range=3.0, color=(1.0, 0.5, 0.25), intensity=8.0),
              dict(kind=2, position=(-0.5, 0.4, 2.0), direction=(0.3, -0.2, -1.0), inner_cone_angle=0.2, outer_cone_angle=0.5, range=0.0, intensity=20.0)]
# The synthetic frame's surfaces lie 2.3 .. 4.2 units (0.023 .. 0.042 km) from the camera.  "near": aerial perspective starts inside that
# range, so relative_depth is 0 for some pixels and a few metres for the others (the near-slice arm of the weight).  "far": it starts one
# kilometre behind the camera, so every pixel is past the near slice and between the two slices of the LUT.
STARTS = {"near": 0.03, "far": -1.0}


def atmosphere(start="near", transmittance=(5, 3), sky_view=(7, 4), aerial=(5, 3, 2), **overrides):
    """The engine's record at the small extents of the issue: 5 / 2 = 2.5 is not the producer's integer quotient."""
    return AF.small_atmosphere(transmittance=transmittance, sky_view=sky_view, aerial=aerial, aerial_perspective_start_km=STARTS.get(start, start),
                               aerial_perspective_exposure=1.5, **overrides)


def sky_images(A, cube_size=3, seed=21):
    """{transmittance, sky_view, aerial, cube}: random finite halves in the producers' layouts (colours in [-0.25, 1), alpha in [0, 4) for
    the sky view, [0, 1) elsewhere)."""
    t, v, a = A.transmittance_lut_size, A.sky_view_lut_size, A.aerial_perspective_lut_size
    return dict(transmittance=SF.random_lut(t[0], t[1], seed, alpha_scale=1.0, special=False), sky_view=SF.random_lut(v[0], v[1], seed + 1, special=False),
                aerial=np.stack([SF.random_lut(a[0], a[1], seed + 2 + z, alpha_scale=1.0, special=False) for z in range(a[2])]),
                cube=np.stack([SF.random_lut(cube_size, cube_size, seed + 100 + f, alpha_scale=2.0, special=False) for f in range(6)]))


def sun_at_empty_pixel(inp, inv_projection_view=INV_PV, camera_position=CAMERA):
    """(sun_dir, (y, x)): L = the -V the checker computes for the empty pixel that looks highest above the horizon, so that pixel sees the
    centre of the sun disc and no planet."""
    detail = {}
    A = atmosphere()
    AP.apply_pbr_atmosphere(inp["depth"], inp["albedo"], inp["normal"], inp["emissive"], inp["mro"], inp["ao"], None, None, 0, inv_projection_view,
                            camera_position, (0.0, 1.0, 0.0), 1.0, A, *sky_images(A).values(), detail=detail)
    nV = detail["sky_nV"]
    k = int(np.argmax(np.where(detail["sky_hit"], -np.inf, nV[1])))
    assert not detail["sky_hit"][k] and nV[1][k] > 0
    sky = np.flatnonzero(detail["sky"])
    return tuple(float(c[k]) for c in nV), (int(detail["ys"][sky[k]]), int(detail["xs"][sky[k]]))


def want(inp, flags, A, sky, lights=None, light_count=None, inv_projection_view=INV_PV, camera_position=CAMERA, sun_dir=PBR_SUN, sun_intensity=SUN_INTENSITY,
         counts=None, detail=None):
    """The checker's image for numpy inputs; lights a uint8 array of records or None."""
    return AP.apply_pbr_atmosphere(inp["depth"], inp["albedo"], inp["normal"], inp["emissive"], inp["mro"], inp["ao"],
                                   inp["resolved"] if flags & HAS_DIRECTIONAL_LIGHT else None, inp["contact"] if flags & HAS_CONTACT_SHADOWS else None, flags,
                                   inv_projection_view, camera_position, sun_dir, sun_intensity, A, sky["transmittance"], sky["sky_view"], sky["aerial"],
                                   sky["cube"], lights, light_count, counts, detail)[0]


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------------
def sky_guards(sky):
    return {k: SF.guard("sky_" + k, v) for k, v in sky.items()}


def out_guard(W, H, transparent):
    import torch

    from gpu_passes import Guard

    if transparent:
        return Guard("final", (H, W, 4), torch.int16, 4 * W, FILL_U16, 8, fill=FILL_U16)
    return Guard("final", (H, W), torch.int32, W, FILL_U32, 4, fill=FILL_U32)


def context(dev, flags, A, guards, out, lights=None, inv_projection_view=INV_PV, camera_position=CAMERA, sun_dir=PBR_SUN, sun_intensity=SUN_INTENSITY, **kw):
    """`dev`: gpu_passes.upload()'s tensors; `guards`: sky_guards(); `out`: the output tensor."""
    from oxylus_amd.renderer import ImageAttachment, PBRAtmosphereContext

    img = lambda t: None if t is None else ImageAttachment.depth(t)  # noqa: E731
    count = 0 if lights is None else lights.numel() * lights.element_size() // 64
    c = PBRAtmosphereContext(img(dev["depth"]), dev["albedo"], dev["normal"], dev["emissive"], dev["mro"], dev["ao"], img(dev["resolved"]), img(dev["contact"]), out,
                             int(flags), [float(x) for x in inv_projection_view], tuple(float(x) for x in camera_position), tuple(float(x) for x in sun_dir),
                             float(sun_intensity), AF.renderer_atmosphere(A), guards["transmittance"].tensor, guards["sky_view"].tensor, guards["aerial"].tensor,
                             guards["cube"].tensor, int(guards["cube"].tensor.shape[1]), lights, count)
    return dataclasses.replace(c, **kw) if kw else c


def got_of(out):
    import torch

    torch.cuda.synchronize()
    return out.bits()[1]


def run(r, inp, flags, A, sky, label, lights=None, dev=None, counts=None, expected=None, **camera):
    """One oxc_apply_pbr_atmosphere between guard bands: every word of the image equal to the checker's, every band and the four sky images
    untouched.  `lights`: a list of gpu_passes.lights_tensor's dicts.  Returns the image."""
    from gpu_passes import lights_tensor, same, upload

    H, W = inp["depth"].shape
    lt = lights_tensor(lights)
    if expected is None:
        expected = want(inp, flags, A, sky, None if lt is None else lt.cpu().numpy(), counts=counts, **camera)
    guards, out = sky_guards(sky), out_guard(W, H, flags & TRANSPARENT_BACKGROUND)
    ctx = context(upload(inp) if dev is None else dev, flags, A, guards, out.tensor, lt, **camera)
    r.apply_pbr_atmosphere(ctx)
    got = got_of(out).reshape(expected.shape)
    out.check(label, expected)
    same(got, expected, f"{label}: final_attachment")
    for k, g in guards.items():
        g.check(label)
        same(g.bits()[1].reshape(sky[k].shape), sky[k], f"{label}: {k} (input)")
    return got


def frame(W=33, H=17, seed=7):
    return synthetic_inputs(W, H, seed=seed)
