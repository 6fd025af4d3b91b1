"""Time oxc_decode_visbuffer_textured (tools/, not bench.py) on the decode row's frame, pass_frames.decode_context: the configs[2] scene with
random 10:10:10 normals and 16 materials, drawn at --size (3840x2160).  The scene has no texcoords of its own: every vertex takes the x and y
halves of its position as its texcoord, so uv varies smoothly over a mesh.  Rows: the old call (oxc_decode_visbuffer); the new call with no
image table; with the albedo image alone; with all five images, each --image-size (1024) square with its full mip chain, random bytes, sRGB
albedo and emissive; the same under a minified view -- the smallest power-of-two uv_size at which every decoded pixel of the frame has
lambda >= 3 -- and the five-image call on a 16 x 16 frame for the launch cost.  The lambda a row reaches is measured, not assumed: one extra
call per row samples a probe image whose level k holds alpha 20 k under albedo factors of 1, so the albedo attachment's alpha byte is
20 lambda; the row reports its minimum, median and maximum over the decoded pixels (resolution 0.05).  Prints one JSON line per row: ms
per call (HIP events around the call, median and minimum of --steps after --warmup) and, from one extra counting call, the counters of oxc_debug_visbuffer_decode_textured_stats.  With --hbm-tbs the streaming floor of the images the
call must move: 8 bytes read and 20 written per pixel (texels and geometry come on top and depend on the view).  The vector-issue estimate
follows from the ISA: DESIGN.md section 31."""
import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import MaterialImagesContext, pack_material_images, pack_material_samplers
from oxylus_amd.synth import pack_materials

FORMATS = (L.IMAGE_R8G8B8A8_SRGB, L.IMAGE_R8G8B8A8_UNORM, L.IMAGE_R8G8B8A8_SRGB, L.IMAGE_R8G8B8A8_UNORM, L.IMAGE_R8G8B8A8_UNORM)


def chains(size, rng):
    levels = int(np.log2(size)) + 1
    return [([rng.integers(0, 256, (max(1, size >> k), max(1, size >> k), 4), dtype=np.uint8) for k in range(levels)], fmt) for fmt in FORMATS]


def set_materials(s, n, flags, uv_size):
    """The 16 materials of the frame again, from a generator of their own, with `flags`, the five images 0 .. 4, sampler 0 and `uv_size`."""
    rng = np.random.default_rng(16)
    m = pack_materials(rng.random((n, 4)), rng.random((n, 3)) * 4.0, rng.random(n), rng.random(n), flags=[flags] * n, sampler_index=[0] * n,
                       image_indices=np.tile(np.arange(5), (n, 1)), uv_size=[[uv_size, uv_size]] * n, uv_offset=[[0.0, 0.0]] * n)
    s.scene.materials.copy_(m.to(s.dev))


def set_probe_materials(s, n, uv_size):
    """Every material: albedo (1, 1, 1, 1), the albedo image alone, image 0, sampler 0 and `uv_size`."""
    m = pack_materials(np.ones((n, 4)), flags=[1] * n, sampler_index=[0] * n, image_indices=np.zeros((n, 5)), uv_size=[[uv_size, uv_size]] * n,
                       uv_offset=[[0.0, 0.0]] * n)
    s.scene.materials.copy_(m.to(s.dev))


def measured_lod(r, s, c, probe, n, uv_size):
    """{min, median, max} of lambda over the decoded pixels at `uv_size`, from the probe image's alpha."""
    set_probe_materials(s, n, uv_size)
    r.decode_visbuffer_textured(c, probe)
    torch.cuda.synchronize()
    alpha = (c.albedo_attachment.view(torch.uint8).view(s.H, s.W, 4)[..., 3])[c.metallic_roughness_occlusion_attachment != 0].float() / 20.0
    return {"lambda_min": float(alpha.min()), "lambda_median": float(alpha.median()), "lambda_max": float(alpha.max())}


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--materials", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=1024)
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the floor (0: not reported)")
    r, dev = pf.renderer()
    lines = []
    rec, keep = pack_material_images(chains(args.image_size, np.random.default_rng(17)), dev)
    tables = MaterialImagesContext.create((0.0, 0.0, 0.0), rec, pack_material_samplers(["LinearRepeated"], dev))
    none = MaterialImagesContext.create((0.0, 0.0, 0.0))
    levels = int(np.log2(args.image_size)) + 1
    probe_levels = [np.full((max(1, args.image_size >> k),) * 2 + (4,), 20 * k, dtype=np.uint8) for k in range(levels)]
    probe_rec, probe_keep = pack_material_images([(probe_levels, L.IMAGE_R8G8B8A8_UNORM)], dev)
    probe = MaterialImagesContext.create((0.0, 0.0, 0.0), probe_rec, pack_material_samplers(["LinearRepeated"], dev))
    for size in (args.size, "16x16"):
        s = pf.main_scene(r, args.meshlets, dev, materials=args.materials)
        s.scene.texcoords = s.scene.positions[:, :2].contiguous().clone()  # the x and y halves of every position
        s.scene.bind()
        W, H = pf.extent(size)
        pf.draw_main(r, s, W, H, visbuffer=True)
        c = pf.decode_context(s)
        minified = 1.0
        while size == args.size and minified < 4096.0 and measured_lod(r, s, c, probe, args.materials, minified)["lambda_min"] < 3.0:
            minified *= 2.0
        rows = [("oxc_decode_visbuffer", None, 0, 1.0), ("no image table", none, 0, 1.0), ("albedo image", tables, 1, 1.0), ("five images", tables, 31, 1.0),
                ("five images, minified", tables, 31, minified)]
        for name, images, flags, uv_size in rows if size == args.size else rows[3:4]:
            lod = measured_lod(r, s, c, probe, args.materials, uv_size) if flags else {}
            set_materials(s, args.materials, flags, uv_size)
            call = (lambda: r.decode_visbuffer(c)) if images is None else (lambda images=images: r.decode_visbuffer_textured(c, images))
            med, mn = pf.time_call(call, args.steps, args.warmup)
            st = {}
            if images is not None:
                st = pf.counted_call(r, L.TUNE_VISBUFFER_DECODE_TEXTURED_STATS, call, r.debug_visbuffer_decode_textured_stats)
            row = {"workload": "textured_decode", "row": name, "size": size, "scene_meshlets": s.M * s.K, "materials": args.materials, "image_size": args.image_size,
                   "pixels": W * H, "uv_size": uv_size, **lod, "ms_median": med, "ms_min": mn, **st}
            pf.streaming_floor(row, 28 * W * H, args.hbm_tbs)
            pf.report(lines, row)
    del keep, probe_keep
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
