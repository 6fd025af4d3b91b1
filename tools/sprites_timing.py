"""Time oxc_draw_sprites (tools/, not bench.py) at --size (3840x2160) and at 16 x 16 over a constant depth and a random lit B10G11R11 image, for
the vis stage, the colour stage and both in one call, on four sprite lists: none; 10 000 sprites of about 16 px, scattered; 1 000 sprites
of about 256 px; 64 full-screen translucent layers (the overdraw worst case).  All sprites lie at one depth in front of the scene, so every
fragment passes in every repeat (the call writes the depth it tests: later repeats see the sprites' own depth, which `>=` still passes), and
the colour stage blends every fragment.  Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of
--steps after --warmup), the fragments of the list, and the bytes a call must at least move -- depth in and out, the visbuffer out, the
colour image in and out, counted over the whole image -- with, under --hbm-tbs, the time they take at that rate."""
import dataclasses
import math
from types import SimpleNamespace

import numpy as np
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import ImageAttachment, PreparedFrame, SpriteContext, pack_sprite

STAGES = (("vis", L.SPRITES_VIS), ("color", L.SPRITES_COLOR), ("both", L.SPRITES_ALL))


def quads(w, h, n, size, rng, full=False):
    """n column-major world matrices that put the unit sprite on about `size` pixels at a random place and angle (identity projection_view),
    all at depth 0.5; `full`: over the whole image."""
    m = np.zeros((n, 4, 4), np.float32)
    ang = np.zeros(n) if full else rng.uniform(0, math.pi, n)
    sw, sh = (np.full(n, 2.0 * w), np.full(n, 2.0 * h)) if full else (rng.uniform(0.75, 1.25, n) * size, rng.uniform(0.75, 1.25, n) * size)
    cx, cy = (np.full(n, w / 2.0), np.full(n, h / 2.0)) if full else (rng.uniform(0, w, n), rng.uniform(0, h, n))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 3] = np.cos(ang) * sw * 2 / w, -np.sin(ang) * sh * 2 / w, cx * 2 / w - 1
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 3] = np.sin(ang) * sw * 2 / h, np.cos(ang) * sh * 2 / h, cy * 2 / h - 1
    m[:, 2, 2], m[:, 2, 3], m[:, 3, 3] = 1.0, 0.5, 1.0
    return np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(n, 16)


def materials(dev):
    from oxylus_amd.synth import pack_materials

    rng = np.random.default_rng(2)
    albedo = torch.from_numpy(np.concatenate([rng.uniform(0, 1, (16, 3)), rng.uniform(0.2, 0.8, (16, 1))], axis=1).astype(np.float32))
    return pack_materials(albedo, alpha_cutoff=torch.zeros(16)).to(dev)


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv, hbm_help="HBM rate in TB/s for the streaming floor of each row (0: not reported)")
    r, dev = pf.renderer()
    lines = []
    mats = materials(dev)
    identity = tuple(np.eye(4, dtype=np.float32).reshape(16))

    def rows(w, h, lists):
        for name, n, size, full in lists:
            rng = np.random.default_rng(7 + n)
            world = torch.from_numpy(quads(w, h, max(n, 1), size, rng, full)).to(dev)
            sprites = torch.from_numpy(np.array([pack_sprite(0, 0.0, k, k % 16, 1.0) for k in range(n)], np.uint32).reshape(-1, 3).view(np.int32)).to(dev)
            if n == 0:
                sprites = torch.zeros((1, 3), dtype=torch.int32, device=dev)
            depth = torch.full((h, w), 0.25, dtype=torch.float32, device=dev)
            lit = torch.from_numpy(np.random.default_rng(3).integers(0, 1 << 30, (h, w), dtype=np.int64).astype(np.int32)).to(dev)
            r.prepared_frame = PreparedFrame(SimpleNamespace(n_mesh_instances=0, meshes=None, transforms=world, mesh_instances=None), 0, None, None, None, None)
            c = SpriteContext.create(sprites, mats, max(n, 1), identity, ImageAttachment.depth(depth), lit, sprite_count=n)
            r.draw_sprites(c)
            torch.cuda.synchronize()
            covered = int((c.visbuffer_2d != -1).sum())
            for stage, bits in STAGES:
                cs = dataclasses.replace(c, stages=bits)
                med, mn = pf.time_call(lambda: r.draw_sprites(cs), args.steps, args.warmup)
                nbytes = w * h * (8 + (4 if bits & L.SPRITES_VIS else 0) + (8 if bits & L.SPRITES_COLOR else 0)) if n else (w * h * 4 if bits & L.SPRITES_VIS else 0)
                out = {"workload": "sprites", "call": "draw_sprites", "row": f"{name}, {stage}", "size": f"{w}x{h}", "sprite_count": n, "covered_pixels": covered,
                       "ms_median": med, "ms_min": mn, "bytes": nbytes}
                pf.streaming_floor(out, nbytes, args.hbm_tbs)
                pf.report(lines, out)

    W, H = pf.extent(args.size)
    rows(W, H, [("no sprites", 0, 0, False), ("10000 sprites of 16 px", 10000, 16, False), ("1000 sprites of 256 px", 1000, 256, False), ("64 full-screen layers", 64, 0, True)])
    rows(16, 16, [("no sprites", 0, 0, False), ("10000 sprites of 16 px", 10000, 16, False), ("64 full-screen layers", 64, 0, True)])
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
