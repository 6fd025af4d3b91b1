"""Time oxc_apply_highlight (tools/, not bench.py) on the configs[2] scene drawn with its visbuffer, decoded, lit and tonemapped at --size
(3840x2160).  Selections: one mesh instance (the one that covers most pixels), 64 and 4096 instances (the most visible first), every covered
pixel (a copy of the mesh instances with one transform, selected), and no pixel (one entry no instance has).  For each it times the mask
alone, the composite alone and both in one call; then the same three calls at 16 x 16 (launch cost).  Prints one JSON line per row: ms per
call (HIP events around the call, median and minimum of --steps after --warmup), the bytes the stages must move -- the visbuffer in and the
mask words out; the colour image in and out (the mask words are 1/32 of either and depth is read under the outline only) -- and, with
--hbm-tbs, the time they take at that rate."""
import dataclasses
from types import SimpleNamespace

import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import HighlightContext, ImageAttachment, TonemapContext

STAGES = (("mask", L.HIGHLIGHT_MASK), ("composite", L.HIGHLIGHT_COMPOSITE), ("both", L.HIGHLIGHT_ALL))


def stage_bytes(stages, w, h):
    words = (w + 63) // 64 * h * 8
    return (w * h * 4 + words if stages & L.HIGHLIGHT_MASK else 0) + (w * h * 8 + words if stages & L.HIGHLIGHT_COMPOSITE else 0)


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv, hbm_help="HBM rate in TB/s for the streaming floor of each row (0: not reported)")
    r, dev = pf.renderer()
    lines = []

    W, H = pf.extent(args.size)
    s = pf.main_scene(r, args.meshlets, dev, materials=16)
    pf.draw_main(r, s, W, H, visbuffer=True)
    pf.decoded_frame(r, s)
    pf.shading_terms(s)
    pbr = pf.pbr_context(s, pf.light_records(s, 8), False)
    r.apply_pbr(pbr)
    tone = TonemapContext.create(pbr.final_attachment, 0, L.TONEMAP_ACES)
    r.apply_tonemap(tone)
    torch.cuda.synchronize()
    frame = r.prepared_frame

    # the transforms the frame shows, the one that covers most pixels first, then the rest of the scene's
    covered = s.vis.view(-1)[s.vis.view(-1) != -1].to(torch.int64)
    transforms = s.scene.mesh_instances[:, 3].to(torch.int64)
    shown, counts = torch.unique(transforms[frame.meshlet_instances_buffer[(covered >> 8) & 0xFFFFFF, 0].to(torch.int64)], return_counts=True)
    order = torch.cat([shown[torch.argsort(counts, descending=True)], transforms[~torch.isin(transforms, shown)]])
    sc = frame.scene
    one_transform = dataclasses.replace(frame, scene=SimpleNamespace(n_mesh_instances=sc.n_mesh_instances, meshes=sc.meshes, transforms=sc.transforms,
                                                                     mesh_instances=sc.mesh_instances.clone()))
    one_transform.scene.mesh_instances[:, 3] = 7
    u32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
    selections = [("one instance", frame, u32(order[:1])), ("64 instances", frame, u32(order[:64])), ("4096 instances", frame, u32(order[:4096])),
                  ("every covered pixel", one_transform, torch.tensor([7], dtype=torch.int32, device=dev)),
                  ("no pixel", frame, torch.tensor([-2], dtype=torch.int32, device=dev))]

    def rows(name, prepared, c, w, h):
        r.prepared_frame = prepared
        r.apply_highlight(c)  # the mask words the composite alone reads
        for stage, bits in STAGES:
            cs = dataclasses.replace(c, stages=bits)
            med, mn = pf.time_call(lambda: r.apply_highlight(cs), args.steps, args.warmup)
            nbytes = stage_bytes(bits, w, h)
            out = {"workload": "highlight", "call": "apply_highlight", "row": f"{name}, {stage}", "size": f"{w}x{h}", "selected_count": int(c.transform_indices.numel()),
                   "ms_median": med, "ms_min": mn, "bytes": nbytes}
            pf.streaming_floor(out, nbytes, args.hbm_tbs)
            pf.report(lines, out)

    for name, prepared, selected in selections:
        c = HighlightContext.over(s.vis, selected, s.M * s.K, s.depth, tone.dst_attachment)
        rows(name, prepared, c, W, H)
        torch.cuda.synchronize()
        bits = c.mask_bits.view(-1)
        set_bits = int(sum(int(((bits >> k) & 1).sum()) for k in range(64)))
        pf.report(lines, {"workload": "highlight", "row": f"{name}, selected pixels", "size": f"{W}x{H}", "pixels": set_bits})

    small = lambda t: t[:16, :16].contiguous()  # noqa: E731
    c16 = HighlightContext.over(small(s.vis), u32(order[:1]), s.M * s.K, ImageAttachment.depth(small(s.depth.data.view(H, W))), small(tone.dst_attachment))
    rows("one instance, 16 x 16", frame, c16, 16, 16)
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
