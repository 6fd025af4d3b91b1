"""Time oxc_apply_debug_view (tools/, not bench.py) on the decode row's frame: the configs[2] scene drawn with its visbuffer and decoded at
--size (3840x2160), a random ambient-occlusion image and a random overdraw count image beside it.  Rows: one id view (Meshlets), MeshLods
(the record chain), Overdraw, Albedo, GTAO, the RMVSM view on the shadow draw's frame, and the Meshlets call at 16 x 16 (launch cost).
Prints one JSON line per row: ms per call (HIP events around the call, median and minimum of --steps after --warmup), the bytes the view
reads and writes and, with --hbm-tbs, the time they take at that rate."""
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L
from oxylus_amd.renderer import DebugViewContext, ImageAttachment

# bytes per pixel a view reads beside the visbuffer and the depth (4 + 4) and the output (8)
EXTRA_BYTES = {L.DEBUG_VIEW_MESHLETS: 0, L.DEBUG_VIEW_MESH_LODS: 0, L.DEBUG_VIEW_OVERDRAW: 4, L.DEBUG_VIEW_ALBEDO: 4, L.DEBUG_VIEW_GTAO: 2}
NAMES = {L.DEBUG_VIEW_MESHLETS: "Meshlets", L.DEBUG_VIEW_MESH_LODS: "MeshLods", L.DEBUG_VIEW_OVERDRAW: "Overdraw", L.DEBUG_VIEW_ALBEDO: "Albedo",
         L.DEBUG_VIEW_GTAO: "GTAO"}


def main(argv=None):
    ap = pf.common_arguments()
    args = pf.parse(ap, argv, hbm_help="HBM rate in TB/s for the streaming floor of each row (0: not reported)")
    r, dev = pf.renderer()
    lines = []

    W, H = pf.extent(args.size)
    s = pf.main_scene(r, args.meshlets, dev, materials=16)
    frame = r.prepared_frame
    pf.draw_main(r, s, W, H, visbuffer=True)
    pf.decoded_frame(r, s)
    pf.shading_terms(s)
    overdraw = torch.randint(0, 32, (H, W), generator=s.g, device=dev, dtype=torch.int32)

    def row(name, c, w, h, nbytes):
        med, mn = pf.time_call(lambda: r.apply_debug_view(c), args.steps, args.warmup)
        out = {"workload": "debug_view", "call": "apply_debug_view", "row": name, "size": f"{w}x{h}", "ms_median": med, "ms_min": mn, "bytes": nbytes}
        pf.streaming_floor(out, nbytes, args.hbm_tbs)
        pf.report(lines, out)

    for view in (L.DEBUG_VIEW_MESHLETS, L.DEBUG_VIEW_MESH_LODS, L.DEBUG_VIEW_OVERDRAW, L.DEBUG_VIEW_ALBEDO, L.DEBUG_VIEW_GTAO):
        row(NAMES[view], DebugViewContext.over(view, s.decoded, ambient_occlusion=s.ao, overdraw=overdraw), W, H, W * H * (16 + EXTRA_BYTES[view]))

    small = lambda t: t[:16, :16].contiguous()  # noqa: E731
    depth16 = ImageAttachment.depth(small(s.depth.data.view(H, W)))
    c16 = DebugViewContext(L.DEBUG_VIEW_MESHLETS, depth16, torch.zeros((16, 16, 4), dtype=torch.int16, device=dev), visbuffer_attachment=small(s.vis))
    row("Meshlets, 16 x 16", c16, 16, 16, 16 * 16 * 16)

    sh = pf.shadow_frame(s)
    pf.draw_shadow_frame(r, sh)
    torch.cuda.synchronize()
    r.prepared_frame = frame
    row("RMVSM", DebugViewContext.vsm(sh.v), W, H, W * H * 12)  # the depth and the output; the page-table words are shared by a page's pixels
    r.close()
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
