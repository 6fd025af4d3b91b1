"""Time oxc_decode_visbuffer (tools/, not bench.py) on pass_frames.decode_context: the configs[2] scene, given random 10:10:10
vertex normals and --materials materials, drawn by oxc_draw_visbuffer at 3840 x 2160, then the call.  Prints one JSON line: ms per call (HIP
events around the call, median and minimum of --steps after --warmup), pixels, from one extra call with the counting instantiation of the
kernel (never the timed one) the decoded / empty pixels, and from the visbuffer the distinct triangles and meshlet instances.  Also the
streaming floor at the rate given with --hbm-tbs: 8 bytes read and 20 written per pixel plus the geometry bytes touched (per distinct
triangle 3 micro indices, 3 vertex ids, 3 positions and 3 normals = 51 bytes; per distinct meshlet instance its record and its Meshlet = 24;
per distinct mesh instance the visbuffer names its MeshInstance, Mesh, MeshLOD, transform and Material = 260).  The vector-issue estimate
follows from the ISA: DESIGN.md section 15.  Per-kernel time comes from a rocprofv3 --kernel-trace --stats run of this script (k_visbuffer_decode)."""
import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd import lib as L


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--materials", type=int, default=16)
    args = pf.parse(ap, argv, hbm_help="measured streaming rate in TB/s for the floor (0: not reported)")

    r, dev = pf.renderer()
    s = pf.main_scene(r, args.meshlets, dev, materials=args.materials)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H, visbuffer=True)
    c = pf.decode_context(s)
    med, mn = pf.time_call(lambda: r.decode_visbuffer(c), args.steps, args.warmup)
    st = pf.counted_call(r, L.TUNE_VISBUFFER_DECODE_STATS, lambda: r.decode_visbuffer(c), r.debug_visbuffer_decode_stats)
    covered = s.vis[s.depth.data.view(H, W) != 0]
    triangles = int(torch.unique(covered).numel())
    named = torch.unique(covered >> 8).long()
    instances = int(named.numel())
    mesh_instances = int(torch.unique(r.prepared_frame.meshlet_instances_buffer[named, 0]).numel())
    geometry = 51 * triangles + 24 * instances + 260 * mesh_instances
    out = {"workload": "visbuffer_decode", "size": args.size, "scene_meshlets": s.M * s.K, "materials": args.materials, "pixels": W * H, "ms_median": med,
           "ms_min": mn, **st, "distinct_triangles": triangles, "distinct_meshlet_instances": instances, "distinct_mesh_instances": mesh_instances,
           "image_bytes": 28 * W * H, "geometry_bytes": geometry}
    pf.streaming_floor(out, 28 * W * H + geometry, args.hbm_tbs)
    r.close()
    lines = []
    pf.report(lines, out)
    return pf.write_out(args.out, lines)


if __name__ == "__main__":
    main()
