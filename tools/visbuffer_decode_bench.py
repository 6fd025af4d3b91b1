"""Time oxc_decode_visbuffer (tools/, not bench.py) on the frame of tools/contact_shadows_bench.py: the configs[2] scene, given random 10:10:10
vertex normals and --materials materials, drawn by oxc_draw_visbuffer at 3840 x 2160, then the call.  Prints one JSON line: ms per call (HIP
events around the call, median and minimum of --steps after --warmup), pixels, from one extra call with the counting instantiation of the
kernel (never the timed one) the decoded / empty pixels, and from the visbuffer the distinct triangles and meshlet instances.  Also the
streaming floor at the rate given with --hbm-tbs: 8 bytes read and 20 written per pixel plus the geometry bytes touched (per distinct
triangle 3 micro indices, 3 vertex ids, 3 positions and 3 normals = 51 bytes; per distinct meshlet instance its record and its Meshlet = 24;
per distinct mesh instance the visbuffer names its MeshInstance, Mesh, MeshLOD, transform and Material = 260).  The vector-issue estimate
follows from the ISA: DESIGN.md section 15.  Per-kernel time comes from a rocprofv3 --kernel-trace --stats run of this script (k_visbuffer_decode)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--meshlets", type=int, default=10_000_000)
    ap.add_argument("--materials", type=int, default=16)
    ap.add_argument("--hbm-tbs", type=float, default=0.0, help="measured streaming rate in TB/s for the floor (0: not reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import bench
    from oxylus_amd import lib as L
    from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance, VisbufferDecodeContext
    from oxylus_amd.synth import SceneSpec, make_scene, pack_materials

    dev = torch.device("cuda:0")
    r = RendererInstance(0)
    K = bench.K_MESHLETS_PER_MESH
    M = max(1, args.meshlets // K)
    scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2), dev)
    g = torch.Generator(device=dev)
    g.manual_seed(15)
    scene.normals = torch.randint(0, 1 << 30, (scene.positions.shape[0],), generator=g, device=dev, dtype=torch.int32)
    rng = np.random.default_rng(15)
    n_mat = args.materials
    scene.materials = pack_materials(rng.random((n_mat, 4)), rng.random((n_mat, 3)) * 4.0, rng.random(n_mat), rng.random(n_mat)).to(dev)
    scene.mesh_instances[:, 2] = (torch.arange(M, device=dev) % n_mat).to(torch.int32)
    scene.bind()
    r.reserve(M, M * K)
    r.prepared_frame = PreparedFrame.create(scene, with_triangles=True)
    cam = scene.cull_camera()
    pv = [cam.projection_view[i] for i in range(16)]
    W, H = (int(v) for v in args.size.split("x"))
    ctx = CullGeometryContext(init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=cam)
    r.seed_meshlet_instances(ctx, M * K)
    r.cull_geometry(ctx)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
    depth = ImageAttachment.depth(torch.zeros((H, W), dtype=torch.float32, device=dev))
    vis = torch.zeros((H, W), dtype=torch.int32, device=dev)
    r.draw_visbuffer(ctx, pv, W, H, visdepth, clear=True, depth=depth, visbuffer=vis)
    torch.cuda.synchronize()
    del visdepth
    c = VisbufferDecodeContext.create(vis, depth, pv, M * K, scene.materials)
    times = []
    for i in range(args.warmup + args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r.decode_visbuffer(c)
        b.record()
        b.synchronize()
        if i >= args.warmup:
            times.append(a.elapsed_time(b))
    r.debug_set_tuning(L.TUNE_VISBUFFER_DECODE_STATS, 1)
    r.decode_visbuffer(c)
    st = r.debug_visbuffer_decode_stats()
    r.debug_set_tuning(L.TUNE_VISBUFFER_DECODE_STATS, 0)
    covered = vis[depth.data.view(H, W) != 0]
    triangles = int(torch.unique(covered).numel())
    named = torch.unique(covered >> 8).long()
    instances = int(named.numel())
    mesh_instances = int(torch.unique(r.prepared_frame.meshlet_instances_buffer[named, 0]).numel())
    geometry = 51 * triangles + 24 * instances + 260 * mesh_instances
    out = {"workload": "visbuffer_decode", "size": args.size, "scene_meshlets": M * K, "materials": n_mat, "pixels": W * H, "ms_median": float(np.median(times)),
           "ms_min": float(np.min(times)), **st, "distinct_triangles": triangles, "distinct_meshlet_instances": instances, "distinct_mesh_instances": mesh_instances,
           "image_bytes": 28 * W * H, "geometry_bytes": geometry}
    if args.hbm_tbs > 0:
        out["streaming_floor_ms"] = (28 * W * H + geometry) / (args.hbm_tbs * 1e12) * 1e3
    r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
