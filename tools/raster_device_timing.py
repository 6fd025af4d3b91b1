"""Time the two rasterisers of one liboxcull build (tools/, not bench.py): oxc_draw_visbuffer on pass_frames' main scene and the three
frames of vsm_draw_bench (first, steady, invalidated), each the median of --steps calls after --warmup, HIP events around the call.
Appends one JSON line to --out with --label and --commit, so that runs of two builds (--lib: another liboxcull.so, e.g. the parent
commit's built from a worktree) can be alternated from a shell loop into one file (profiles/raster_device_timing.jsonl)."""
import json

import torch

import pass_frames as pf  # first: it puts the repository root on sys.path
from oxylus_amd.renderer import RendererInstance, VsmDrawContext


def main(argv=None):
    ap = pf.common_arguments()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="result")
    ap.add_argument("--commit", default="")
    ap.add_argument("--round", type=int, default=0)
    args = pf.parse(ap, argv)
    r, dev = RendererInstance(0, lib_path=args.lib), torch.device("cuda:0")
    s = pf.main_scene(r, args.meshlets, dev)
    W, H = pf.extent(args.size)
    pf.draw_main(r, s, W, H)
    visdepth = torch.empty((H, W), dtype=torch.int64, device=dev)
    med, mn = pf.time_call(lambda: r.draw_visbuffer(s.ctx, s.pv, W, H, visdepth, clear=True), args.steps, args.warmup)
    row = {"label": args.label, "commit": args.commit, "round": args.round, "size": args.size, "steps": args.steps, "warmup": args.warmup,
           "draw_visbuffer_ms_median": med, "draw_visbuffer_ms_min": mn}
    sh = pf.shadow_frame(s)
    v, scene = sh.v, s.scene
    g = torch.Generator().manual_seed(5)
    for kind in ("first", "steady", "invalidated"):
        if kind == "invalidated":
            v.dirty_mesh_instance_indices = torch.randperm(s.M, generator=g)[:8].to(torch.int32).to(dev)
            v.mesh_instances_buffer, v.meshes_buffer = scene.mesh_instances, scene.meshes
            v.transforms_world_buffer = v.transforms_previous_buffer = scene.transforms
        d = VsmDrawContext.create(v, pf.shadow_cull(r, sh), with_commands=True)
        med, mn = pf.time_call(lambda: r.draw_physical_pages(d), args.steps, args.warmup)
        row[f"vsm_draw_{kind}_ms_median"], row[f"vsm_draw_{kind}_ms_min"] = med, mn
    r.close()
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
