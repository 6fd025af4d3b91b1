#!/usr/bin/env python3
"""bench.py -- meshlets/s culled on MI355X (BASELINE.json metric); rank 0 prints ONE JSON line.

  python bench.py --gpus N --steps K --warmup W
  (N > 1 without a torchrun environment: bench.py starts `python -m torch.distributed.run --nproc-per-node N` itself and
   fails loudly when it cannot; under the driver's own torchrun launch it just joins the world.)

Default workload = BASELINE.json configs[2], the full north-star path on one GPU: 10M meshlet instances (10 000 mesh
instances x 1000 meshlets, 64 vertices / 64 triangles each, unique geometry ~10 GB) + a 4096^2 HiZ (13 mips) built from a
synthetic 8192^2 depth image.  One FRAME is the reference's sequence (RendererInstance.cpp:842-884 for a given depth and a
given prior-visibility mask):
    oxc_generate_hiz -> oxc_cull_geometry(TestAll)  [early: cull_meshlets_hiz + cull_triangles + compaction]
                     -> oxc_cull_geometry(TestAll | LatePass)  [late]
A frame takes well under a millisecond, so a STEP is `inner_reps` frames (stated in config) -- 20 steps are >= 0.5 s of GPU
work and `value` is not launch latency.  All inputs are generated in HBM; the ABI takes device pointers (no PCIe in the loop).

N > 1 = configs[3]: ONE scene of N x 12.5M meshlets ("100M sharded 8 ways"; weak scaling) whose mesh instances are dealt to the ranks
in interleaved blocks of 64 instances (SURVEY 8e's mitigation; --shard-block 0: contiguous ranges, which are depth slabs of this scene and
skewed -- a short nested run times that form too, "assignment_ab"; --independent-scenes: rounds 1-4's one scene per rank), shard-local ids and outputs.  Rank 0 builds the pyramid and broadcasts its top (levels >= 2, 5.6 MB; `--hiz-exchange whole`:
all 89.5 MB) over RCCL/xGMI, the other ranks build levels 0-1 from their copy of the depth image; the per-rank counters
{emitted, early, late, index_count} are all-gathered every frame.  The HiZ a frame culls against is the PRIOR frame's, so its
build + broadcast run one frame ahead on a second stream (double-buffered pyramid) and overlap the cull.

The configs[1] result (1M meshlets, frustum + cone only) rides along as the nested object "configs1" (batched x16 on three
streams, AND one call per frame on one stream).  `--workload config2` prints it as the main line instead; `--workload
config1` is the reference's CPU-runnable case (BASELINE configs[0], host cores only); bounds | loop | vsm | config5 live in
tools/bench_aux.py.

Extra objects: "roofline" (dominant kernel: algorithmic bytes of SURVEY 8d / HIP-event kernel time, averaged over >= 50
launches, vs the 8 TB/s HBM peak; every kernel in "kernels", the whole frame in "stage_frac") and "cpu_baseline" (the scalar
C checker, oracle/, running the same sequence over a bounded prefix of the same arrays on the host; a reported baseline,
not the target).

A plain run does only what the headline needs: set-up, warm-up, the timed steps, the outputs (--dump-outputs) and the result
line.  Everything else -- the checked frame and bit_match, the CPU baseline, the scheduling / exchange / assignment variants, the
kernel profile and rooflines, and the nested runs (tris124, configs1, configs4, real_geometry, configs0) -- runs with --full.

  --dump-outputs DIR: after the timed steps, what the last frame computed as DIR/<name>.npy (float64, float32 for the pyramid,
  under 64 MB in all; rank 0's shard when N > 1).  Lists are sorted, as the checks compare them; a list longer than
  DUMP_SAMPLE entries is cut to a fixed seeded sample of positions, so two builds with the same arguments compare entry by entry.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from oxylus_amd import lib as L  # noqa: E402
from oxylus_amd.renderer import CullGeometryContext, ImageAttachment, PreparedFrame, RendererInstance  # noqa: E402
from oxylus_amd.synth import SceneSpec, make_depth, make_scene  # noqa: E402
from bench_line import emit  # noqa: E402  (tools/bench_line.py: full record -> gpurun_out/bench_full.json, compact headline -> stdout)

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
PROFILE_ROUNDS = ("r06", "r05")  # committed rocprofv3 summaries under profiles/, newest first: the second clock and the PMC traffic of the line
K_MESHLETS_PER_MESH = 1000


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="config3", choices=["config3", "config2", "config1", "config5", "bounds", "loop", "vsm"])
    ap.add_argument("--inner-reps", type=int, default=0, help="frames per step (default: 48 for config3, 9600 for config2)")
    ap.add_argument("--tris", type=int, default=64, help="config3: triangles per meshlet; > 64 uses an index extension of SURVEY A.7, see --index-form")
    ap.add_argument("--index-form", default="pairs", choices=["pairs", "wide"],
                    help="config3 with --tris > 64: 'pairs' (default; wide_triangle_index = 2: every index is {u32 id, u32 corner}, no id limit -- BASELINE's 10 M x 124 "
                         "and 12.5 M-meshlet shards) or 'wide' (wide_triangle_index = 1: (id << 9) | corner, at most 2^23 ids, so 8 M meshlets)")
    ap.add_argument("--small-triangle-cull", action="store_true", help="config3: turn the opt-in small-triangle cull on (default off = reference behaviour)")
    ap.add_argument("--views", type=int, default=16, help="config5: number of cascade views per step")
    ap.add_argument("--meshlets", type=int, default=0, help="override meshlets per GPU (default 10M; 12.5M per rank when N > 1; 1M for config2)")
    ap.add_argument("--copies", type=int, default=0, help="config2: independent scene copies rotated through (default: >= 1.1 GB)")
    ap.add_argument("--streams", type=int, default=3, help="config2: independent batches in flight (contexts on their own HIP streams)")
    ap.add_argument("--batch", type=int, default=16, help="config2 / config5: frames (views) per oxc_cull_geometry_batch call (max 16)")
    ap.add_argument("--implicit-lists", action="store_true", help="config5: leave the per-view MeshletInstance lists implicit ({first, count} runs per mesh instance, include/oxcull.h: "
                                                                   "implicit_meshlet_instances) on the main line; by default the records are written as the reference's cull_meshes writes them "
                                                                   "(reference-equivalent output) and the implicit form is timed as a variant")
    ap.add_argument("--no-configs1", action="store_true", help="config3: skip the nested configs[1] measurement (1M meshlets, frustum + cone)")
    ap.add_argument("--no-configs4", action="store_true", help="config3: skip the nested configs[4] measurement (10M meshlets x 16 views)")
    ap.add_argument("--no-configs0", action="store_true", help="config3: skip the nested configs[0] measurement (1k entities, host only, ~2 s)")
    ap.add_argument("--no-real-geometry", action="store_true", help="config3: skip the nested run of the same frame over instanced real meshes (clusteriser-built)")
    ap.add_argument("--async-triangles", action="store_true",
                    help="config3: time the main line with async_triangles = 1 (triangle stages on the context's own stream, frames pipeline); the default line is in "
                         "order on one stream and carries the pipelined figure as the nested object \"async_triangles\"")
    ap.add_argument("--no-share-pass-tests", action="store_true",
                    help="config3: every call runs its own frustum + cone tests; by default the two calls of a frame set share_pass_tests (include/oxcull.h): the late "
                         "call reuses the early call's results -- same outputs; the other form is timed as a variant in scheduling_ab")
    ap.add_argument("--unordered-output", type=int, default=1, choices=[0, 1, 2],
                    help="config3: unordered_output of include/oxcull.h on the main line.  Default 1 -- SURVEY 7: \"benchmark the unordered one, parity-test the ordered one "
                         "(and the unordered one after sort)\": the triangle stage is one launch that allocates its output slots with an atomic_add, like the reference; "
                         "0 = ascending lists (the library's default), 2 = appending HiZ meshlet tests too.  The other forms are timed as scheduling_ab variants; "
                         "bit_match compares unordered lists sorted")
    ap.add_argument("--no-tris124", action="store_true", help="config3: skip the nested run with BASELINE's stated meshlet shape (64 verts / 124 tris, pair index form, 10 M meshlets)")
    ap.add_argument("--no-scheduling-ab", action="store_true", help="config3: skip the short timed runs of the other schedulings (profiling runs: their concurrent kernels would "
                                                                    "be averaged into the per-kernel durations of a kernel trace)")
    ap.add_argument("--no-exchange-ab", action="store_true", help="N > 1: skip the short timed run with the other --hiz-exchange form")
    ap.add_argument("--no-native-comm-ab", action="store_true", help="N > 1: skip the short timed run with the exchanges through the OTHER RCCL path (the C ABI's own entry points "
                                                                     "when the main line uses torch.distributed, and the reverse)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-overlap", action="store_true", help="N > 1: build + broadcast the pyramid on the cull stream instead of one frame ahead on a second stream")
    ap.add_argument("--hiz-exchange", default="top", choices=["whole", "top"],
                    help="N > 1: 'top' (default, the north star's wording: \"a broadcast of the top HiZ mips\") = only levels >= --hiz-top-level travel "
                         "(5.6 MB at level 2) and every rank builds the lower levels from its own copy of the prior-frame depth image; 'whole' = rank 0 "
                         "broadcasts every level (89.5 MB; assumes nothing about the other ranks).  Same pyramid bytes on every rank either way.")
    ap.add_argument("--hiz-top-level", type=int, default=2)
    ap.add_argument("--independent-scenes", action="store_true", help="N > 1: every rank generates a scene of its own (rounds 1-4's form: no visibility skew between ranks by construction) "
                                                                      "instead of culling its shard of ONE spatially coherent scene (the default since round 5: every rank's instances are placed where "
                                                                      "the whole scene's grid puts their global indices; per_rank_visible beside per_rank_ms_per_frame)")
    ap.add_argument("--one-scene", action="store_true", help="(the default for N > 1 since round 5; kept for older command lines)")
    ap.add_argument("--shard-block", type=int, default=64, help="N > 1, one scene: B > 0 = interleaved blocks of B mesh instances dealt round robin (default 64: SURVEY 8e's 64 instances x 1000 "
                                                                 "meshlets = 64k meshlets), 0 = contiguous instance ranges (depth slabs of the synthetic scene: skewed)")
    ap.add_argument("--no-assignment-ab", action="store_true", help="N > 1, one scene: skip the nested short run with the OTHER assignment (contiguous ranges <-> interleaved blocks)")
    ap.add_argument("--native-comm", action="store_true",
                    help="N > 1: run the two exchanges (counter all-gather, HiZ broadcast) through the C ABI's RCCL entry points "
                         "(oxc_exchange_counts / oxc_broadcast_hiz) instead of torch.distributed; the rendezvous stays torch.distributed")
    ap.add_argument("--cpu-seconds", type=float, default=6.0)
    ap.add_argument("--cpu-prefix", type=int, default=1000, help="config3 cpu_baseline / bit_match sample: the first this-many mesh instances")
    ap.add_argument("--entities", type=int, default=1000, help="config1: entity count")
    ap.add_argument("--full", action="store_true", help="config3: also run the checks, CPU baseline, variants, kernel profile, rooflines and nested runs (a plain run "
                                                        "times the main line only; the --no-* options above trim a --full run)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="config3: write the last timed frame's outputs to DIR/<name>.npy (see the module docstring)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------------
# process / world setup
# ------------------------------------------------------------------------------------------------------------------
def respawn_under_torchrun(args):
    """`bench.py --gpus N` outside a torchrun environment: become the launcher."""
    import socket
    import subprocess

    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus and not os.environ.get("OXC_BENCH_DEBUG_BACKEND"):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but only {n_dev} GPU(s) are visible; refusing to report a {n_dev}-GPU number as {args.gpus}")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    raise SystemExit(rc)


class Env:
    pass


def setup(args) -> Env:
    e = Env()
    e.rank = int(os.environ.get("RANK", "0"))
    e.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    e.world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != e.world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={e.world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no GPU visible (the cull path has no CPU fallback; --workload config1 is the CPU-only case)")
    # OXC_BENCH_DEBUG_BACKEND=gloo: exercise the N > 1 control flow (sharding, double-buffered pyramid, events, exchanges) with all ranks on
    # whatever GPUs exist -- a development aid for one-GPU boxes; the line it prints says so and is not a measurement
    e.debug_backend = os.environ.get("OXC_BENCH_DEBUG_BACKEND", "")
    if e.debug_backend:
        e.local_rank = e.local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(e.local_rank)
    e.dev = torch.device("cuda", e.local_rank)
    e.dist = None
    if e.world > 1:
        import torch.distributed as dist

        if e.debug_backend:
            dist.init_process_group(e.debug_backend)
        else:
            dist.init_process_group("nccl", device_id=e.dev)  # RCCL over xGMI
        e.dist = dist
    e.r = RendererInstance(e.local_rank)
    e.stream = torch.cuda.Stream(device=e.dev)
    # The product's own RCCL entry points (oxc_comm_*, oxc_exchange_counts, oxc_broadcast_hiz[_levels]): their communicators are set up at every
    # N > 1 run on real GPUs -- the main line takes them with --native-comm, and otherwise a short nested run (native_comm_ab) does, so that
    # the first multi-GPU run exercises them either way.  The rendezvous (the 128-byte id) travels through torch.distributed.
    e.native_comm = bool(args.native_comm and e.dist is not None)
    # native_ready: True = set up, False = cannot be, None = not tried yet -- without --native-comm the set-up waits until the main line has been
    # measured and runs under native_comm_ab's watchdog (a rendezvous that hangs must not cost the run its headline)
    e.native_ready, e.native_error = None, None
    if e.dist is not None and e.debug_backend and not os.environ.get("OXC_BENCH_DEBUG_TRY_NATIVE"):
        # (OXC_BENCH_DEBUG_TRY_NATIVE=1: try anyway -- two ranks on one GPU make ncclCommInitRank fail or hang, which is how the error path and the
        #  watchdog of native_comm_ab are exercised on a one-GPU box)
        e.native_ready, e.native_error = False, f"debug backend {e.debug_backend}: every rank is on the same GPU, RCCL needs one device per rank"
    elif e.dist is not None and e.native_comm:
        e.native_ready, e.native_error = native_comm_init(e, e.r)
        if not e.native_ready:
            raise SystemExit(f"bench.py: --native-comm but the communicator could not be set up: {e.native_error}")
    return e


def native_comm_init(e, renderer):
    """oxc_comm_unique_id on rank 0 -> every rank -> oxc_comm_init; (ok on EVERY rank, first error)."""
    err = None
    try:
        box = [renderer.comm_unique_id() if e.rank == 0 else None]
    except Exception as ex:  # noqa: BLE001  (librccl could not be loaded, ...)
        box, err = [None], f"rank 0: {ex}"
    e.dist.broadcast_object_list(box, src=0)
    if box[0] is not None:
        try:
            renderer.comm_init(box[0], e.rank, e.world)
        except Exception as ex:  # noqa: BLE001
            err = f"rank {e.rank}: {ex}"
    else:
        err = err or "rank 0 could not create the id"
    errs = [None] * e.world
    e.dist.all_gather_object(errs, err)
    bad = [x for x in errs if x]
    return (not bad), (bad[0][:200] if bad else None)


def barrier(e):
    if e.dist is not None:
        e.dist.barrier()


PER_RANK_SECONDS = []  # of the last timed_steps(): every rank's own wall time (rank order)


def max_over_ranks(e, seconds: float) -> float:
    PER_RANK_SECONDS[:] = [seconds]
    if e.dist is None:
        return seconds
    t = torch.tensor([seconds], dtype=torch.float64, device=e.dev)
    if e.debug_backend:
        allt = [torch.zeros(1, dtype=torch.float64) for _ in range(e.world)]
        e.dist.all_gather(allt, t.cpu())
    else:
        allt = [torch.zeros(1, dtype=torch.float64, device=e.dev) for _ in range(e.world)]
        e.dist.all_gather(allt, t)
    PER_RANK_SECONDS[:] = [float(x.item()) for x in allt]
    return max(PER_RANK_SECONDS)


def usable_cores() -> int:
    """Host threads this process may actually run at once: the affinity mask, cut down by a cgroup CPU quota when the
    container has one (a box can show 256 CPUs in the mask and still be limited to a few cores' worth of time)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    quota = None
    try:  # cgroup v2: "<quota|max> <period>"
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = int(q) / int(period)
    except (OSError, ValueError):
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and period > 0:
                quota = q / period
        except (OSError, ValueError):
            pass
    if quota is not None:
        cores = max(1, min(cores, int(quota + 0.999)))
    return cores


def ramp_clocks(e, seconds=0.75):
    """Not steps: a fresh box idles at low DPM clocks; the first ~0.5 s of work runs 2-3x slower and would be measured
    instead of the kernels."""
    ramp = torch.empty(256 << 20, dtype=torch.uint8, device=e.dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        with torch.cuda.stream(e.stream):
            for _ in range(20):
                e.r.stream_read_probe(ramp, e.stream)
        torch.cuda.synchronize()
    del ramp


def stream_read_ceiling(e) -> float:
    """Measured streaming-read ceiling of this GPU (plain 16 B/lane loads over 2 GiB), GB/s."""
    probe = torch.empty(2 << 30, dtype=torch.uint8, device=e.dev)
    probe.random_(0, 255)
    with torch.cuda.stream(e.stream):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # the memory clock needs sustained streaming before the rate settles
            for _ in range(30):
                e.r.stream_read_probe(probe, e.stream)
            e.stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(e.stream)
        for _ in range(30):
            e.r.stream_read_probe(probe, e.stream)
        e1.record(e.stream)
    torch.cuda.synchronize()
    gbps = 30 * probe.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9
    del probe
    return gbps


def timed_steps(e, run_step, steps: int, warmup: int) -> float:
    """W untimed steps, then EXACTLY `steps` steps between barrier + synchronize pairs; max over ranks, seconds."""
    with torch.cuda.stream(e.stream):
        for i in range(warmup):
            run_step(i)
    torch.cuda.synchronize()
    barrier(e)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(e.stream):
        for i in range(steps):
            run_step(i)
    torch.cuda.synchronize()
    barrier(e)
    return max_over_ranks(e, time.perf_counter() - t0)


def profile_kernels(e, renderers, run, n: int) -> dict:
    """Instrumented pass: every kernel of `n` calls of run(i) bracketed by a HIP-event pair on the stream it runs on
    (oxc_profile_begin/end).  Raw event-to-event time per launch (what rocprofv3's kernel duration also spans: dispatch +
    run); the cost of an empty pair is reported, not subtracted."""
    for rr in renderers:
        rr.profile_begin()
    with torch.cuda.stream(e.stream):
        for i in range(n):
            run(i)
    acc, empty = {}, 0.0
    for rr in renderers:
        p = rr.profile_end()
        empty = max(empty, p["empty_pair_ms"])
        for name, k in p["kernels"].items():
            a = acc.setdefault(name, {"launches": 0, "total_ms": 0.0})
            a["launches"] += k["launches"]
            a["total_ms"] += k["total_ms"]
    out = {name: {"launches": k["launches"], "avg_us": k["total_ms"] / k["launches"] * 1e3} for name, k in acc.items()}
    out["_empty_event_pair_us"] = round(empty * 1e3, 3)
    return out


def kernel_source_sha16() -> str:
    """sha256 over the device sources of the cull path (oxcull_kernels.hip + the three headers it is made of): what
    tools/summarize_profiles.py stamps into a committed profile.  The other translation units (rasteriser, terrain, bounds, HPB
    producers) do not contain a kernel of the frames this file times."""
    import hashlib

    h = hashlib.sha256()
    for f in ("oxcull_kernels.hip", "oxcull_kernels.hpp", "oxcull_device.hpp", "oxcull_types.hpp"):
        h.update(open(os.path.join(ROOT, "oxylus_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def committed_profile(names):
    for n in names:
        try:
            with open(os.path.join(ROOT, "profiles", n)) as f:
                return n, json.load(f)
        except (OSError, ValueError):
            continue
    return None, None


def pmc_traffic(profile_names, match) -> tuple:
    """HBM bytes per launch from a committed rocprofv3 --pmc summary (FETCH_SIZE x 1024 x 2 + WRITE_SIZE x 1024, separate
    passes, as MI355X_MICROARCH.md prescribes).  PMC counters cannot be read from inside this process, so the figure belongs to the
    build the profile was taken from: the third value says whether that is the device code of this tree (kernel_source_sha16)."""
    name, pm = committed_profile([profile_names] if isinstance(profile_names, str) else profile_names)
    if pm is None:
        return None, None, None
    vals = [cs["hbm_read_bytes_corrected"] + cs.get("hbm_write_bytes", 0) for k, cs in pm.get("pmc", {}).items() if match(k) and "hbm_read_bytes_corrected" in cs]
    if not vals:
        return None, None, None
    same = pm.get("kernel_source_sha16") == kernel_source_sha16() if pm.get("kernel_source_sha16") else None
    return round(sum(vals) / len(vals)), f"profiles/{name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, per launch)", same


def pmc_read_written(profile_names) -> dict:
    """{kernel: (HBM bytes read, written) per launch} of the committed --pmc summary (FETCH_SIZE x 1024 x 2 / WRITE_SIZE x 1024)."""
    _, pm = committed_profile([profile_names] if isinstance(profile_names, str) else profile_names)
    return {k: (cs["hbm_read_bytes_corrected"], cs.get("hbm_write_bytes", 0)) for k, cs in (pm or {}).get("pmc", {}).items() if "hbm_read_bytes_corrected" in cs}


def rocprof_kernel_us(profile_names) -> dict:
    """Average kernel durations of the committed rocprofv3 --kernel-trace --stats summary: the second clock beside the HIP-event times."""
    _, pm = committed_profile([profile_names] if isinstance(profile_names, str) else profile_names)
    return {r["kernel"]: r["avg_us"] for r in (pm or {}).get("kernel_trace_stats", [])}


# ------------------------------------------------------------------------------------------------------------------
# configs[2] (N = 1) / configs[3] (N > 1): HiZ build + two-pass occlusion cull + triangle cull + compaction
# ------------------------------------------------------------------------------------------------------------------
def hiz_algorithmic_bytes(w: int, h: int, levels: int) -> int:
    """one depth texel read per mip-0 texel, every level written, the 64x64-tile level read again by the tail."""
    written = sum(max(1, w >> k) * max(1, h >> k) for k in range(levels)) * 4
    return 4 * w * h + written + (4 * max(1, w >> 6) * max(1, h >> 6) if levels > 7 else 0)


DUMP_SAMPLE = 1 << 20  # entries kept of a longer list: worst case (pairs, every list sampled) 3 x 8.4 + 16.8 MB + the 4.2 MB pyramid sample
DUMP_LIMIT = 64 << 20


def dump_outputs(out_dir, counters, visible, ne, index_words, pairs, mask, hiz_data):
    """--dump-outputs: the outputs of the last frame as DIR/<name>.npy.  visible = early list [0, ne) then late list; index_words = the
    late call's index list (each call's list starts at 0); counters = (total, early, late, late index_count).  Lists are sorted (the
    unordered forms allocate slots by atomics), then cut to a fixed seeded sample of positions when longer than DUMP_SAMPLE."""
    import numpy as np

    def sample(t, seed):
        if t.shape[0] <= DUMP_SAMPLE:
            return t
        pos = torch.randint(0, t.shape[0], (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(seed)).sort()[0]
        return t[pos.to(t.device)]

    keys = index_words.to(torch.int64) & 0xFFFFFFFF
    if pairs:  # {u32 id, u32 corner}: sorted by (id, corner), written as two columns (a packed key would pass 2^53)
        keys = (keys.view(-1, 2)[:, 0] << 32) | keys.view(-1, 2)[:, 1]
    keys = sample(torch.sort(keys)[0], 3)
    arrays = {
        "counters": torch.tensor(counters, dtype=torch.float64),
        "visible_early": sample(torch.sort(visible[:ne])[0], 1).double(),
        "visible_late": sample(torch.sort(visible[ne:])[0], 2).double(),
        "indices_late": (torch.stack([keys >> 32, keys & 0xFFFFFFFF], dim=1) if pairs else keys).double(),
        "visibility_mask": sample(mask, 4).double(),
        "hiz_sample": sample(hiz_data, 5).float(),
    }
    arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes"
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def bench_config3(args, e):
    r, dev, stream, rank, world, dist = e.r, e.dev, e.stream, e.rank, e.world, e.dist
    lib, ctxp, sp = r._lib, r._ctx, C.c_void_p(stream.cuda_stream)
    K = K_MESHLETS_PER_MESH
    wide = args.tris > 64
    pairs = wide and args.index_form == "pairs"  # {u32 id, u32 corner} pairs beyond 2^23 ids
    W = 2 if pairs else 1                        # words per index
    wti = 2 if pairs else (1 if wide else 0)     # wide_triangle_index of include/oxcull.h
    n_meshlets = args.meshlets or (10_000_000 if world == 1 else 12_500_000)
    if wide and not pairs:
        n_meshlets = min(n_meshlets, 8_000_000)  # 23-bit instance id of the wide index
    M = max(1, n_meshlets // K)
    n_meshlets = M * K
    inner = args.inner_reps or 48
    HW = 4096

    def check(st):
        if st != L.OXC_OK:
            raise RuntimeError(lib.oxc_last_error(ctxp).decode())

    shard_desc = None
    world_meshlets = n_meshlets * world  # meshlets all ranks cull per frame
    with torch.cuda.stream(stream):
        if world > 1 and not args.independent_scenes:
            # ONE scene of M x world instances, sharded: contiguous ranges of the instance index (= slabs of the scene's grid, far to near) or
            # interleaved blocks (oxylus_amd/shard.py shard_ranges); a rank generates only its own instances, placed by their global indices
            from oxylus_amd.shard import shard_ranges

            M_total = M * world
            mine = shard_ranges(M_total, world, args.shard_block)[rank]
            mine = [mine] if args.shard_block <= 0 else mine
            gids = torch.cat([torch.arange(a, b, dtype=torch.int64) for a, b in mine]) if mine else torch.zeros(0, dtype=torch.int64)
            assert gids.numel() > 0, "a rank without instances: fewer blocks than ranks"
            M = int(gids.numel())
            n_meshlets = M * K
            scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2 + rank, tris_per_meshlet=args.tris), dev,
                               global_ids=gids, global_total=M_total)
            world_meshlets = M_total * K
            shard_desc = {"one_scene": True, "scene_mesh_instances": M_total, "shard_block_instances": args.shard_block,
                          "assignment": "contiguous instance ranges" if args.shard_block <= 0 else f"interleaved blocks of {args.shard_block} instances", "this_rank_ranges": len(mine)}
        else:
            scene = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=True, seed=0x0A1DE5 + 2 + rank, tris_per_meshlet=args.tris), dev)
        r.reserve(M, n_meshlets)
        frame = PreparedFrame.create(scene, with_triangles=True, max_tris=128 if wide else 64, index_words=W)
        depth = ImageAttachment.depth(make_depth(2 * HW, 2 * HW, 64, seed=3, device=dev))  # the same image on every rank
        hiz = [ImageAttachment.hiz(HW, HW, dev) for _ in range(2)]  # double-buffered: the pyramid of the next frame can be built beside the cull of this one
        ctx = CullGeometryContext(use_hiz=True, init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=scene.cull_camera(), hiz_attachment=hiz[0],
                                  stages=L.STAGE_ALL, wide_triangle_index=wti, small_triangle_cull=args.small_triangle_cull)
        r.prepared_frame = frame
        r.seed_meshlet_instances(ctx, n_meshlets)
        # random prior-visibility mask, p = 0.3; every frame starts from it again
        g = torch.Generator(device=dev).manual_seed(5 + rank)
        words = frame.meshlet_instance_visibility_mask_buffer.numel()
        bits = (torch.rand((words, 32), generator=g, device=dev) < 0.3).to(torch.int64)
        mask0 = (bits << torch.arange(32, device=dev)).sum(1).to(torch.int32)
        del bits
        mask = frame.meshlet_instance_visibility_mask_buffer
    torch.cuda.synchronize()
    cframe = frame.c()
    pf = C.byref(cframe)
    cctx = [ctx.c()]
    for hz in hiz[1:]:  # one pre-marshalled context per pyramid buffer (same sequence buffers)
        c2 = L.CullGeometryContext()
        C.memmove(C.byref(c2), C.byref(cctx[0]), C.sizeof(L.CullGeometryContext))
        c2.hiz_attachment = hz.c()
        cctx.append(c2)
    mgs, mgs_low = [], []
    xmode = {"top": world > 1 and args.hiz_exchange == "top"}  # (mutable: the A/B run at the end times the other form)
    k_top = max(1, min(args.hiz_top_level, hiz[0].levels - 1))
    for hz in hiz:
        mg = L.MainGeometryContext()
        mg.struct_size = C.sizeof(L.MainGeometryContext)
        mg.depth_attachment, mg.hiz_attachment = depth.c(), hz.c()
        mgs.append(mg)
        lo = L.MainGeometryContext()  # the same image with only the levels below k_top: what a non-root rank builds itself
        lo.struct_size = C.sizeof(L.MainGeometryContext)
        lo.depth_attachment, lo.hiz_attachment = depth.c(), hz.c()
        lo.hiz_attachment.levels = k_top
        mgs_low.append(lo)
    hiz_bytes = hiz[0].data.numel() * 4
    wire_bytes = lambda top_: hiz_bytes - (hiz[0].level_offset[k_top] if top_ else 0)  # noqa: E731
    hiz_wire_bytes = wire_bytes(xmode["top"])

    # ---- multi-GPU plumbing: second context + stream for the pyramid producer, events, counter all-gather ----
    # "one frame ahead": the pyramid a frame culls against is given (the prior frame's), so its build (+ broadcast) can run on a second
    # stream beside the previous frame's cull.  Default for N > 1 (the exchange must not sit in the frame); at N = 1 the main line keeps
    # the strict in-order frame on one stream and the pipelined form is timed as a variant (scheduling_ab).
    use_overlap = [world > 1 and not args.no_overlap]
    overlap = use_overlap[0]
    r_hiz = RendererInstance(e.local_rank)  # its own context: the producer runs beside the cull (one context = one ordered queue)
    native_ready, native_error = e.native_ready, e.native_error
    if native_ready:  # (--native-comm) ... and its own communicator: the broadcast must not queue behind the cull context's calls
        native_ready, native_error = native_comm_init(e, r_hiz)
    use_native = [bool(e.native_comm and native_ready)]  # (mutable: native_comm_ab times the other path)
    comm_stream = torch.cuda.Stream(device=dev)
    ev_ready = [torch.cuda.Event() for _ in hiz]
    ev_free = [torch.cuda.Event() for _ in hiz]
    have_free = [False for _ in hiz]
    primed = [False]
    if world > 1:
        my_counts = torch.zeros(4, dtype=torch.int32, device=dev)
        gathered = torch.zeros(world * 4, dtype=torch.int32, device=dev)
    csp = C.c_void_p(comm_stream.cuda_stream)

    def produce_hiz(b, ahead):
        """Rank 0 builds pyramid buffer b from the depth image; everybody receives it (RCCL broadcast over xGMI).  ahead: on the second
        stream with the producer's own context; otherwise in order on the cull stream with the cull context."""
        top = xmode["top"]
        rr, st_, sp_ = (r_hiz, comm_stream, csp) if ahead else (r, stream, sp)
        if rank == 0 or top:  # 'top': the other ranks build levels < k_top from their own copy of the depth image
            st = rr._lib.oxc_generate_hiz(rr._ctx, C.byref(mgs[b] if rank == 0 else mgs_low[b]), sp_)
            if st != L.OXC_OK:
                raise RuntimeError(rr._lib.oxc_last_error(rr._ctx).decode())
        if dist is not None:
            if use_native[0]:
                (r_hiz if ahead else r).broadcast_hiz(hiz[b], 0, st_, first_level=k_top if top else 0)
            else:
                with torch.cuda.stream(st_):
                    dist.broadcast(hiz[b].data[hiz[b].level_offset[k_top] // 4:] if top else hiz[b].data, src=0)

    def gather_counts(c):
        # {emitted, early, late, index_count} of this rank's last call -> every rank (north star's all-gather); packed on the
        # device out of the call's counter slot, no host round trip
        check(lib.oxc_pack_counters(ctxp, C.byref(c), C.c_void_p(my_counts.data_ptr()), sp))
        if use_native[0]:
            check(lib.oxc_exchange_counts(ctxp, C.c_void_p(my_counts.data_ptr()), C.c_void_p(gathered.data_ptr()), sp))
        elif e.debug_backend:  # gloo has no device all-gather: stage through the host (debug aid only)
            host = torch.zeros(world * 4, dtype=torch.int32)
            stream.synchronize()
            dist.all_gather_into_tensor(host, my_counts.cpu())
            gathered.copy_(host)
        else:
            dist.all_gather_into_tensor(gathered, my_counts)

    frame_no = [0]
    use_async = [bool(args.async_triangles)]  # async_triangles (include/oxcull.h): triangle stages on the context's own stream, frames pipeline
    # share_pass_tests (include/oxcull.h): both calls of a frame have the same camera, transforms and list (RendererInstance.cpp:842-884), so the
    # late call takes the frustum + cone results from the early one
    use_share = [not args.no_share_pass_tests]
    use_unord = [int(args.unordered_output)]  # unordered_output (include/oxcull.h): the reference's atomic slot allocation instead of the ordered emit

    def run_frame(record=None):
        f = frame_no[0]
        frame_no[0] += 1
        b = f % len(hiz)
        mask.copy_(mask0, non_blocking=True)  # restore the synthetic prior-visibility mask (1.25 MB copy)
        if use_overlap[0]:
            if not primed[0]:  # entering the pipelined form: this frame's own pyramid first
                comm_stream.wait_stream(stream)
                produce_hiz(b, True)
                ev_ready[b].record(comm_stream)
                primed[0] = True
            # next frame's pyramid: produced now, on the side stream, into the other buffer (free once frame f-1 has culled)
            nb = (f + 1) % len(hiz)
            if have_free[nb]:
                comm_stream.wait_event(ev_free[nb])
            produce_hiz(nb, True)
            ev_ready[nb].record(comm_stream)
            stream.wait_event(ev_ready[b])
        else:
            if primed[0]:  # leaving the pipelined form: nothing of the producer may still be in flight
                stream.wait_stream(comm_stream)
                primed[0] = False
            produce_hiz(b, False)
        c = cctx[b]
        c.async_triangles = int(use_async[0])
        c.share_pass_tests = int(use_share[0])
        c.unordered_output = use_unord[0]
        c.cull_flags = L.CULL_TEST_ALL
        check(lib.oxc_cull_geometry(ctxp, pf, C.byref(c), sp))
        if record is not None:
            record("early", c)
        c.cull_flags = L.CULL_TEST_ALL | L.CULL_LATE_PASS
        check(lib.oxc_cull_geometry(ctxp, pf, C.byref(c), sp))
        if record is not None:
            record("late", c)
        if use_overlap[0]:
            ev_free[b].record(stream)
            have_free[b] = True
        if world > 1:
            gather_counts(c)

    def run_step(_i):
        for _ in range(inner):
            run_frame()

    # ---- one checked frame: counters + parity of what is being timed against the CPU checker (rank 0) ----
    snap = {}

    def record(tag, c):
        torch.cuda.synchronize()
        out = L.Counters()
        check(lib.oxc_read_counters(ctxp, C.byref(c), C.byref(out), sp))
        first = out.early_visible_meshlet_instances if tag == "late" else 0
        snap[tag] = {"emitted": out.cull_triangles_cmd_x, "index_count": out.draw_index_count, "first": first,
                     "early": out.early_visible_meshlet_instances, "late": out.late_visible_meshlet_instances, "total": out.total_visible_meshlet_instances}
        if rank == 0:
            lim = min(args.cpu_prefix, M) * K  # the checker's sample: ids below `lim` (ascending lists: a prefix of each list)
            vis = frame.visible_meshlet_instances_indices_buffer[first:first + out.cull_triangles_cmd_x]
            shift = 32 if pairs else (9 if wide else 8)

            def keys(t):  # an index list as ascending-comparable int64 keys: the packed u32, or (id << 32) | corner of a pair
                if pairs:
                    p2 = t.view(-1, 2).to(torch.int64) & 0xFFFFFFFF
                    return (p2[:, 0] << 32) | p2[:, 1]
                return t.to(torch.int64) & 0xFFFFFFFF

            def unkeys(k):  # ... and back to the words of the list
                if pairs:
                    return torch.stack([(k >> 32), k & 0xFFFFFFFF], dim=1).to(torch.int32).reshape(-1)
                return k.to(torch.int32)

            if use_unord[0]:  # an unordered list is compared SORTED (the ordered form's lists ascend)
                vis = torch.sort(vis)[0]
                allidx = torch.sort(keys(frame.reordered_indices_buffer[:out.draw_index_count * W]))[0]
                nv = int(torch.searchsorted(vis, torch.tensor([lim], dtype=torch.int32, device=dev)).item())
                ni = int(torch.searchsorted(allidx, torch.tensor([lim << shift], dtype=torch.int64, device=dev)).item())
                snap[tag]["visible_prefix"] = vis[:nv].cpu()
                snap[tag]["indices_prefix"] = unkeys(allidx[:ni]).cpu()
                del allidx
            else:
                nv = int(torch.searchsorted(vis, torch.tensor([lim], dtype=torch.int32, device=dev)).item())
                # packed (id << 8 | corner) values are u32: search an upper-bounded head of the list as int64
                head = keys(frame.reordered_indices_buffer[:min(out.draw_index_count, nv * (384 if wide else 192)) * W])
                ni = int(torch.searchsorted(head, torch.tensor([lim << shift], dtype=torch.int64, device=dev)).item())
                snap[tag]["visible_prefix"] = vis[:nv].cpu()
                snap[tag]["indices_prefix"] = frame.reordered_indices_buffer[:ni * W].cpu()

    if args.full:
        with torch.cuda.stream(stream):
            run_frame(record)
        torch.cuda.synchronize()
        mask_after = mask[: (min(args.cpu_prefix, M) * K + 31) // 32].cpu() if rank == 0 else None
        counts = {"total": snap["late"]["total"], "early": snap["late"]["early"], "late": snap["late"]["late"],
                  "early_index_count": snap["early"]["index_count"], "late_index_count": snap["late"]["index_count"]}
        v_early, v_late = counts["early"], counts["late"]
        t_early, t_late = counts["early_index_count"] // 3, counts["late_index_count"] // 3

    def outputs_checksum():
        """Every output of the last frame folded into a few integers (device-side sums): what a scheduling variant must reproduce.
        Lists written with unordered_output are sorted first (early and late list each; the ordered form's lists ascend)."""
        torch.cuda.synchronize()
        out = L.Counters()
        check(lib.oxc_read_counters(ctxp, C.byref(cctx[(frame_no[0] - 1) % len(hiz)]), C.byref(out), sp))
        ne = out.early_visible_meshlet_instances
        nv = ne + out.late_visible_meshlet_instances
        vis = frame.visible_meshlet_instances_indices_buffer[:nv].to(torch.int64)
        idx = frame.reordered_indices_buffer[:out.draw_index_count * W].to(torch.int64) & 0xFFFFFFFF
        if pairs:
            idx = (idx.view(-1, 2)[:, 0] << 32) | idx.view(-1, 2)[:, 1]
        if use_unord[0]:
            vis = torch.cat([torch.sort(vis[:ne])[0], torch.sort(vis[ne:])[0]])
            idx = torch.sort(idx)[0]
        if pairs:
            idx = idx % 2147483629  # (keeps the weighted sum below inside int64)
        wv = torch.arange(1, 1 + vis.numel(), device=dev, dtype=torch.int64) % 1000003
        wi = torch.arange(1, 1 + idx.numel(), device=dev, dtype=torch.int64) % 1000003
        return (out.early_visible_meshlet_instances, out.late_visible_meshlet_instances, out.draw_index_count, int((vis * wv).sum().item()),
                int((idx * wi).sum().item()), int(mask.to(torch.int64).sum().item()))

    ramp_clocks(e)
    elapsed = timed_steps(e, run_step, args.steps, args.warmup)
    per_rank_ms_per_frame = [round(t * 1e3 / (args.steps * inner), 6) for t in PER_RANK_SECONDS]
    per_rank_visible, ranks_seen = None, None
    if world > 1:  # the all-gathered counters of the last frame: {emitted by the late call, early, late, index_count} per rank
        torch.cuda.synchronize()
        gcpu = gathered.cpu().view(world, 4)
        per_rank_visible = [int(gcpu[k, 1] + gcpu[k, 2]) for k in range(world)]
        ranks_seen = int((gcpu.to(torch.int64).abs().sum(1) > 0).sum().item())  # rows of the gathered counters some rank has filled in
    frames = args.steps * inner
    ms_per_frame = elapsed * 1e3 / frames
    value = world_meshlets * frames / elapsed
    main_async, main_ahead, main_share, main_unord = use_async[0], use_overlap[0], use_share[0], use_unord[0]

    def base_line(counts, exchange_ab=None):
        """The result line's contract keys and config; a --full run adds its checks and measurements."""
        n_tri = None if counts["early_index_count"] is None else counts["early_index_count"] // 3 + counts["late_index_count"] // 3
        return {
            "metric": "meshlets/s culled", "value": round(value, 1), "unit": "meshlets/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1e3 / args.steps, 6), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": ("configs[2]: 10M meshlets + 4096^2 prior-frame HiZ (13 mips, built from an 8192^2 depth): HiZ build + early/late occlusion cull + "
                             "per-triangle cull + compaction into the indirect-draw buffers (" + ("unordered_output = 1: slots allocated by atomic_add as in the reference, lists "
                             "compared sorted" if main_unord else "ascending lists") + ")" if world == 1 else
                             f"configs[3]: {world_meshlets} meshlets sharded {world} ways by " + ("contiguous range" if not (shard_desc and shard_desc["shard_block_instances"] > 0) else shard_desc["assignment"]) + (" of ONE scene" if shard_desc else " (an independent scene per rank)") + " (the configs[2] pipeline per rank): rank 0 builds the "
                             "4096^2 pyramid and broadcasts it over RCCL/xGMI, per-rank counters all-gathered every frame, shard-local ids and outputs"),
                "meshlets_per_gpu": n_meshlets, "mesh_instances": M, "meshlets_per_mesh": K, "tris_per_meshlet": args.tris, "verts_per_meshlet": 64,
                "index_form": ("pairs {u32 id, u32 corner}, 24 B per triangle (wide_triangle_index = 2)" if pairs else "(id << 9) | corner (wide_triangle_index = 1)" if wide else "(id << 8) | corner (visbuffer.slang:9-14)"),
                "inner_reps": inner, "frames_timed": frames, "ms_per_frame": round(ms_per_frame, 6), "small_triangle_cull": bool(args.small_triangle_cull),
                "visible_fraction": round((counts["early"] + counts["late"]) / n_meshlets, 4),
                "triangles_per_visible_meshlet": None if n_tri is None else round(n_tri / max(1, counts["early"] + counts["late"]), 2),
                "sharding": "single GPU" if world == 1 else {"ranks": world, "rccl_ranks": 0 if e.debug_backend else world, "rccl_ranks_seen": 0 if e.debug_backend else ranks_seen, "debug_backend_not_a_measurement": e.debug_backend or None, "backend": "oxc_comm_* (RCCL via the C ABI)" if use_native[0] else (f"torch.distributed {e.debug_backend} (debug)" if e.debug_backend else "torch.distributed nccl (RCCL)"),
                                                             "hiz_exchange": (f"levels >= {k_top} broadcast, lower levels built by every rank from its own depth copy" if xmode["top"] else "whole pyramid broadcast from rank 0"),
                                                             "hiz_broadcast_bytes_per_frame": hiz_wire_bytes, "hiz_one_frame_ahead_on_second_stream": use_overlap[0],
                                                             "counters_all_gather_bytes_per_rank": 16, "per_rank_ms_per_frame": per_rank_ms_per_frame,
                                                             "per_rank_visible": per_rank_visible, "scene": shard_desc or {"one_scene": False, "note": "an independent scene per rank (seed + rank): no visibility skew between ranks by construction; --one-scene shards one scene"},
                                                             "hiz_exchange_ab": exchange_ab},
                "async_triangles": bool(use_async[0]), "share_pass_tests": bool(use_share[0]), "unordered_output": main_unord,
            },
        }

    # ---- the last timed frame's outputs (--dump-outputs), before anything below runs another frame ----
    torch.cuda.synchronize()
    last_b = (frame_no[0] - 1) % len(hiz)
    last = L.Counters()
    check(lib.oxc_read_counters(ctxp, C.byref(cctx[last_b]), C.byref(last), sp))
    ne, nl = last.early_visible_meshlet_instances, last.late_visible_meshlet_instances
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, (last.total_visible_meshlet_instances, ne, nl, last.draw_index_count), frame.visible_meshlet_instances_indices_buffer[:ne + nl], ne,
                     frame.reordered_indices_buffer[:last.draw_index_count * W], pairs, mask, hiz[last_b].data)
    if not args.full:
        r_hiz.close()
        return base_line({"total": last.total_visible_meshlet_instances, "early": ne, "late": nl, "early_index_count": None, "late_index_count": last.draw_index_count})
    sum_main = outputs_checksum()

    # ---- the same frames under other schedulings, short runs: (a) async_triangles flipped -- the triangle stage of a call on the context's
    # own stream beside the next call's meshlet stage / the next HiZ build; (b, N = 1) the pyramid of the NEXT frame built on a second
    # stream beside this frame's cull (what N > 1 does by default); (c) both.  Every variant must leave the outputs of the in-order run.
    ab_steps = max(2, args.steps // 4)

    def timed_variant(async_on, ahead_on, share_on, unord=None):
        use_async[0], use_overlap[0], use_share[0] = async_on, ahead_on, share_on
        use_unord[0] = main_unord if unord is None else unord
        if rank == 0 and os.environ.get("OXC_BENCH_TRACE"):
            print(f"[bench]   variant async={async_on} ahead={ahead_on} share={share_on} unordered={use_unord[0]}", file=sys.stderr, flush=True)
        el = timed_steps(e, run_step, ab_steps, 1)
        return {"async_triangles": async_on, "hiz_one_frame_ahead_on_second_stream": ahead_on, "share_pass_tests": share_on, "unordered_output": use_unord[0],
                "ms_per_frame": round(el * 1e3 / (ab_steps * inner), 6),
                "value": round(world_meshlets * ab_steps * inner / el, 1), "frames_timed": ab_steps * inner, "outputs_match_main_line": outputs_checksum() == sum_main}

    variants = []
    if not args.no_scheduling_ab:
        for other in (u for u in (0, 1) if u != main_unord):  # the list layouts of include/oxcull.h (compared as sorted sets)
            variants.append(timed_variant(main_async, main_ahead, main_share, other))
        variants.append(timed_variant(main_async, main_ahead, not main_share))
        if main_share or main_unord:  # the library's all-defaults form: ascending lists, every call testing on its own
            variants.append(timed_variant(main_async, main_ahead, False, 0))
            variants[-1]["library_defaults"] = True
        variants.append(timed_variant(not main_async, main_ahead, main_share))
        if world == 1:
            variants.append(timed_variant(main_async, not main_ahead, main_share))
            variants.append(timed_variant(not main_async, not main_ahead, main_share))
        use_async[0], use_overlap[0], use_share[0], use_unord[0] = main_async, main_ahead, main_share, main_unord
        with torch.cuda.stream(stream):
            run_frame()  # (back in the main line's form before the kernel profile below)
        torch.cuda.synchronize()
    sched_ab = {"main_line": {"async_triangles": main_async, "hiz_one_frame_ahead_on_second_stream": main_ahead, "share_pass_tests": main_share,
                              "unordered_output": main_unord, "ms_per_frame": round(ms_per_frame, 6)},
                "variants": variants,
                "note": "unordered_output (include/oxcull.h): 0 = ascending lists, test + ordered emit per stage; 1 = the triangle stage as ONE launch that appends behind an "
                        "atomic_add on index_count per 128-meshlet span (cull_triangles.slang:71-88), the last partial round of spans handed out in 64-meshlet chunks by ticket; the HiZ "
                        "meshlet stage keeps its ordered emit -- variants are compared with the main line as sorted sets.  library_defaults = ordered + unshared.  "
                        "share_pass_tests: the late call of a frame reads the early call's frustum + cone results (one bit per meshlet) instead of testing again -- a cache "
                        "inside liboxcull, valid because both calls of a frame have the same camera, transforms and list (RendererInstance.cpp:842-884); the variant that flips it is "
                        "the frame with every call testing on its own.  async_triangles: hipStreamWaitEvent fork / join inside liboxcull (include/oxcull.h); one frame ahead: bench-side second stream + second context with "
                        "events both ways, double-buffered pyramid -- legal here because the depth image a frame's pyramid is built from is given; in the engine the "
                        "pyramid is built from the early draw's depth between the two culls of a frame (RendererInstance.cpp:842-884), which is why the main line stays in order"}

    # ---- N > 1: the other --hiz-exchange form, a short run, so that one multi-GPU run decides between them ----
    exchange_ab = None
    if world > 1 and not args.no_exchange_ab:
        exchange_ab = {("top" if xmode["top"] else "whole"): {"ms_per_frame": round(ms_per_frame, 6), "broadcast_bytes_per_frame": wire_bytes(xmode["top"])}}
        xmode["top"] = not xmode["top"]
        el_x = timed_steps(e, run_step, ab_steps, 1)
        exchange_ab["top" if xmode["top"] else "whole"] = {"ms_per_frame": round(el_x * 1e3 / (ab_steps * inner), 6), "broadcast_bytes_per_frame": wire_bytes(xmode["top"]),
                                                            "frames_timed": ab_steps * inner}
        xmode["top"] = not xmode["top"]
        with torch.cuda.stream(stream):
            run_frame()  # (leaves the pyramids in the main mode's state for the kernel profile below)
        torch.cuda.synchronize()

    # ---- SURVEY 8d's f: candidates that reach test_occlusion (four pyramid taps = 16 B each), counted by the counting instantiations of
    # the two meshlet tests in one untimed frame (oxc_debug_count_occlusion_candidates) ----
    occl_candidates = {"early": None, "late": None}
    if hasattr(lib, "oxc_debug_count_occlusion_candidates"):
        cnt = [torch.zeros(256 * 64, dtype=torch.int32, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            mask.copy_(mask0, non_blocking=True)
            produce_hiz(0, False)
            c = cctx[0]
            c.async_triangles, c.share_pass_tests, c.unordered_output = 0, int(use_share[0]), use_unord[0]
            for k_, flags in enumerate((L.CULL_TEST_ALL, L.CULL_TEST_ALL | L.CULL_LATE_PASS)):
                check(lib.oxc_debug_count_occlusion_candidates(ctxp, C.c_void_p(cnt[k_].data_ptr())))
                c.cull_flags = flags
                check(lib.oxc_cull_geometry(ctxp, pf, C.byref(c), sp))
            check(lib.oxc_debug_count_occlusion_candidates(ctxp, None))
        torch.cuda.synchronize()
        occl_candidates = {"early": int(cnt[0].to(torch.int64).sum().item()), "late": int(cnt[1].to(torch.int64).sum().item())}
        if outputs_checksum() != sum_main and rank == 0:
            print("[bench] WARNING: the counting instantiations changed an output", file=sys.stderr, flush=True)
        del cnt

    # ---- per-kernel times (>= 50 launches each) and rooflines: algorithmic bytes of SURVEY 8d ----
    if rank == 0 and os.environ.get("OXC_BENCH_TRACE"):
        print("[bench]   kernel profile", file=sys.stderr, flush=True)
    n_prof = max(50, min(inner, 96))
    renderers = [r, r_hiz]
    kern = profile_kernels(e, renderers, lambda i: run_frame(), n_prof)
    tri_bytes_per_meshlet = 4 + 8 + 16 + (3 * args.tris + 3) // 4 * 4 + 4 * 64 + 8 * 64  # 988 B (V=64, T=64), SURVEY 8d a11
    H = 2 if wide else 1
    alg = {  # per launch
        "hiz": hiz_algorithmic_bytes(HW, HW, hiz[0].levels),
        "prepare_instances": M * (212 + 384),
        # 8 B MeshletInstance + 16 B MeshletBounds per meshlet + the mask word read and written (1/8 B each) + SURVEY 8d's 16 f: four
        # pyramid taps per candidate that reaches test_occlusion (counted above; round 4 left them out)
        "cull_meshlets_test": n_meshlets * (24.0 + 0.25) + 16.0 * (occl_candidates["early"] or 0),
        "cull_meshlets_test_late": n_meshlets * (24.0 + 0.25) + 16.0 * (occl_candidates["late"] or 0),
        "cull_meshlets_emit": n_meshlets / 8.0 + 4.0 * v_early,
        "cull_meshlets_emit_late": n_meshlets / 8.0 + 4.0 * v_late,
        "cull_triangles_test": v_early * (tri_bytes_per_meshlet + 8.0 * H),
        "cull_triangles_test_late": v_late * (tri_bytes_per_meshlet + 8.0 * H),
        "cull_triangles_emit": v_early * (8.0 * H + 4.0) + 12.0 * t_early,
        "cull_triangles_emit_late": v_late * (8.0 * H + 4.0) + 12.0 * t_late,
    }
    tri_out_bytes = 12.0 * W  # per emitted triangle: three u32 indices, or three {u32 id, u32 corner} pairs (24 B)
    alg["cull_triangles_emit"] = v_early * (8.0 * H + 4.0) + tri_out_bytes * t_early
    alg["cull_triangles_emit_late"] = v_late * (8.0 * H + 4.0) + tri_out_bytes * t_late
    if main_unord:  # the fused kernel tests AND expands: no pass masks or visible ids through memory (-2 x 8 H, -4 B per visible meshlet)
        alg["cull_triangles_test"] = v_early * tri_bytes_per_meshlet + tri_out_bytes * t_early
        alg["cull_triangles_test_late"] = v_late * tri_bytes_per_meshlet + tri_out_bytes * t_late
    # the second clock: the committed rocprofv3 --kernel-trace --stats averages of the same kernels (of the build the profile was taken
    # from; HIP-event spans above include ~4.5 us of event overhead per launch, reported as _empty_event_pair_us, not subtracted)
    # (the committed profiles are of the default workload: T = 64, ordered lists; any other shape has no counters of its own and says so)
    std_shape = not args.small_triangle_cull and main_unord == 1 and main_share
    prof_names = ([f"{t}_config3_pmc.json" for t in PROFILE_ROUNDS] if (std_shape and not wide and n_meshlets == 10_000_000) else
                  [f"{t}_pairs124_pmc.json" for t in PROFILE_ROUNDS] if (std_shape and pairs and n_meshlets == 10_000_000) else
                  [f"{t}_tris124_pmc.json" for t in PROFILE_ROUNDS] if (std_shape and wide and not pairs and n_meshlets == 8_000_000) else [])
    rp = rocprof_kernel_us(prof_names) if prof_names else {}
    pmc_rw = pmc_read_written(prof_names) if prof_names else {}
    rp_names = {"prepare_instances": ["oxc::k_prepare_instances"], "hiz": ["oxc::k_hiz_tile", "oxc::k_hiz_tail"],
                "cull_meshlets_test": ["oxc::k_cull_meshlets_test_shared<false>" if main_share else "oxc::k_cull_meshlets_test<true, true, false, 4>"],
                "cull_meshlets_test_late": ["oxc::k_cull_meshlets_test_shared<true>" if main_share else "oxc::k_cull_meshlets_test<true, true, true, 4>"],
                "cull_meshlets_emit": ["oxc::k_cull_meshlets_emit<true, false>"], "cull_meshlets_emit_late": ["oxc::k_cull_meshlets_emit<true, true>"],
                "cull_triangles_test": ["oxc::k_cull_triangles_fused_pairs<false, false>" if (main_unord and pairs) else f"oxc::k_cull_triangles_fused<false, {str(wide).lower()}, false>" if main_unord else f"oxc::k_cull_triangles_test<false, {str(wide).lower()}, false>"],
                "cull_triangles_test_late": ["oxc::k_cull_triangles_fused_pairs<true, false>" if (main_unord and pairs) else f"oxc::k_cull_triangles_fused<true, {str(wide).lower()}, false>" if main_unord else f"oxc::k_cull_triangles_test<true, {str(wide).lower()}, false>"],
                "cull_triangles_emit": ["oxc::k_cull_triangles_emit_pairs<false>" if pairs else f"oxc::k_cull_triangles_emit<false, {str(wide).lower()}>"],
                "cull_triangles_emit_late": ["oxc::k_cull_triangles_emit_pairs<true>" if pairs else f"oxc::k_cull_triangles_emit<true, {str(wide).lower()}>"]}
    kernels, frame_alg, frame_kernel_us = {}, 0.0, 0.0
    for name, k in kern.items():
        if name.startswith("_"):
            kernels[name] = k
            continue
        per_frame = k["launches"] / n_prof
        ent = {"launches_per_frame": round(per_frame, 3), "launches_timed": k["launches"], "avg_us": round(k["avg_us"], 3)}
        if all(n in rp for n in rp_names.get(name, ["?"])):
            ent["kernel_avg_us_rocprof"] = round(sum(rp[n] for n in rp_names[name]), 3)
        if all(n in pmc_rw for n in rp_names.get(name, ["?"])):  # HBM bytes per launch by the PMC counters of the committed profile (read x 2 correction applied, + written)
            ent["traffic"] = round(sum(sum(pmc_rw[n]) for n in rp_names[name]))
            ent["traffic_read_written"] = [round(sum(pmc_rw[n][0] for n in rp_names[name])), round(sum(pmc_rw[n][1] for n in rp_names[name]))]
        b = alg.get(name)
        if b is not None:
            ent["algorithmic_bytes_per_launch"] = round(b)
            ent["achieved_GBps"] = round(b / (k["avg_us"] * 1e-6) / 1e9, 1)
            ent["frac"] = round(b / (k["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4)
            frame_alg += b * per_frame
        frame_kernel_us += k["avg_us"] * per_frame
        if b is not None and name in ("cull_meshlets_test", "cull_meshlets_test_late"):
            ent["traffic_over_algorithmic"] = round(ent["traffic"] / b, 3) if "traffic" in ent else None
        if name == "hiz" and "traffic" in ent:
            ent["traffic_over_algorithmic"] = round(ent["traffic"] / b, 3)
            ent["achieved_traffic_GBps"] = round(ent["traffic"] / (k["avg_us"] * 1e-6) / 1e9, 1)
            ent["note"] = ("parity mode: the reference's mip-0 point sample at (2x+2, 2y+2) (hiz.slang:92-95) touches every line of every other depth row and uses half of it: "
                           "the read side fetches ~2.6x the sampled texels; frac is on SURVEY 8d's algorithmic bytes, achieved_traffic_GBps is what the memory system moved")
        kernels[name] = ent
    # dominant kernel: the triangle test (both instantiations: early + late launch of a frame)
    tt = [kern[n] for n in ("cull_triangles_test", "cull_triangles_test_late") if n in kern]
    roofline = None
    stream_gbps = stream_read_ceiling(e)
    if tt:
        dom_us = sum(k["avg_us"] * k["launches"] for k in tt) / sum(k["launches"] for k in tt)
        dom_bytes = (alg["cull_triangles_test"] + alg["cull_triangles_test_late"]) / 2.0
        achieved = dom_bytes / (dom_us * 1e-6) / 1e9
        dom_name = ("k_cull_triangles_fused_pairs" if pairs else "k_cull_triangles_fused") if main_unord else "k_cull_triangles_test"
        traffic, traffic_src, traffic_same = pmc_traffic(prof_names, lambda k: dom_name in k) if prof_names else (None, None, None)
        roofline = {"bound": "hbm", "kernel": f"{dom_name} (early + late launch of a frame, averaged" + (f"; test + expansion in one launch: {tri_bytes_per_meshlet} B read per visible meshlet + {int(tri_out_bytes)} B written per emitted triangle)" if main_unord else ")"),
                    "achieved": round(achieved, 1),
                    "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "traffic_over_algorithmic": round(traffic / dom_bytes, 3) if traffic else None,
                    "traffic_profile_is_of_this_device_code": traffic_same, "algorithmic_bytes_per_launch": round(dom_bytes), "kernel_avg_us": round(dom_us, 3),
                    "launches_averaged": sum(k["launches"] for k in tt), "measured_stream_read_GBps": round(stream_gbps, 1),
                    "frac_of_measured_stream_read": round(achieved / stream_gbps, 4)}
        rpn = rp_names["cull_triangles_test"] + rp_names["cull_triangles_test_late"]
        if all(n in rp for n in rpn):  # the committed rocprofv3 --kernel-trace --stats average of the same two instantiations
            roofline["kernel_avg_us_rocprof"] = round(sum(rp[n] for n in rpn) / 2.0, 3)
    # The same frame charged with the bytes THIS design needs (weak #4 of the round-5 review): with share_pass_tests the late meshlet test reads the early
    # call's pass bit and the mask word for every meshlet (0.375 B) but the MeshletInstance record + bounds (24 B) only of meshlets that passed the camera
    # tests (= its occlusion candidates, counted) -- the reference's flow charges 24.25 B for every meshlet.
    needed_late = None
    if main_share and occl_candidates["late"] is not None and "cull_meshlets_test_late" in kern:
        needed_late = n_meshlets * 0.375 + (24.0 + 16.0) * occl_candidates["late"]
    frame_needed = frame_alg - ((alg["cull_meshlets_test_late"] - needed_late) if needed_late is not None else 0.0)
    stage = {"algorithmic_bytes_per_frame": round(frame_alg), "ms_per_frame": round(ms_per_frame, 6),
             "achieved_GBps": round(frame_alg / (ms_per_frame * 1e-3) / 1e9, 1), "stage_frac": round(frame_alg / (ms_per_frame * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
             "needed_bytes_per_frame": round(frame_needed), "stage_frac_needed_bytes": round(frame_needed / (ms_per_frame * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
             "sum_of_kernel_us_per_frame": round(frame_kernel_us, 1),
             "occlusion_candidates": occl_candidates,
             "note": "whole frame (HiZ build + early + late, every kernel) against the 8 TB/s peak; bytes = SURVEY 8d per-kernel figures incl. 16 B of pyramid taps per occlusion candidate (counted).  "
                     "With share_pass_tests the late meshlet test is still CHARGED the reference's 24.25 B per meshlet although it fetches ~14.7 (no MeshletInstance "
                     "record and no bounds for steps nothing of which passed the camera tests): ~95 MB of the frame's algorithmic bytes, and that kernel's frac, are the "
                     "reference's traffic, not this kernel's (SURVEY 8d defines algorithmic bytes by the reference's data flow)"}

    # ---- CPU checker on a bounded prefix of the SAME arrays: bit_match + cpu_baseline (rank 0, N = 1) ----
    bit_match, cpu_baseline, hiz_match, unpinned, bit_detail = None, None, None, None, None
    if rank == 0 and os.environ.get("OXC_BENCH_TRACE"):
        print("[bench]   checker", file=sys.stderr, flush=True)
    if rank == 0:
        import oracle  # checker only

        oracle.build()
        m0 = min(args.cpu_prefix, M)
        sub = scene.prefix(m0, "cpu")
        cam = sub.cull_camera()
        hz_cpu = hiz[0].data.cpu()
        if world == 1 and not args.no_cpu_baseline:  # the checker builds the pyramid itself from the same depth image
            dcpu = depth.data.view(2 * HW, 2 * HW).cpu()
            own = torch.zeros_like(hz_cpu)
            t_h0 = time.perf_counter()
            oracle.generate_hiz(dcpu, own, HW, HW, hiz[0].levels, hiz[0].level_offset)
            t_hiz_cpu = time.perf_counter() - t_h0
            hiz_match = bool(torch.equal(own.view(torch.int32), hz_cpu.view(torch.int32)))
            del dcpu, own
        hz = oracle.make_hiz(hz_cpu, HW, HW, hiz[0].levels, hiz[0].level_offset)
        mask_cpu0 = mask0[: (m0 * K + 31) // 32].cpu()

        def cpu_sequence():
            v = oracle.Visibility(m0 * K, 0, 0)
            out = torch.zeros(m0 * K, dtype=torch.int32)
            mk = mask_cpu0.clone()
            res = {}
            for tag, flags in (("early", L.CULL_TEST_ALL), ("late", L.CULL_TEST_ALL | L.CULL_LATE_PASS)):
                n_e = oracle.cull_meshlets_hiz(sub, cam, sub.meshlet_instances, flags, hz, v, mk, out)
                first = v.early if tag == "late" else 0
                res[tag] = (out[first:first + n_e].clone(),
                            oracle.cull_triangles(sub, cam, sub.meshlet_instances, out, first, n_e, wide=wti, small_triangle_cull=args.small_triangle_cull))
            return res, mk

        t_c0 = time.perf_counter()
        want, mask_want = cpu_sequence()
        t_seq = time.perf_counter() - t_c0
        bit_detail = {f"{t}_{what}": bool(want[t][i].numel() == snap[t][key].numel() and torch.equal(want[t][i], snap[t][key]))
                      for t in ("early", "late") for i, what, key in ((0, "visible", "visible_prefix"), (1, "indices", "indices_prefix"))}
        nbits = m0 * K  # (the sample's mask bits: whole words, and the low bits of the word it shares with the next instance)
        mw, ma = mask_want.clone(), mask_after.clone()
        if nbits % 32:
            keep = (1 << (nbits % 32)) - 1
            mw[-1] &= keep
            ma[-1] &= keep
        bit_detail["mask"] = bool(torch.equal(mw, ma))
        bit_match = all(bit_detail.values())
        if not args.no_cpu_baseline:
            # What no oracle can pin (the reference is compiled fast-math and ships no vectors): on the same sample, how many decisions
            # change under fused multiply-adds / reciprocal divisions, and how many triangles are ill-conditioned at all.
            with oracle.variant("fast"):
                fast, mask_fast = cpu_sequence()
            def tri1(t):  # one key per emitted triangle: its first index (packed u32, or the pair as id << 32 | corner)
                if not t.numel():
                    return torch.zeros(0).numpy()
                if pairs:
                    a6 = t.view(-1, 6).numpy().astype("int64") & 0xFFFFFFFF
                    return (a6[:, 0] << 32) | a6[:, 1]
                return t.view(-1, 3)[:, 0].numpy().astype("int64") & 0xFFFFFFFF

            import numpy as _np

            flags = oracle.triangle_boundary_flags(sub, cam, sub.meshlet_instances, want["late"][0], 0, want["late"][0].numel())
            unpinned = {"sample": f"first {m0 * K} meshlet instances, both passes", "visible_meshlets_differ": sum(int(_np.setxor1d(want[t][0].numpy(), fast[t][0].numpy()).size) for t in ("early", "late")),
                        "mask_bits_differ": int(_np.unpackbits((mask_want.numpy() ^ mask_fast.numpy()).view(_np.uint8)).sum()),
                        "triangles_differ": sum(int(_np.setxor1d(tri1(want[t][1]), tri1(fast[t][1])).size) for t in ("early", "late")),
                        "triangles_emitted": sum(int(want[t][1].numel() // 3) for t in ("early", "late")),
                        "late_triangles_tested": int(want["late"][0].numel()) * min(args.tris, 64), "late_triangles_ill_conditioned": int(flags.sum()),
                        "note": "canonical checker vs its fast-math-envelope build (oracle/Makefile); tools/unpinned_gap.py, profiles/r02_unpinned_gap.json"}
        if world == 1 and not args.no_cpu_baseline:
            reps = int(max(1, min(args.cpu_seconds / 2 / max(t_seq, 1e-3), 200)))
            t_c0 = time.perf_counter()
            for _ in range(reps):
                cpu_sequence()
            dt = (time.perf_counter() - t_c0) / reps
            share = t_hiz_cpu * (m0 * K) / n_meshlets  # the pyramid build serves all N meshlets: its share for the sample
            single = m0 * K / (dt + share)

            # All host cores: the instance range split into word-aligned pieces (4 instances x 1000 meshlets = 125 mask words, so no two
            # threads share a mask word), each thread runs both passes + both triangle passes over its piece with private output buffers,
            # then the pieces are concatenated in order (ids and packed indices rebased) -- and must equal the one-thread result.
            from concurrent.futures import ThreadPoolExecutor

            cores = usable_cores()
            pool = ThreadPoolExecutor(max_workers=cores)
            # (four pieces per thread, handed out in order by a pool: visibility is spatially coherent, so equal ranges are not equal work)
            piece = max(4, -(-(-(-m0 // (4 * cores))) // 4) * 4)  # ceil(m0 / (4 cores)) rounded up to a multiple of 4 instances
            cuts = list(range(0, m0, piece)) + [m0]
            ranges = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
            shift = 9 if wide else 8

            def cpu_piece(a, b, mk, box, slot):
                mli = sub.meshlet_instances[a * K:b * K]
                v = oracle.Visibility((b - a) * K, 0, 0)
                out = torch.zeros((b - a) * K, dtype=torch.int32)
                res = {}
                for tag, flags in (("early", L.CULL_TEST_ALL), ("late", L.CULL_TEST_ALL | L.CULL_LATE_PASS)):
                    n_e = oracle.cull_meshlets_hiz(sub, cam, mli, flags, hz, v, mk, out)
                    first = v.early if tag == "late" else 0
                    res[tag] = (out[first:first + n_e].clone(),
                                oracle.cull_triangles(sub, cam, mli, out, first, n_e, wide=wti, small_triangle_cull=args.small_triangle_cull))
                box[slot] = res

            def cpu_sequence_mt():
                mk = mask_cpu0.clone()
                box = [None] * len(ranges)
                list(pool.map(lambda it: cpu_piece(it[1][0], it[1][1], mk, box, it[0]), enumerate(ranges)))
                res = {}
                for tag in ("early", "late"):
                    def rebase(t, a):  # a piece's indices name piece-local ids
                        if not pairs:
                            return t + ((a * K) << shift)
                        t = t.clone()
                        t.view(-1, 2)[:, 0] += a * K
                        return t

                    res[tag] = (torch.cat([box[i][tag][0] + a * K for i, (a, b) in enumerate(ranges)]),
                                torch.cat([rebase(box[i][tag][1], a) for i, (a, b) in enumerate(ranges)]))
                return res, mk

            got_mt, mask_mt = cpu_sequence_mt()
            mt_ok = bool(all(torch.equal(got_mt[t][0], want[t][0]) and torch.equal(got_mt[t][1], want[t][1]) for t in ("early", "late")) and torch.equal(mask_mt, mask_want))
            reps_mt = int(max(2, min(args.cpu_seconds / 2 / max(t_seq / max(1, min(cores, len(ranges))) * 2, 1e-3), 400)))
            t_c0 = time.perf_counter()
            for _ in range(reps_mt):
                cpu_sequence_mt()
            dt_mt = (time.perf_counter() - t_c0) / reps_mt
            pool.shutdown()
            cpu_baseline = {"value": round(m0 * K / (dt_mt + share), 1), "unit": "meshlets/s", "cores": min(cores, len(ranges)), "host_cores_usable": cores, "kind": "port",
                            "sample": f"{reps_mt} runs of the same sequence (cull_meshlets_hiz early + cull_triangles, late + cull_triangles; oracle/oxcull_oracle.c, scalar C) over the "
                                      f"first {m0 * K} meshlet instances of the same arrays, the instance range cut into {len(ranges)} word-aligned pieces worked off by a pool of "
                                      f"{min(cores, len(ranges))} threads, private outputs concatenated in order ({dt_mt:.3f} s per run; equals the one-thread result: {mt_ok}) + that sample's share of the scalar, "
                                      f"one-thread 4096^2 pyramid build ({t_hiz_cpu:.2f} s for the whole image)",
                            "matches_single_thread": mt_ok, "single_thread_value": round(single, 1), "single_thread_sequence_s_per_run": round(dt, 3),
                            "hiz_build_s": round(t_hiz_cpu, 3), "sequence_s_per_run": round(dt_mt, 4)}

    line = base_line(counts, exchange_ab)
    line.update({
        "bit_match": bit_match, "bit_match_detail": bit_detail if rank == 0 else None, "hiz_bit_match": hiz_match, "bit_match_sample": f"first {min(args.cpu_prefix, M) * K} meshlet instances: visible lists, packed triangle indices, mask words, both passes",
        "unpinned_gap": unpinned, "counts": counts, "kernels": kernels, "stage": stage, "roofline": roofline, "cpu_baseline": cpu_baseline,
        "scheduling_ab": sched_ab,
    })
    # ---- N > 1: the same frames with BOTH exchanges through the other RCCL path -- the C ABI's own entry points (oxc_exchange_counts,
    # oxc_broadcast_hiz[_levels]: SURVEY 8b lists them in the boundary) when the main line ran on torch.distributed, and the reverse with
    # --native-comm -- a short run, outputs check-summed against the main line.  These entry points had never run with more than one rank
    # when this was written (one-GPU builder box): every failure is caught and reported, and a hang is cut off by a watchdog that prints the
    # main line as it stands and ends the process, so the run keeps its headline whatever the exchange does.
    if world > 1 and not getattr(args, "no_native_comm_ab", False):
        if native_ready is False:
            line["native_comm_ab"] = {"skipped": native_error or "the communicators could not be set up"}
        else:
            import threading

            done = threading.Event()

            def watchdog():
                if done.wait(float(os.environ.get("OXC_BENCH_NATIVE_AB_TIMEOUT", "120"))):
                    return
                if rank == 0:
                    line["native_comm_ab"] = {"timed_out_s": float(os.environ.get("OXC_BENCH_NATIVE_AB_TIMEOUT", "120")), "note": "the run with the other exchange path did not finish: "
                                              "the process was ended by the watchdog after printing the main line"}
                    line["summary"] = line_summary(line)
                    emit(line)
                sys.stdout.flush()
                if rank != 0:
                    time.sleep(5.0)  # rank 0 prints first; a launcher that sees a rank die would take the others down
                os._exit(0)

            threading.Thread(target=watchdog, daemon=True).start()
            if native_ready is None:  # the communicators of the two contexts, now that the main line is safe (under the watchdog)
                if e.native_ready is None:
                    e.native_ready, e.native_error = native_comm_init(e, r)
                native_ready, native_error = e.native_ready, e.native_error
                if native_ready:
                    native_ready, native_error = native_comm_init(e, r_hiz)
            main_native = use_native[0]
            res_n = {"path": "torch.distributed nccl (RCCL)" if main_native else "oxc_comm_* (RCCL via the C ABI: oxc_exchange_counts, oxc_broadcast_hiz" + ("_levels)" if xmode["top"] else ")")}
            try:
                if not native_ready:
                    raise RuntimeError(f"oxc_comm_init: {native_error}")
                use_native[0] = not main_native
                gathered.zero_()
                el_n = timed_steps(e, run_step, ab_steps, 1)
                sum_n = outputs_checksum()
                g2 = gathered.cpu().view(world, 4)
                res_n.update({"ms_per_frame": round(el_n * 1e3 / (ab_steps * inner), 6), "value": round(world_meshlets * ab_steps * inner / el_n, 1), "frames_timed": ab_steps * inner,
                              "outputs_match_main_line": sum_n == sum_main, "rccl_ranks_seen": int((g2.to(torch.int64).abs().sum(1) > 0).sum().item()),
                              "per_rank_visible": [int(g2[k, 1] + g2[k, 2]) for k in range(world)], "main_line_ms_per_frame": round(ms_per_frame, 6)})
            except Exception as ex:  # noqa: BLE001  (OXC_RCCL_ERROR, ...; the other ranks then sit in a collective until the watchdog ends them)
                res_n["error"] = str(ex)[:300]
            use_native[0] = main_native
            errs = [None] * world
            dist.all_gather_object(errs, res_n.get("error"))
            if any(errs):
                res_n["error"] = next(x for x in errs if x)
            done.set()
            line["native_comm_ab"] = res_n
            with torch.cuda.stream(stream):
                run_frame()
            torch.cuda.synchronize()
    # free the 25 GB of this workload before the nested one
    r_hiz.close()
    del scene, frame, depth, hiz, mask0
    torch.cuda.empty_cache()
    return line


# ------------------------------------------------------------------------------------------------------------------
# configs[1]: 1M meshlets, one camera, frustum + cone cull + ordered compaction
# ------------------------------------------------------------------------------------------------------------------
def bench_config2(args, e, steps: int, warmup: int, with_cpu: bool):
    """A step = one 1M-meshlet frame (one RendererInstance::cull_geometry over one scene copy).  The 24 MB working set would sit
    in the 256 MB Infinity Cache, so frames rotate over >= 1.1 GB of independent copies.  A single call is three
    dependent launches of ~26 us in total, so it is measured twice: `batched` (16 frames per oxc_cull_geometry_batch launch, three
    contexts on three streams, eager) and `one_call_per_frame` (oxc_cull_geometry per frame, ONE stream, replayed from a HIP graph
    so the host is out of the picture)."""
    r, dev, stream, rank, world, dist = e.r, e.dev, e.stream, e.rank, e.world, e.dist
    lib = r._lib
    K = K_MESHLETS_PER_MESH
    n_meshlets = args.meshlets if (args.meshlets and args.workload == "config2") else 1_000_000
    M = max(1, n_meshlets // K)
    n_meshlets = M * K
    n_streams = max(1, args.streams)
    batch = max(1, min(16, args.batch))
    renderers = [r] + [RendererInstance(e.local_rank) for _ in range(n_streams - 1)]
    streams = [stream] + [torch.cuda.Stream(device=dev) for _ in range(n_streams - 1)]
    sps = [C.c_void_p(s_.cuda_stream) for s_ in streams]
    bytes_per_copy = n_meshlets * 24 + M * 212
    copies = args.copies or max(n_streams * batch, -(-1_150_000_000 // bytes_per_copy))
    copies = -(-copies // (n_streams * batch)) * (n_streams * batch)

    class Step:
        def __init__(self, rr, scene):
            self.frame = PreparedFrame.create(scene, with_triangles=False)
            self.cframe = self.frame.c()
            self.ctx = CullGeometryContext(use_hiz=False, init_cull_meshes=False, cull_flags=L.CULL_TEST_ALL, cull_camera=scene.cull_camera(), stages=L.STAGE_MESHLETS)
            rr.prepared_frame = self.frame
            rr.seed_meshlet_instances(self.ctx, scene.n_meshlet_instances)
            self.cctx = self.ctx.c()
            self.pf, self.pc = C.byref(self.cframe), C.byref(self.cctx)

    with torch.cuda.stream(stream):
        base = make_scene(SceneSpec(n_mesh_instances=M, meshlets_per_mesh=K, with_geometry=False, seed=0x0A1DE5 + 2 + rank), dev)
        scenes = [base] + [base.clone() for _ in range(copies - 1)]
        for rr in renderers:
            rr.reserve(M, n_meshlets)
        st_ = [Step(renderers[i % n_streams], s) for i, s in enumerate(scenes)]
    torch.cuda.synchronize()

    def check(rr, st):
        if st != L.OXC_OK:
            raise RuntimeError(lib.oxc_last_error(rr._ctx).decode())

    groups = []
    for k in range(n_streams):
        lst = [s for i, s in enumerate(st_) if i % n_streams == k]
        for j in range(0, len(lst), batch):
            grp = lst[j:j + batch]
            groups.append((k, (L.PreparedFrame * batch)(*[g_.cframe for g_ in grp]), (L.CullGeometryContext * batch)(*[g_.cctx for g_ in grp])))
    one_stream = [False]

    def run_group(gi):
        k, cf, cc = groups[gi % len(groups)]
        check(renderers[k], lib.oxc_cull_geometry_batch(renderers[k]._ctx, batch, cf, cc, sps[0] if one_stream[0] else sps[k]))

    # parity of what is timed: copy 0 against the checker
    with torch.cuda.stream(stream):
        check(r, lib.oxc_cull_geometry(r._ctx, st_[0].pf, st_[0].pc, sps[0]))
    torch.cuda.synchronize()
    c0 = r.read_counters(st_[0].ctx, stream)
    visible_fraction = c0.cull_triangles_cmd_x / n_meshlets
    bit_match, cpu_scene = None, None
    if rank == 0:
        import oracle

        oracle.build()
        cpu_scene = base.to("cpu")
        want = oracle.cull_meshlets(cpu_scene, cpu_scene.cull_camera(), cpu_scene.meshlet_instances, nthreads=os.cpu_count() or 1)
        got = st_[0].frame.visible_meshlet_instances_indices_buffer[: c0.cull_triangles_cmd_x].cpu()
        bit_match = bool(want.numel() == got.numel() and torch.equal(want, got))

    ramp_clocks(e, 0.5)
    # ---- (a) batched: `batch` frames per launch, n_streams contexts/streams, eager; a step = one frame ----
    inner = args.inner_reps if (args.inner_reps and args.workload == "config2") else 9600
    inner = max(batch, inner // batch * batch)

    def run_step(_i):
        for u in range(inner // batch):
            run_group(u)

    def fork_join_step(i):  # the side streams start after / are joined into the timing stream
        for s_ in streams[1:]:
            s_.wait_stream(stream)
        run_step(i)
        for s_ in streams[1:]:
            stream.wait_stream(s_)

    elapsed = timed_steps(e, fork_join_step, steps, warmup)
    value = n_meshlets * world * steps * inner / elapsed
    batched = {"value": round(value, 1), "ms_per_frame": round(elapsed * 1e3 / (steps * inner), 6), "frames_per_launch": batch, "streams": n_streams,
               "frames_timed": steps * inner, "seconds": round(elapsed, 3)}

    # ---- (b) one call per frame, one stream: a HIP graph of one rotation through the copies ----
    one_stream[0] = True
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1, stream=stream):
        for s in st_:
            check(r, lib.oxc_cull_geometry(r._ctx, s.pf, s.pc, sps[0]))
    reps1 = max(2, (steps * inner // 4) // copies)

    def replay(_i):
        for _ in range(reps1):
            g1.replay()

    el1 = timed_steps(e, replay, 1, 1)
    single = {"value": round(n_meshlets * world * reps1 * copies / el1, 1), "ms_per_frame": round(el1 * 1e3 / (reps1 * copies), 6), "frames_per_launch": 1, "streams": 1,
              "hip_graph": True, "frames_timed": reps1 * copies, "seconds": round(el1, 3)}
    del g1

    # ---- (c) the same single call with unordered_output = 1 (include/oxcull.h): the test kernel appends its survivors behind one atomic_add per
    # 1024 meshlets (cull_meshlets.slang:55-70 aggregated through the ballots) and no emit kernel runs -- two launches per call instead of three
    for s_ in st_:
        s_.cctx.unordered_output = 1
    with torch.cuda.stream(stream):
        st_[0].frame.visible_meshlet_instances_indices_buffer.fill_(-1)
        check(r, lib.oxc_cull_geometry(r._ctx, st_[0].pf, st_[0].pc, sps[0]))
    torch.cuda.synchronize()
    cu = L.Counters()
    check(r, lib.oxc_read_counters(r._ctx, st_[0].pc, C.byref(cu), sps[0]))
    unordered_match = None
    if rank == 0:
        got_u = torch.sort(st_[0].frame.visible_meshlet_instances_indices_buffer[: cu.cull_triangles_cmd_x])[0].cpu()
        unordered_match = bool(cu.cull_triangles_cmd_x == c0.cull_triangles_cmd_x and torch.equal(want, got_u))
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=stream):
        for s_ in st_:
            check(r, lib.oxc_cull_geometry(r._ctx, s_.pf, s_.pc, sps[0]))

    def replay2(_i):
        for _ in range(reps1):
            g2.replay()

    el2 = timed_steps(e, replay2, 1, 1)
    single_unordered = {"value": round(n_meshlets * world * reps1 * copies / el2, 1), "ms_per_frame": round(el2 * 1e3 / (reps1 * copies), 6), "frames_per_launch": 1, "streams": 1,
                        "hip_graph": True, "unordered_output": 1, "launches_per_call": 2, "frames_timed": reps1 * copies, "seconds": round(el2, 3),
                        "sorted_list_equals_the_checkers": unordered_match}
    del g2
    for s_ in st_:
        s_.cctx.unordered_output = 0

    # ---- per-kernel times on one stream (>= 50 batched launches) and the roofline of the dominant kernel ----
    n_prof = max(50, min(len(groups), 96))
    kern = profile_kernels(e, renderers, run_group, n_prof)
    one_stream[0] = False
    kernels = {}
    for name, k in kern.items():
        kernels[name] = k if name.startswith("_") else {"launches_timed": k["launches"], "avg_us": round(k["avg_us"], 3)}
    stream_gbps = stream_read_ceiling(e)
    roofline = None
    if "cull_meshlets_test" in kern:
        # 8 B MeshletInstance + 16 B MeshletBounds per meshlet + per-mesh tables 212/K B; the 4*v B of index writes are
        # done by cull_meshlets_emit and are NOT charged to this kernel (its ballots: 1/8 B per meshlet written)
        bytes_per_launch = n_meshlets * batch * (24.0 + 212.0 / K + 0.125)
        us = kern["cull_meshlets_test"]["avg_us"]
        achieved = bytes_per_launch / (us * 1e-6) / 1e9
        traffic, src, traffic_same = pmc_traffic([f"{t}_config2_pmc.json" for t in PROFILE_ROUNDS], lambda k: "k_cull_meshlets_test_batch" in k)
        roofline = {"bound": "hbm", "kernel": f"k_cull_meshlets_test_batch ({batch} frames per launch)", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic, "traffic_source": src, "traffic_profile_is_of_this_device_code": traffic_same,
                    "algorithmic_bytes_per_launch": round(bytes_per_launch),
                    "kernel_avg_us": round(us, 3), "launches_averaged": kern["cull_meshlets_test"]["launches"], "measured_stream_read_GBps": round(stream_gbps, 1),
                    "frac_of_measured_stream_read": round(achieved / stream_gbps, 4)}
        stage_bytes = n_meshlets * (24.0 + 212.0 / K + 4.0 * visible_fraction)
        batched["stage_frac"] = round(stage_bytes / (batched["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        single["stage_frac"] = round(stage_bytes / (single["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        single_unordered["stage_frac"] = round(stage_bytes / (single_unordered["ms_per_frame"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)

    cpu_baseline = None
    if with_cpu and rank == 0 and world == 1 and cpu_scene is not None:
        import oracle

        cores = usable_cores()
        cam = cpu_scene.cull_camera()
        t0 = time.perf_counter()
        oracle.cull_meshlets(cpu_scene, cam, cpu_scene.meshlet_instances, nthreads=1)
        dt1 = time.perf_counter() - t0
        cal = 8
        while True:  # grow the calibration run until thread start-up no longer dominates it
            tc = time.perf_counter()
            oracle.cull_meshlets(cpu_scene, cam, cpu_scene.meshlet_instances, nthreads=cores, passes=cal)
            t_cal = time.perf_counter() - tc
            if t_cal > 0.5 or cal >= 4096:
                break
            cal *= 4
        passes = int(min(max(1, args.cpu_seconds / (t_cal / cal)), 1_000_000))
        t0 = time.perf_counter()
        oracle.cull_meshlets(cpu_scene, cam, cpu_scene.meshlet_instances, nthreads=cores, passes=passes)
        dt = time.perf_counter() - t0
        cpu_baseline = {"value": round(n_meshlets * passes / dt, 1), "unit": "meshlets/s", "cores": cores, "kind": "port",
                        "sample": f"{passes} passes over the same {n_meshlets}-meshlet scene (copy 0), oracle/oxcull_oracle.c orc_cull_meshlets_mt_passes, "
                                  f"static range split over {cores} pthreads, {dt:.1f} s", "single_thread_value": round(n_meshlets / dt1, 1)}
    for rr in renderers[1:]:
        rr.close()
    return {
        "workload": "configs[1]: 1M meshlets, one camera, frustum + cone cull + ordered compaction (cull_meshlets stage)",
        "meshlets_per_gpu": n_meshlets, "mesh_instances": M, "copies_rotated": copies, "working_set_MB": round(copies * bytes_per_copy / 1e6, 1),
        "visible_fraction": round(visible_fraction, 4), "bit_match": bit_match, "batched": batched, "one_call_per_frame": single,
        "one_call_per_frame_unordered": single_unordered, "kernels": kernels,
        "roofline": roofline, "cpu_baseline": cpu_baseline,
    }


# ------------------------------------------------------------------------------------------------------------------
# configs[0]: ~1k entities, ECS transform update + host AABB frustum test (CPU only, the reference's own runnable case)
# ------------------------------------------------------------------------------------------------------------------
def measure_config1(args, seconds: float) -> dict:
    """BASELINE configs[0].  No GPU: the engine's coarse cull is host code (Scene.cpp:1690-1740 world-matrix chain through
    parents, BoundingVolume.cpp:32-53 AABB::get_transformed, :72-88 AABB::is_on_frustum against Camera::get_frustum,
    Camera.cpp:57-74).  The scalar C restatement (oracle/) IS the implementation measured here -- there is no HIP path for
    1 000 entities (one launch costs more than the whole update) -- so this line carries no roofline.  All-core figure: one
    independent 1 000-entity scene per host thread.  `seconds`: CPU time budget of the two timed runs together."""
    import threading

    import oracle
    from oxylus_amd.synth import camera_frustum_planes, make_entities

    oracle.build()
    n = args.entities
    trs, parent, aabb = make_entities(n, depth=3)
    planes = camera_frustum_planes([0.0, 2.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], 60.0, 16.0 / 9.0, 0.1, 1000.0)
    _, vis, nvis = oracle.entities_update_and_cull(trs, parent, aabb, planes)
    t0 = time.perf_counter()
    oracle.entities_update_and_cull(trs, parent, aabb, planes, passes=200)
    per_pass = (time.perf_counter() - t0) / 200
    passes = int(max(200, min(seconds / 2 / per_pass, 5_000_000)))
    t0 = time.perf_counter()
    oracle.entities_update_and_cull(trs, parent, aabb, planes, passes=passes)
    dt1 = time.perf_counter() - t0
    cores = usable_cores()
    threads = [threading.Thread(target=oracle.entities_update_and_cull, args=(trs.copy(), parent.copy(), aabb.copy(), planes), kwargs={"passes": passes}) for _ in range(cores)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dtn = time.perf_counter() - t0
    one, allc = n * passes / dt1, n * passes * cores / dtn
    return {
        "metric": "entities/s (ECS transform update + AABB frustum test, host)", "value": round(allc, 1), "unit": "entities/s", "n_gpus": 0, "steps": passes,
        "warmup": 200, "ms_per_step": round(dtn / passes * 1e3, 6), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"configs[0]: {n} entities in parent chains of depth 3: world = parent * T*R*S, world AABB = baked.get_transformed(world), "
                               "AABB::is_on_frustum against Camera::get_frustum (60 deg, 16:9, 0.1..1000)", "entities": n, "visible": nvis, "threads": cores,
                   "scenes_in_flight": cores},
        "single_thread_value": round(one, 1), "ms_per_update_one_thread": round(dt1 / passes * 1e3, 6), "roofline": None,
        "cpu_baseline": {"value": round(one, 1), "unit": "entities/s", "cores": 1, "kind": "port",
                         "sample": f"{passes} updates of the same {n}-entity scene, oracle/oxcull_oracle.c orc_entities_update_and_cull, one thread, {dt1:.1f} s"}}


def bench_config1(args):
    emit(measure_config1(args, args.cpu_seconds))


def line_summary(line: dict) -> dict:
    """The nested figures of the default line once more, compact, as its LAST key: the driver keeps the tail of stdout (round-4 review:
    the nested tris124 / configs1 / configs4 values were in no driver-held record)."""
    def g(d, *path, nd=None):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return round(d, nd) if (nd is not None and isinstance(d, float)) else d

    sm = {"ms_per_frame": g(line, "config", "ms_per_frame", nd=4), "stage_frac": g(line, "stage", "stage_frac"), "stage_frac_needed_bytes": g(line, "stage", "stage_frac_needed_bytes"),
          "roofline_frac": g(line, "roofline", "frac"), "bit_match": line.get("bit_match"), "hiz_bit_match": line.get("hiz_bit_match")}
    # what no oracle can pin (the reference is compiled fast-math): decisions that differ between the canonical checker and its fast-math-envelope build,
    # on the synthetic soup (whose backface determinants sit close to the 1e-4 threshold: a pessimistic proxy) and on the clusteriser-built real meshes
    def gap(u):
        return None if not isinstance(u, dict) else {"meshlets": u.get("visible_meshlets_differ"), "mask_bits": u.get("mask_bits_differ"), "triangles": u.get("triangles_differ"),
                                                     "of_triangles": u.get("triangles_emitted")}
    if line.get("unpinned_gap") or g(line, "real_geometry", "unpinned_gap"):
        sm["unpinned_gap"] = {"synthetic": gap(line.get("unpinned_gap")), "real_geometry": gap(g(line, "real_geometry", "unpinned_gap"))}
    kn = line.get("kernels") or {}
    sm["kernel_us"] = {k: round(v["avg_us"], 1) for k, v in kn.items() if isinstance(v, dict) and "avg_us" in v}
    if "hiz" in kn:
        sm["hiz"] = {k: kn["hiz"].get(k) for k in ("frac", "traffic", "traffic_over_algorithmic", "achieved_traffic_GBps")}
    for v in g(line, "scheduling_ab", "variants") or []:
        key = ("defaults_ms_per_frame" if v.get("library_defaults") else
               "ordered_shared_ms" if (v["unordered_output"] == 0 and v["share_pass_tests"] and not v["async_triangles"] and not v["hiz_one_frame_ahead_on_second_stream"]) else
               "unordered_unshared_ms" if (v["unordered_output"] == 1 and not v["share_pass_tests"] and not v["async_triangles"] and not v["hiz_one_frame_ahead_on_second_stream"]) else None)
        if key:
            sm[key] = round(v["ms_per_frame"], 4)
            sm.setdefault("variants_match", True)
            sm["variants_match"] = bool(sm["variants_match"] and v["outputs_match_main_line"])
    sh = g(line, "config", "sharding")
    if isinstance(sh, dict):  # N > 1
        sm["sharding"] = {"assignment": g(sh, "scene", "assignment") or "an independent scene per rank", "per_rank_visible": sh.get("per_rank_visible"),
                          "per_rank_ms_per_frame": sh.get("per_rank_ms_per_frame")}
        sm["sharding"]["rccl_ranks_seen"] = sh.get("rccl_ranks_seen")
        if "native_comm_ab" in line:
            nb = line["native_comm_ab"]
            sm["native_comm_ab"] = {k: (nb[k][:160] if isinstance(nb[k], str) else nb[k]) for k in ("path", "ms_per_frame", "outputs_match_main_line", "rccl_ranks_seen", "error", "skipped", "timed_out_s") if k in nb}
        if "assignment_ab" in line:
            ab = line["assignment_ab"]
            sm["sharding"]["other_assignment"] = {k: ab[k] for k in ("assignment", "value", "ms_per_frame", "per_rank_visible")}
    if "tris124" in line:
        sm["tris124"] = {"meshlets": g(line, "tris124", "meshlets"), "index": "pairs" if "pairs" in (g(line, "tris124", "index_form") or "") else "wide9",
                         "ms_per_frame": g(line, "tris124", "ms_per_frame", nd=4), "frac": g(line, "tris124", "roofline", "frac"), "stage_frac": g(line, "tris124", "stage", "stage_frac"),
                         "traffic": g(line, "tris124", "roofline", "traffic"), "bit_match": g(line, "tris124", "bit_match")}
    if "configs1" in line:
        c1 = line["configs1"]
        sm["configs1"] = {"batched_frac": g(c1, "roofline", "frac"), "batched_stage_frac": g(c1, "batched", "stage_frac"), "value": g(c1, "batched", "value"),
                          "one_call_us": round(1e3 * c1["one_call_per_frame_unordered"]["ms_per_frame"], 2), "one_call_frac": g(c1, "one_call_per_frame_unordered", "stage_frac"),
                          "one_call_launches": g(c1, "one_call_per_frame_unordered", "launches_per_call"),
                          "bit_match": bool(c1.get("bit_match") and c1["one_call_per_frame_unordered"].get("sorted_list_equals_the_checkers"))}
    if "configs4" in line:
        c4 = line["configs4"]
        sm["configs4"] = {"ms_per_step": g(c4, "ms_per_step", nd=4), "value": g(c4, "value"), "frac": g(c4, "roofline", "frac"), "stage_frac": g(c4, "stage", "stage_frac"),
                          "lists": g(c4, "config", "meshlet_instance_lists"), "implicit_lists_ms_per_step": g(c4, "implicit_lists_variant", "ms_per_step", nd=4),
                          "implicit_lists_match": g(c4, "implicit_lists_variant", "outputs_match_main_line"), "bit_match": c4.get("bit_match")}
    if "configs0" in line:
        sm["configs0"] = {"entities_per_s": g(line, "configs0", "value"), "cores": g(line, "configs0", "config", "threads"), "one_core": g(line, "configs0", "single_thread_value"),
                          "ms_per_update_one_thread": g(line, "configs0", "ms_per_update_one_thread")}
    if "real_geometry" in line:
        sm["real_geometry"] = {"ms_per_frame": g(line, "real_geometry", "ms_per_frame", nd=4), "bit_match": g(line, "real_geometry", "bit_match"),
                               "visible_fraction": g(line, "real_geometry", "visible_fraction"), "tri_kernel_frac_requested_bytes": g(line, "real_geometry", "roofline", "frac"),
                               "tri_kernel_us": g(line, "real_geometry", "roofline", "kernel_avg_us"), "traffic": g(line, "real_geometry", "roofline", "traffic")}
    return sm


def main():
    args = parse()
    if args.dump_outputs and args.workload != "config3":
        raise SystemExit(f"bench.py: --dump-outputs writes the outputs of the default workload (config3), not of --workload {args.workload}")
    if args.workload == "config1":
        return bench_config1(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args)
    e = setup(args)
    if args.workload in ("bounds", "loop", "vsm", "config5"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_aux

        fn = {"bounds": bench_aux.bench_bounds, "loop": bench_aux.bench_loop, "vsm": bench_aux.bench_vsm, "config5": bench_aux.bench_config5}[args.workload]
        if args.steps == 20 and args.warmup == 5:  # these workloads cap their own step counts; keep the old defaults
            args.steps, args.warmup = 50, 5
        return fn(args, e.r, e.dev, e.stream, e.rank, e.world, e.dist)
    if args.workload == "config2":
        res = bench_config2(args, e, args.steps, args.warmup, with_cpu=not args.no_cpu_baseline)
        if e.rank == 0:
            b = res["batched"]
            emit({
                "metric": "meshlets/s culled", "value": b["value"], "unit": "meshlets/s", "n_gpus": e.world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(b["seconds"] * 1e3 / args.steps, 6), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                "data": "synthetic", "config": {"workload": res["workload"], "inner_reps": b["frames_timed"] // args.steps, **{k: res[k] for k in
                                                ("meshlets_per_gpu", "mesh_instances", "copies_rotated", "working_set_MB", "visible_fraction")},
                                                "frames_per_launch": b["frames_per_launch"], "streams": b["streams"]},
                "bit_match": res["bit_match"], "batched": b, "one_call_per_frame": res["one_call_per_frame"], "one_call_per_frame_unordered": res["one_call_per_frame_unordered"],
                "kernels": res["kernels"], "roofline": res["roofline"],
                "cpu_baseline": res["cpu_baseline"]})
    else:
        def stage_note(what):  # progress on stderr: which part of the default line is running (a fault names no kernel)
            if e.rank == 0:
                print(f"[bench] {what}", file=sys.stderr, flush=True)

        stage_note("configs[2] main line")
        line = bench_config3(args, e)
        if args.full and e.world > 1 and not args.independent_scenes and not args.no_assignment_ab:
            # the OTHER assignment of the same scene, a short run: contiguous instance ranges (the north star's wording; depth slabs of this
            # synthetic scene, i.e. skewed) beside the interleaved blocks of the main line, or the reverse -- per_rank_visible tells them apart
            import copy

            a3 = copy.copy(args)
            a3.shard_block = 0 if args.shard_block > 0 else 64
            a3.steps, a3.warmup, a3.dump_outputs = max(2, args.steps // 4), 1, None
            a3.no_scheduling_ab, a3.no_cpu_baseline, a3.no_exchange_ab, a3.no_native_comm_ab, a3.cpu_prefix = True, True, True, True, min(args.cpu_prefix, 100)
            stage_note("assignment_ab")
            t = bench_config3(a3, e)
            if e.rank == 0:
                sh = t["config"]["sharding"]
                line["assignment_ab"] = {"assignment": sh["scene"]["assignment"], "value": t["value"], "ms_per_frame": t["config"]["ms_per_frame"], "frames_timed": t["config"]["frames_timed"],
                                         "per_rank_visible": sh["per_rank_visible"], "per_rank_ms_per_frame": sh["per_rank_ms_per_frame"], "bit_match": t["bit_match"]}
        if args.full and e.world == 1 and not args.no_tris124 and args.tris == 64 and not args.meshlets:
            # BASELINE's stated meshlet shape -- 64 vertices / 124 triangles -- does not fit the reference's 24 + 8 bit packed index: the same
            # frame at the literal 10 M meshlets with the pair form (wide_triangle_index = 2: {u32 id, u32 corner}, 24 B per emitted triangle, two
            # 64-lane triangle passes), a short run.  (`--tris 124 --index-form wide` is round 5's (id << 9) | corner form: at most 2^23 ids, 8 M meshlets.)
            import copy

            a2 = copy.copy(args)
            a2.tris, a2.steps, a2.warmup, a2.index_form, a2.dump_outputs = 124, max(4, args.steps // 4), 1, "pairs", None
            a2.no_scheduling_ab, a2.no_cpu_baseline, a2.cpu_prefix = True, True, min(args.cpu_prefix, 250)
            stage_note("tris124")
            t = bench_config3(a2, e)
            line["tris124"] = {"workload": "the configs[2] frame with 64 vertices / 124 triangles per meshlet (BASELINE's stated shape): wide_triangle_index = 2, "
                                           f"{{u32 id, u32 corner}} pairs, {t['config']['meshlets_per_gpu']} meshlets, 4096^2 HiZ", "value": t["value"], "unit": "meshlets/s",
                               "ms_per_frame": t["config"]["ms_per_frame"], "frames_timed": t["config"]["frames_timed"], "index_form": t["config"]["index_form"],
                               "meshlets": t["config"]["meshlets_per_gpu"],
                               "visible_fraction": t["config"]["visible_fraction"], "triangles_per_visible_meshlet": t["config"]["triangles_per_visible_meshlet"],
                               "bit_match": t["bit_match"], "bit_match_detail": t["bit_match_detail"], "bit_match_sample": t["bit_match_sample"], "counts": t["counts"], "roofline": t["roofline"], "stage": t["stage"],
                               "kernels": {k: v for k, v in t["kernels"].items() if k.startswith("cull_triangles") or k.startswith("_")}}
        if args.full and e.world == 1 and not args.no_configs1:
            stage_note("configs1")
            line["configs1"] = bench_config2(args, e, steps=8, warmup=1, with_cpu=not args.no_cpu_baseline)
        if args.full and e.world == 1 and not args.no_configs4:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_aux

            stage_note("configs4")
            line["configs4"] = bench_aux.bench_config5(args, e.r, e.dev, e.stream, e.rank, e.world, e.dist, nested=True)
        if args.full and e.world == 1 and not args.no_real_geometry:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_aux

            stage_note("real_geometry")
            line["real_geometry"] = bench_aux.bench_real_geometry(args, e.r, e.dev, e.stream, e.rank)
        if args.full and e.world == 1 and not args.no_configs0:
            stage_note("configs0")
            line["configs0"] = measure_config1(args, min(args.cpu_seconds, 2.0))  # BASELINE configs[0]: CPU only by definition, milliseconds per update
        if e.rank == 0:
            line["summary"] = line_summary(line)
            emit(line)  # full record -> gpurun_out/bench_full.json; stdout: ONE compact line (<= 4 KB) the driver parses
    if e.dist is not None:
        e.dist.destroy_process_group()
    e.r.close()


if __name__ == "__main__":
    main()
