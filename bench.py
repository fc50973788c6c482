#!/usr/bin/env python
"""bench.py — ICP frames/sec of the MI355X registration hot path (BASELINE.json metric).

A "step" is one sage_icp::RegisterFrame() call run to convergence (the span the reference times,
pipeline/sageICP.cpp:79-88) on one synthetic labelled scan, with the scan and the replicated map
already resident in HBM when the timed region starts.

  N = 1   workload c2: 120,000-pt scan vs 1,000,000-pt semantic voxel map, identity initial guess,
          reference start-up parameters (sigma = 2.0 -> max_corr 6.0, kernel 2/3, sem_th 0.4).
  N > 1   the SAME frame, query-sharded in contiguous blocks over the N ranks (one process per
          GPU), map replicated, the 17 Gauss-Newton sums exchanged over xGMI each iteration
          -> strong scaling.  (--workload c4 runs the 500k-vs-10M multi-GPU config;
          --independent gives every rank a whole frame instead: throughput, weak scaling.)
          `python bench.py --gpus N` launches its own ranks (torch.distributed.run) when it was
          not started under a launcher.

Prints ONE JSON line on rank 0 (see the task contract), including
  roofline      the search + accumulation kernel (k_icp).  `achieved` / `frac` are what rocprofv3 shows
                for it — FETCH_SIZE x 2 per launch / kernel-trace duration / 8 TB/s (`frac_basis` says
                so) — whenever profiles/icp_counters.json holds counters taken on exactly the device
                code that runs; `traffic_floor_us` (that traffic at the achievable 6.3 TB/s) and
                `x_over_traffic_floor` put the kernel's distance from its own traffic in one number.
                Beside them, named for what they are: `executed_bytes_frac` (SURVEY.md 8d's compact
                records for the pairs the kernel actually evaluates / HIP-event duration: mostly cache
                traffic, not an HBM fraction) and `effective_gather_gbs` (8d's contractual figure with
                every candidate of the 27 voxels charged: what the reference scans).  Without fresh
                counters `frac` falls back to the executed-bytes figure and `frac_basis` says that.
  cpu_baseline  the CPU oracle (a structure-faithful port of the reference path, OpenMP) timed on a
                bounded sample of the same frame: warm-up, thread sweep, median of 5 at the fastest
                count, and the 1-thread time; rank 0 at N = 1 only.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
HBM_ACHIEVABLE_GBS = 6300.0   # same guide: what a streaming kernel reaches


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c2", choices=["c1", "c2", "c4", "c5"])
    ap.add_argument("--params", default=None, choices=["cold", "steady", "dense", "dense_nosem"],
                    help="default: cold (c1, c2), steady (c4: SURVEY 8d), dense (c5)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workload (debug only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--independent", action="store_true",
                    help="N > 1: every rank registers a WHOLE frame against its own copy of the map "
                         "(one stream per GPU, no exchange): the throughput curve of BASELINE config 5; "
                         "value = frames of all ranks per second, scaling weak")
    ap.add_argument("--cpu-seconds", type=float, default=12.0,
                    help="CPU time budget of the cpu_baseline sample")
    ap.add_argument("--exchange", default="auto", choices=["auto", "direct", "rccl"],
                    help="N > 1, query-sharded: how the ranks' Gauss-Newton sums meet — 'direct' (stores over xGMI into HIP-IPC "
                         "mapped blocks, inside the solving wave / k_fin), 'rccl' (ncclAllReduce between two k_fin launches), "
                         "'auto' (direct when every rank can set it up and it passes its cross-check against RCCL, else RCCL)")
    ap.add_argument("--no-profile-events", action="store_true",
                    help="do not record per-kernel HIP events in the timed region")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="rank 0 writes what the last timed step returned as DIR/<name>.npy (float64): pose, stats, "
                         "n_corr_hist — for comparing two builds output for output (the inputs are seeded)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def dump_outputs(d, pose, st):
    """What the caller of the timed entry receives (sageicp_register_frame_resident): the pose and the
    statistics that describe the computation — the wall-clock fields of the statistics are left out."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "pose.npy"), np.asarray(pose, dtype=np.float64))        # qx qy qz qw tx ty tz
    np.save(os.path.join(d, "stats.npy"), np.array(
        [st.iterations, st.converged, st.n_queries, st.n_corr_first, st.n_corr_last, st.last_step_norm],
        dtype=np.float64))
    np.save(os.path.join(d, "n_corr_hist.npy"), np.array(st.n_corr_hist[:], dtype=np.float64))


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


def device_source_hash():
    """sha256 over what the profiler counters describe (profiles/collect.py): every source and header of the
    library and the build recipe with its flags"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "sage-icp_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    for f in (os.path.join(ROOT, "sage-icp_amd", "build.py"), os.path.join(ROOT, "include", "sageicp.h")):
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def apply_counters(roofline, c, source_hash, one_launch, compulsory, executed_bytes):
    """`achieved` / `frac` / `traffic` of the roofline object from an entry of profiles/icp_counters.json — only when
    the entry was collected on exactly this build (`source_hash`) and on the form of the loop that ran; otherwise
    they stay null and `frac_basis` says why (tests/test_abi_and_host.py feeds a wrong hash)."""
    want = "k_loop" if one_launch else "k_icp"
    if not c:
        return roofline
    if c.get("source_sha256") != source_hash:
        roofline["frac_basis"] = ("none: profiles/icp_counters.json was collected on another build of the library "
                                  "(re-run profiles/run_profiles.sh + profiles/collect.py)")
        return roofline
    if c.get("kernel") != want:
        roofline["frac_basis"] = "none: profiles/icp_counters.json describes %s, this run went through %s" % (c.get("kernel"), want)
        return roofline
    if not c.get("hbm_bytes_per_launch"):
        return roofline
    kt_us = c["avg_launch_us_kernel_trace"]
    roofline["counters_fresh"] = True
    roofline["counters"] = c.get("counters_source")
    roofline["traffic"] = c["hbm_bytes_per_launch"]
    roofline["achieved"] = round(roofline["traffic"] / (kt_us * 1e-6) / 1e9, 1)
    roofline["frac"] = round(roofline["achieved"] / HBM_PEAK_GBS, 4)
    roofline["frac_basis"] = ("rocprofv3 FETCH_SIZE x 2 per iteration / kernel-trace duration per iteration / 8 TB/s ("
                              + str(c.get("counters_source", "")).split(" (")[0] + ")")
    floor_us = roofline["traffic"] / (HBM_ACHIEVABLE_GBS * 1e9) * 1e6
    roofline["traffic_floor_us"] = round(floor_us, 2)
    roofline["x_over_traffic_floor"] = round(kt_us / floor_us, 2)
    roofline["traffic_over_compulsory"] = round(roofline["traffic"] / compulsory, 3)
    roofline["traffic_over_algorithmic"] = round(roofline["traffic"] / executed_bytes, 3)
    for key in ("avg_launch_us_kernel_trace", "valu_frac", "useful_inst_frac", "valu_insts_per_launch",
                "lane_utilization", "l2_hit_rate", "wait_frac"):
        if key in c:
            roofline[key] = c[key]
    return roofline


def cpu_quota():
    """The container's CPU quota in cores (cgroup v2 cpu.max / v1 cfs quota), or None."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(int(q) / int(p), 2)
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else round(q / p, 2)
    except Exception:
        return None


def cpu_baseline(args, w, wl, prm, scan, iters, fps, gpu_pose, gpu_stats):
    """The oracle (structure-faithful CPU port) on the same frame: reproducible protocol.
    Returns (cpu_baseline, parity): the second is the oracle's FULL registration of the frame the
    timed region registered, compared with the pose and counts the timed region produced."""
    import numpy as np
    import oracle                              # the checker / CPU port, timed as a baseline
    om = oracle.Map(wl["voxel"], 100.0)
    om.add_points(w["stream"])
    avail = oracle.num_threads()

    def run(nt, k):
        t = time.perf_counter()
        _, ost = om.register_frame(scan, oracle.IDENTITY, prm["max_dist"], prm["kernel"], prm["sem_th"],
                                   nthreads=nt, max_iter=k)
        return (time.perf_counter() - t) / max(ost.iterations, 1), ost

    run(min(avail, 32), 2)                                         # page in, spin up the pool
    t1, _ = run(1, 1)                                              # one thread, one iteration
    # the port does not scale to every hardware thread of the box (memory-bound hash walks), and a
    # container with a CPU quota lets a short burst run wider than it can sustain: sweep a few
    # thread counts for at least 0.6 s each (several scheduler periods) and keep the fastest as
    # THE baseline
    sweep = {}
    for nt in sorted({min(avail, c) for c in (8, 16, 32, 64, 128, avail)}):
        run(nt, 1)
        t0, its, spent = time.perf_counter(), 0, 0.0
        while time.perf_counter() - t0 < 0.6:
            v, _ = run(nt, 3)
            spent += 3 * v
            its += 3
        sweep[nt] = spent / its
    threads = min(sweep, key=sweep.get)
    # median of 5 repetitions at that count, K iterations each, within the time budget
    k = int(max(3, min(iters, args.cpu_seconds / 5.0 / max(sweep[threads], 1e-9))))
    reps, ost = [], None
    for _ in range(5):
        v, ost = run(threads, k)
        reps.append(v)
    reps.sort()
    per_iter = reps[2]
    cpu_fps = 1.0 / (per_iter * iters)
    # parity of the headline workload itself: the oracle registers the whole frame once (every
    # iteration, to convergence) and is compared with what the timed region returned
    if per_iter * iters > 60.0:
        # c4: minutes of oracle time.  The oracle's full registration of exactly this frame was run once in the
        # build container (tests/golden/make_c4_golden.py -> tests/golden/c4_full.npz: data only); the timed
        # region's pose and counts are compared with that fixture instead.
        return _cpu_dict(locals(), None), parity_from_fixture(args, w, scan, gpu_pose, gpu_stats, per_iter * iters)
    t = time.perf_counter()
    opose, ofull = om.register_frame(scan, oracle.IDENTITY, prm["max_dist"], prm["kernel"], prm["sem_th"],
                                     nthreads=threads)
    t_full = time.perf_counter() - t
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(opose), np.asarray(gpu_pose, dtype=np.float64)))
    parity = {"against": "oracle (CPU restatement of the reference path; parity unpinned by the reference, "
                         "DESIGN.md section 5), full registration of the frame of the timed region",
              "pose_delta_m": float("%.3e" % np.linalg.norm(e[:3])),
              "pose_delta_rad": float("%.3e" % np.linalg.norm(e[3:])),
              "tolerance": {"m": 1e-4, "rad": 1e-4},
              "iterations": [int(gpu_stats.iterations), int(ofull.iterations)],
              "iterations_equal": bool(gpu_stats.iterations == ofull.iterations),
              "n_corr_first_last": [[int(gpu_stats.n_corr_first), int(gpu_stats.n_corr_last)],
                                    [int(ofull.n_corr_first), int(ofull.n_corr_last)]],
              "n_corr_equal": bool(gpu_stats.n_corr_first == ofull.n_corr_first and
                                   gpu_stats.n_corr_last == ofull.n_corr_last),
              "candidates_equal": bool(gpu_stats.sum_candidates == ofull.sum_candidates_total),
              "oracle_seconds": round(t_full, 2),
              "ok": bool(np.linalg.norm(e[:3]) < 1e-4 and np.linalg.norm(e[3:]) < 1e-4 and
                         gpu_stats.iterations == ofull.iterations)}
    return _cpu_dict(locals(), 1.0 / t_full), parity


def parity_from_fixture(args, w, scan, gpu_pose, gpu_stats, oracle_seconds_estimate):
    import numpy as np
    import oracle
    path = os.path.join(ROOT, "tests", "golden", "c4_full.npz")
    params = args.params or "steady"
    why = None
    if args.workload != "c4" or args.scale != 1.0 or not os.path.exists(path):
        why = "no committed fixture for this workload"
    else:
        g = np.load(path)
        same = (params + "_pose" in g and [int(x) for x in g["map_size"]][0] == w["map"].size() and
                np.array_equal(g["scan_checksum"], [float(np.sum(scan[:, :3])), float(np.sum(scan[:, 3]))]))
        if not same:
            why = "the committed fixture is not of this frame"
    if why:
        return {"skipped": "the oracle needs ~%.0f s for this frame and %s; parity of this workload is checked in "
                           "tests/test_gpu_parity.py" % (oracle_seconds_estimate, why)}
    iters, conv, nc_first, nc_last, sum_cq, _ = [int(x) for x in g[params + "_counts"]]
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(g[params + "_pose"]), np.asarray(gpu_pose, dtype=np.float64)))
    return {"against": "tests/golden/c4_full.npz: the oracle's full registration of this frame, run once in the build "
                       "container (make_c4_golden.py; the oracle: CPU restatement of the reference path, parity unpinned "
                       "by the reference, DESIGN.md section 5)",
            "pose_delta_m": float("%.3e" % np.linalg.norm(e[:3])),
            "pose_delta_rad": float("%.3e" % np.linalg.norm(e[3:])),
            "tolerance": {"m": 1e-4, "rad": 1e-4},
            "iterations": [int(gpu_stats.iterations), iters],
            "iterations_equal": bool(gpu_stats.iterations == iters),
            "n_corr_first_last": [[int(gpu_stats.n_corr_first), int(gpu_stats.n_corr_last)], [nc_first, nc_last]],
            "n_corr_equal": bool(gpu_stats.n_corr_first == nc_first and gpu_stats.n_corr_last == nc_last),
            "candidates_equal": bool(gpu_stats.sum_candidates == sum_cq),
            "oracle_seconds": None,
            "ok": bool(np.linalg.norm(e[:3]) < 1e-4 and np.linalg.norm(e[3:]) < 1e-4 and gpu_stats.iterations == iters)}


def _cpu_dict(v, cpu_fps_full):
    cpu_fps, reps, sweep, threads = v["cpu_fps"], v["reps"], v["sweep"], v["threads"]
    args, iters, scan, ost = v["args"], v["iters"], v["scan"], v["ost"]
    return {"value": round(cpu_fps, 5), "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": "median of 5 runs of the first %d of %d ICP iterations of the same %s frame "
                      "(%d queries) on %d OpenMP threads (OMP_PROC_BIND=close, OMP_PLACES=cores) after "
                      "a warm-up; per-iteration cost is constant, scaled to the %d iterations the "
                      "frame takes" % (v["k"], iters, args.workload, len(scan), threads, iters),
            "seconds_per_iteration": round(v["per_iter"], 5),
            "seconds_per_iteration_runs": [round(x, 5) for x in reps],
            "seconds_per_iteration_1_thread": round(v["t1"], 4),
            "frames_per_second_1_thread": round(1.0 / (v["t1"] * iters), 6),
            "threads_available": v["avail"], "cpu_quota": cpu_quota(),
            "seconds_per_iteration_by_threads": {str(a): round(b, 5) for a, b in sorted(sweep.items())},
            "sweep_vs_reported": round(sweep[threads] / v["per_iter"], 3),
            "candidates_per_query": round(ost.sum_candidates_total / max(ost.iterations, 1) / len(scan), 1),
            "frames_per_second_whole_frame_once": None if cpu_fps_full is None else round(cpu_fps_full, 5),
            "speedup_gpu_over_cpu": round(v["fps"] / cpu_fps, 1),
            "speedup_note": "GPU frames/s / CPU frames/s, the CPU figure extrapolated from the sampled "
                            "iterations to the frame's iteration count (frames_per_second_whole_frame_once: "
                            "one un-sampled run of the whole frame, for comparison)"}


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    # the CPU baseline's OpenMP pool: pinned, one thread per core (read when libgomp starts)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    # RCCL prints a version banner on stdout when a communicator is created; the contract is ONE
    # JSON line on stdout, so everything before the final print goes to stderr.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))

    import numpy as np
    import torch   # device sync + torch.distributed rendezvous only; the hot path is the C ABI
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False")
    # SAGEICP_BENCH_DEVICE / SAGEICP_BENCH_BACKEND=gloo: put several ranks on ONE GPU without RCCL —
    # only to exercise the direct exchange between processes on a 1-GPU box
    local_dev = int(os.environ.get("SAGEICP_BENCH_DEVICE", local_rank))
    backend = os.environ.get("SAGEICP_BENCH_BACKEND", "nccl")
    if "SAGEICP_BENCH_DEVICE" in os.environ and world > 1:
        # the ranks share ONE GPU: each runs on its own part of the CUs (CU-masked streams, capi_internal.h), so that the
        # persistent grids of their one-launch loops are resident side by side instead of waiting for each other
        os.environ.setdefault("SAGEICP_CU_SHARE", "%d/%d" % (rank, world))
    torch.cuda.set_device(local_dev)
    # SAGEICP_FORCE_COMM=1 runs the multi-GPU code path (process group, RCCL communicator, in-stream
    # all-reduce) even with one rank, so it can be exercised on a 1-GPU box under torchrun.
    force_comm = os.environ.get("SAGEICP_FORCE_COMM", "0") == "1" and "RANK" in os.environ
    use_dist = world > 1 or force_comm
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", world_size=world, rank=rank,
                                    device_id=torch.device("cuda", local_dev))
        else:
            dist.init_process_group(backend=backend, world_size=world, rank=rank)
    red_dev = "cuda" if backend == "nccl" else "cpu"      # where the bench's own reductions live

    # the .so is a build artefact (git-ignored): build it in-tree if a fresh checkout has none
    if local_rank == 0 and not os.path.exists(os.path.join(ROOT, "sage-icp_amd", "libsageicp_hip.so")):
        import importlib.util
        spec = importlib.util.spec_from_file_location(
            "_sageicp_build", os.path.join(ROOT, "sage-icp_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    if use_dist:
        dist.barrier()
    import sage_icp_amd as sage
    from sage_icp_amd import synthetic as syn
    from sage_icp_amd.sharding import shard_bounds

    if sage.device_count() <= local_dev:
        raise SystemExit("HIP device %d not visible to libsageicp_hip.so" % local_dev)

    wl = syn.WORKLOADS[args.workload]
    if args.params is None:
        args.params = {"c5": "dense", "c4": "steady"}.get(args.workload, "cold")
    prm = syn.PARAMS[args.params]
    t_gen = time.time()
    w = syn.make_workload(args.workload,
                          lambda: sage.VoxelHashMap(wl["voxel"], 100.0, device=local_dev),
                          scale=args.scale)
    vmap, scan = w["map"], w["scan"]
    vmap.sync()                                    # map mirror resident before the timed region
    lo, hi = (0, len(scan)) if args.independent else shard_bounds(len(scan), rank, world)
    frame = sage.Frame(vmap, scan[lo:hi])          # this rank's block of the scan, resident in HBM
    t_gen = time.time() - t_gen

    comm = None
    exchange = "none"
    have_rccl = False
    use_p2p = False          # this run's choice (a failed exchange disables it inside the library)

    def all_agree(flag):
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    RCCL_TEXT = "RCCL all-reduce of 20 fp64 sums over %d ranks + solve launch" % world

    if use_dist and args.independent:
        exchange = "none: independent frames, one per rank"
    elif use_dist:
        have_rccl = backend == "nccl" and os.environ.get("SAGEICP_NO_RCCL", "0") != "1" and args.exchange != "direct"
        if have_rccl:
            ids = [sage.Comm.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ids, src=0)
            comm = sage.Comm(ids[0], rank, world, local_dev)
            exchange = RCCL_TEXT
        else:
            comm = sage.Comm(None, rank, world, local_dev)
        # Direct exchange over xGMI (HIP IPC): preferred when every rank can set it up, RCCL
        # otherwise (SAGEICP_NO_P2P=1 forces RCCL).
        if args.exchange == "rccl" and not have_rccl:
            raise SystemExit("--exchange rccl: no RCCL side (backend %s)" % backend)
        if os.environ.get("SAGEICP_NO_P2P", "0") != "1" and args.exchange != "rccl" and world <= 8:
            try:
                mine = comm.p2p_export()
            except Exception as e:                  # noqa
                sys.stderr.write("rank %d: p2p export failed: %s\n" % (rank, e))
                mine = b""
            handles = [None] * world
            dist.all_gather_object(handles, mine)
            ok = all(h is not None and len(h) == sage.P2P_HANDLE_BYTES for h in handles)
            if ok:
                try:
                    comm.p2p_connect(handles)
                except Exception as e:              # noqa
                    sys.stderr.write("rank %d: p2p connect failed: %s\n" % (rank, e))
                    ok = False
            use_p2p = all_agree(ok)
            if not use_p2p and comm.p2p_enabled:
                comm.p2p_enable(False)
        if use_p2p:
            exchange = "direct exchange of 20 fp64 sums over xGMI between %d ranks (HIP IPC), solved in k_fin" % world
        elif not have_rccl:
            raise SystemExit("no exchange path: RCCL disabled and the direct exchange unavailable")

    def step():
        return sage.register_frame(frame, vmap, sage.IDENTITY, prm["max_dist"], prm["kernel"],
                                   prm["sem_th"], comm=comm, return_stats=True)

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def warm():
        try:
            for _ in range(args.warmup):
                step()
            return True
        except sage.SageIcpError as e:
            sys.stderr.write("rank %d: warm-up failed: %s\n" % (rank, e))
            return False

    def fall_back(why):
        """every rank leaves the direct exchange for RCCL together"""
        nonlocal use_p2p, exchange
        if not have_rccl:
            raise SystemExit("direct exchange failed and there is no RCCL side to fall back to")
        if comm.p2p_enabled:
            comm.p2p_enable(False)
        use_p2p = False
        exchange = RCCL_TEXT + " (" + why + ")"

    fence()          # every rank has its map and frame in HBM before the first exchange is waited for
    cross_check = None
    if use_dist and use_p2p and have_rccl:
        # cross-check before trusting the direct exchange on this node: the same frame through
        # RCCL and through the mapped blocks must give the same pose (the summation order over
        # the ranks differs, nothing else)
        try:
            comm.p2p_enable(False)
            pose_rccl, _ = step()
            comm.p2p_enable(True)
            pose_p2p, _ = step()
            same = bool(np.allclose(pose_rccl, pose_p2p, rtol=0.0, atol=1e-6))
            cross_check = {"pose_rccl_vs_direct_max_abs": float("%.3e" % np.max(np.abs(pose_rccl - pose_p2p))),
                           "same_within_1e-6": same}
        except sage.SageIcpError as e:
            sys.stderr.write("rank %d: exchange cross-check failed: %s\n" % (rank, e))
            same = False
            cross_check = {"error": str(e), "same_within_1e-6": False}
        if not all_agree(same):
            fall_back("direct exchange failed its cross-check")
    ok = warm()
    if use_dist and use_p2p and not all_agree(ok):
        fall_back("direct exchange failed")
        ok = warm()
    if not ok:
        raise SystemExit("warm-up failed")

    # level 1: HIP events around k_icp in one iteration out of 8 of the timed region (bracketing
    # every launch costs several % of the frame rate this line reports)
    def timed():
        """EXACTLY args.steps steps between two fences; None if a step failed on this rank"""
        sage.set_profiling(0 if args.no_profile_events else 1)
        # the per-wave counters behind sum_candidates / pairs_evaluated (the bytes models of the line) are
        # instrumentation the C++ shim's calls never pay for: off in the timed region, one counted frame after it
        sage.set_counting(False)
        try:
            fence()
            t0 = time.perf_counter()
            stats, pose, good = [], None, True
            try:
                for _ in range(args.steps):
                    pose, st = step()
                    stats.append(st)
            except sage.SageIcpError as e:
                sys.stderr.write("rank %d: timed step failed: %s\n" % (rank, e))
                good = False
            fence()
            elapsed = time.perf_counter() - t0
        finally:                               # (whatever happens in there: the process-wide switches go back)
            sage.set_profiling(0)
            sage.set_counting(True)
        return (elapsed, stats, pose) if good else None

    res = timed()
    if use_dist and not all_agree(res is not None):
        # an exchange failed in the timed region: every rank switches to RCCL and times again
        if not use_p2p:
            raise SystemExit("a timed step failed")
        fall_back("direct exchange failed")
        if not all_agree(warm()):
            raise SystemExit("warm-up failed after the fallback to RCCL")
        res = timed()
        if not all_agree(res is not None):
            raise SystemExit("a timed step failed")
    if res is None:
        raise SystemExit("a timed step failed")
    elapsed, stats, pose = res
    if use_dist:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    # Where an iteration of the sharded loop goes (not in the timed region: bracketing every kernel
    # costs stream time): one more frame on every rank with HIP events around each launch — the
    # search of this rank's shard, and the finish (reduction, exchange with the peers, solve).
    # the same frame once more with the counters on: C_q and the pairs evaluated, per iteration (every rank:
    # under a communicator the call is collective)
    fence()
    try:
        _, counted = step()
    except sage.SageIcpError as e:
        raise SystemExit("the counted frame after the timed region failed: %s" % e)
    fence()

    breakdown = None
    if use_dist and not args.independent:
        loop_env = os.environ.get("SAGEICP_LOOP")
        sage.set_profiling(2)
        try:
            fence()
            _, sb = step()
            fence()
            breakdown = {"loop_form": "one launch for the whole loop (k_loop + its solving wave, the exchange inside)"
                                      if sb.single_launch else "k_icp + k_fin per iteration",
                         "lanes_per_query": sb.lanes_per_query}
            if sb.nn_launches and sb.single_launch:
                breakdown["iteration_us"] = round(sb.us_nn / sb.nn_launches, 2)
                # the same frame through the launch-per-iteration loop, whose two launches can be told apart
                os.environ["SAGEICP_LOOP"] = "0"
                fence()
                _, sb = step()
                fence()
            if sb.nn_launches and not sb.single_launch:
                breakdown["launch_per_iteration"] = {
                    "shard_compute_us_per_iteration": round(sb.us_nn / sb.nn_launches, 2),
                    "exchange_us_per_iteration": round(sb.us_fin / sb.nn_launches, 2),
                    "note": "rank 0, one frame after the timed region, HIP events around every launch: "
                            "k_icp on this rank's shard | k_fin incl. the wait for the peers' sums (direct "
                            "exchange) or k_fin + ncclAllReduce + k_fin (RCCL); on one GPU k_fin takes ~6 us"}
        except sage.SageIcpError as e:
            sys.stderr.write("rank %d: breakdown frame failed: %s\n" % (rank, e))
        finally:
            if loop_env is None:
                os.environ.pop("SAGEICP_LOOP", None)
            else:
                os.environ["SAGEICP_LOOP"] = loop_env
            sage.set_profiling(0)

    # what every rank ran, for the line: the form of the loop in the timed frames and what its map handle says about fall-backs
    ls = vmap.loop_status()
    mine = {"rank": rank,
            "loop_form": "one launch" if all(st.single_launch for st in stats) else
                         ("launch per iteration" if not any(st.single_launch for st in stats) else "mixed"),
            "lanes_per_query": int(stats[-1].lanes_per_query), "queries": int(hi - lo),
            "calls_single_launch": int(ls.calls_single_launch), "calls_per_iteration": int(ls.calls_per_iteration),
            "calls_chained": int(ls.calls_chained),
            "loop_timeouts": int(ls.timeouts), "last_fallback": int(ls.last_fallback)}
    per_rank = [mine]
    if use_dist:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)

    if rank != 0:
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, pose, stats[-1])

    # the host-buffer entry the C++ shim calls (frame uploaded inside the call), not the headline
    host_entry_ms = None
    if world == 1:
        sage.register_frame(scan, vmap, sage.IDENTITY, prm["max_dist"], prm["kernel"], prm["sem_th"])
        t0 = time.perf_counter()
        k_host = max(3, min(args.steps, 10))
        for _ in range(k_host):
            sage.register_frame(scan, vmap, sage.IDENTITY, prm["max_dist"], prm["kernel"], prm["sem_th"])
        host_entry_ms = 1e3 * (time.perf_counter() - t0) / k_host

    last = stats[-1]
    iters = last.iterations
    n_local = hi - lo
    us_nn = sum(s.us_nn for s in stats)             # the timed sample of k_icp launches
    launches = sum(s.nn_launches for s in stats)
    all_launches = sum(s.iterations for s in stats)  # every k_icp launch of the timed region
    cands = counted.sum_candidates                   # sum of C_q over the launches of the counted frame (by the kernel)
    pairs = counted.pairs_evaluated
    roofline = None
    if launches:
        n_corr = 0.5 * (last.n_corr_first + last.n_corr_last) * n_local / max(len(scan), 1)
        avg_us = us_nn / launches
        cand_per_launch = cands / max(counted.iterations, 1)
        pairs_per_launch = pairs / max(counted.iterations, 1)
        # Bytes the EXECUTED algorithm needs per launch, in SURVEY 8d's compact representation
        # (fused form): 448 B per query (16 query + 27 x 16 hash slots) + 16 B per (query, map
        # point) pair the search actually evaluates — counted by the kernel; the exact cell lower
        # bound prunes the rest without loading them — + 32 B per accepted correspondence.
        executed_bytes = 448.0 * n_local + 16.0 * pairs_per_launch + 32.0 * n_corr
        executed_gbs = executed_bytes / (avg_us * 1e-6) / 1e9          # GB/s
        # SURVEY 8d's contractual figure charges EVERY candidate of the 27 voxels (what the
        # reference's scan touches): an effective gather rate, not a bound on this kernel
        survey_bytes = 448.0 * n_local + 16.0 * cand_per_launch + 32.0 * n_corr
        compulsory = 16 * (vmap.size() + n_local + 4 * vmap.num_voxels())
        one_launch = bool(last.single_launch)
        # `achieved` / `frac` mean ONE thing: HBM-side bytes per iteration as rocprofv3 counts them (FETCH_SIZE x 2,
        # the guide's gfx950 correction) / the kernel-trace duration of the same iteration / 8 TB/s — from the
        # counter passes committed under profiles/, used only when they were collected on exactly this build and
        # this form of the loop.  Without such counters they are null (never a model under the same name); the
        # byte MODELS of the executed algorithm are reported under their own names, over the live HIP-event time.
        roofline = {"bound": "hbm",
                    "kernel": ("k_loop (the whole ICP loop in one launch: correspondence search + Gauss-Newton sums, "
                               "per iteration)") if one_launch else "k_icp (correspondence search + Gauss-Newton sums)",
                    "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                    "counters_fresh": False,
                    "frac_basis": "none: no rocprofv3 counters collected on this build and loop form "
                                  "(profiles/run_profiles.sh + profiles/collect.py refresh them)",
                    "traffic": None,
                    "executed_bytes_gbs": round(executed_gbs, 1),
                    "executed_bytes_frac": round(executed_gbs / HBM_PEAK_GBS, 4),
                    "algorithmic_bytes_per_launch": round(executed_bytes),
                    "algorithmic_bytes_model": "448 B x queries + 16 B x (query, map point) pairs evaluated "
                                               "(counted by the kernel) + 32 B x correspondences, per iteration: "
                                               "mostly L2 / Infinity-Cache traffic, NOT an HBM fraction",
                    "effective_gather_gbs": round(survey_bytes / (avg_us * 1e-6) / 1e9, 1),
                    "effective_gather_bytes_per_launch": round(survey_bytes),
                    "effective_gather_note": "SURVEY 8d's figure: every candidate of the 27 voxels charged "
                                             "(what the reference scans); the kernel prunes most of them "
                                             "exactly, so this rate is not bounded by the HBM peak",
                    # SURVEY 8d "compulsory" figure: every map point, query and hash slot once per
                    # launch in the compact representation (16 B each)
                    "compulsory_bytes_per_launch": int(compulsory),
                    "compulsory_gbs": round(compulsory / (avg_us * 1e-6) / 1e9, 1),
                    "avg_launch_us": round(avg_us, 2), "launches_timed": launches,
                    "launches": all_launches, "queries_per_launch": n_local,
                    "lanes_per_query": last.lanes_per_query,
                    "scan_form": "compact 16-B records behind an exact fp32 filter" if last.compact_scan
                                 else "full 32-B fp64 records",
                    "loop_form": "one launch for the whole loop (k_loop + its solving wave): avg_launch_us is the "
                                 "launch / its iterations, solve and hand-offs included"
                                 if one_launch else ("k_icp launches chained (no k_fin between them: the solving wave of the one-launch loop "
                                                     "resident beside them); avg_launch_us is k_icp alone, ms_per_step the whole iteration"
                                                     if mine["calls_chained"] else "k_icp + k_fin per iteration"),
                    "candidates_per_query": round(cand_per_launch / max(n_local, 1), 1),
                    "pairs_evaluated_frac": round(pairs / max(cands, 1), 4),
                    "pair_counts": "the library's per-wave counters (C_q, pairs evaluated) are off in the timed region — "
                                   "as for the C++ shim's calls, which pass no statistics — and on for one frame after it",
                    "timing": ("HIP events on the launch stream around the k_loop launch of every frame of the timed "
                               "region / its iterations") if one_launch else
                              ("mean k_icp duration from HIP events on the launch stream around 1 launch in 8 "
                               "of the timed region (an event pair also brackets the launch gap: the "
                               "rocprofv3 kernel-trace mean under profiles/ is ~3 us shorter)")}
        # What bounds the kernel, from the rocprofv3 counter passes of this command
        # (profiles/collect.py -> profiles/icp_counters.json).  They are measurements of a
        # particular build: used only when the device code they were taken on is the code that ran.
        cpath = os.path.join(ROOT, "profiles", "icp_counters.json")
        if os.path.exists(cpath) and world == 1 and args.scale == 1.0:
            try:
                c = json.load(open(cpath)).get("%s-%s" % (args.workload, args.params))
            except Exception as e:      # noqa
                c = None
                roofline["frac_basis"] = "none: profiles/icp_counters.json unreadable: %s" % e
            apply_counters(roofline, c, device_source_hash(), one_launch, compulsory, executed_bytes)

    fps = args.steps / elapsed * (world if args.independent else 1)
    cpu = parity = None
    if world == 1 and not args.no_cpu_baseline:
        cpu, parity = cpu_baseline(args, w, wl, prm, scan, iters, fps, pose, counted)

    err = None
    try:
        Tg = w["T_gt"]
        R1, R2 = syn.quat_to_mat(pose[:4]), syn.quat_to_mat(Tg[:4])
        ang = float(np.arccos(np.clip((np.trace(R1.T @ R2) - 1) / 2, -1, 1)))
        err = {"translation_m": round(float(np.linalg.norm(pose[4:] - Tg[4:])), 5),
               "rotation_rad": round(ang, 6)}
    except Exception:
        pass

    out = {
        "metric": "ICP frames/sec (120k-pt scan vs 1M-pt map)" if args.workload == "c2"
                  else "ICP frames/sec (%s)" % args.workload,
        "value": round(fps, 3),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4),
        "ms_per_step_host_entry": None if host_entry_ms is None else round(host_entry_ms, 4),
        "higher_is_better": True,
        "scaling": "weak" if args.independent else "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "%s-%s: %d-pt labelled scan vs %d-pt semantic voxel map (voxel %.1f m, "
                               "20+20 pts/voxel), max_corr %.2f kernel %.4f sem_th %.2f, identity "
                               "guess, full ICP loop to convergence"
                               % (args.workload, args.params, len(scan), vmap.size(), wl["voxel"],
                                  prm["max_dist"], prm["kernel"], prm["sem_th"]),
                   "parallelism": ("independent frames x%d (one whole frame per rank and step), map "
                                   "replicated, no exchange" % world) if use_dist and args.independent
                                  else "query-sharded x%d, map replicated, %s" % (world, exchange)
                                  if use_dist else "single GPU",
                   "ranks": world,
                   # which entry `value` times (the contract: inputs resident in HBM when the timed region starts; the
                   # PCIe-inclusive rate of the host-buffer entry the C++ shim calls is `ms_per_step_host_entry`, never `value`)
                   "entry": "sageicp_register_frame_resident (frame and map in HBM); the host-buffer entry "
                            "sageicp_register_frame, which sage_icp::RegisterFrame() of the shim calls, is timed in the same run "
                            "as ms_per_step_host_entry",
                   "counters_in_timed_region": "off (sageicp_set_counting(0)): the per-wave candidate / pair counters are "
                                               "instrumentation the shim's calls never pay for; one counted frame follows "
                                               "the timed region — frames/s are not comparable with BENCH files before round 5",
                   # what ran, without reading stderr: the exchange form of the timed region, the ranks
                   # RCCL itself reports for the communicator (ncclCommCount; None: no communicator),
                   # and the pose of one frame registered through both forms before the timed region
                   "exchange": ("none" if comm is None else "direct" if use_p2p else "rccl"),
                   "rccl_ranks": None if comm is None else comm.describe()["rccl_ranks"],
                   "comm": None if comm is None else comm.describe(),
                   "exchange_cross_check": cross_check,
                   "exchange_requested": args.exchange,
                   "per_rank": per_rank,
                   "iteration_breakdown": breakdown,
                   "scan_points": len(scan), "map_points": vmap.size(),
                   "map_voxels": vmap.num_voxels(), "iterations_per_frame": iters,
                   "correspondences_first_last": [last.n_corr_first, last.n_corr_last],
                   "converged": bool(last.converged),
                   "pose_error_vs_planted": err, "setup_seconds": round(t_gen, 1)},
        "roofline": roofline,
        "cpu_baseline": cpu,
        "parity": parity,
    }
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
