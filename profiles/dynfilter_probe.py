"""What Preprocess()'s dynamic vehicle filter (csrc/dyn_filter.hip) costs per 120k-point frame (synthetic_dynamic
scenes: ~7 % vehicle points, ~9 % landmark points).
    python profiles/dynfilter_probe.py [frames of the long stream, default 200]

  1. the filter inside the pipeline, per frame: device time of its launches (HIP events, sageicp_set_profiling),
     host step (waiting for the cluster table + PCL order replay + static test), wall time of the whole filter
  2. per-frame pipeline time (RegisterFrame wall, Python side) with the filter off, on, and on with prefetch
  3. a long stream through the pipeline with the filter on, frames/s
  4. context only: the CPU restatement (tests/dynfilter_ref.cpp, brute force) on the same frames"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np  # noqa: E402
import sage_icp_amd as sage  # noqa: E402
from sage_icp_amd import synthetic_dynamic as sd  # noqa: E402

N_LONG = int(sys.argv[1]) if len(sys.argv) > 1 else 200
N = 120000
frames = sd.make_dynamic_stream(31, 40, n=N)[0]
med = lambda v: float(np.median(v))   # noqa: E731


def run(pipe, fr, prefetch=False, info=False):
    t, inf = [], []
    for k, f in enumerate(fr):
        if prefetch and k + 1 < len(fr):
            pipe.prefetch(fr[k + 1])
        t0 = time.perf_counter()
        pipe.RegisterFrame(f)
        t.append(1e3 * (time.perf_counter() - t0))
        if info:
            inf.append(pipe.dynamic_filter_info())
    return np.array(t[5:]), inf[5:]


res = {"frame_points": N}
# 1. the filter's own cost, inside the pipeline (profiling on: HIP events around its three launch batches)
sage.set_profiling(1)
on = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
_, inf = run(on, frames, info=True)
sage.set_profiling(0)
res["vehicle_points"] = med([i["vehicle_points"] for i in inf])
res["landmark_points"] = med([i["landmark_points"] for i in inf])
res["clusters"] = med([i["clusters"] for i in inf])
res["filter_us_device"] = med([i["us_device"] for i in inf])
res["filter_us_host_step"] = med([i["us_host"] for i in inf])
res["filter_us_wall_profiled"] = med([i["us_wall"] for i in inf])
on2 = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
_, inf = run(on2, frames, info=True)
res["filter_us_wall"] = med([i["us_wall"] for i in inf])
res["filter_us_host_step_unprofiled"] = med([i["us_host"] for i in inf])

# 2. per-frame pipeline time: off / on / on + prefetch (the same frames, three fresh pipelines; two rounds each)
for rnd in range(2):
    for name, kw, pf in (("off", {}, False), ("on", {"dynamic_vehicle_filter": True}, False),
                         ("on_prefetch", {"dynamic_vehicle_filter": True}, True)):
        p = sage.SageICP(sage.make_pipeline_config(**kw))
        t, _ = run(p, frames, prefetch=pf)
        res.setdefault("pipeline_ms_" + name, []).append(med(t))
for k in [k for k in res if k.startswith("pipeline_ms_")]:
    res[k] = min(res[k])
res["filter_cost_ms_per_frame"] = res["pipeline_ms_on"] - res["pipeline_ms_off"]
res["filter_cost_ms_per_frame_prefetch"] = res["pipeline_ms_on_prefetch"] - res["pipeline_ms_off"]

# 3. a long stream with the filter on (frames generated outside the timed calls)
p = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
gen = sd.make_dynamic_stream(41, N_LONG, n=N)[0] if N_LONG <= 60 else None
kept, t_all = 0, []
for k in range(N_LONG):
    f = gen[k] if gen is not None else sd._scene(np.random.default_rng(1000 + k), N, -0.5 * N_LONG + k, k)[0]
    t0 = time.perf_counter()
    p.RegisterFrame(f)
    t_all.append(time.perf_counter() - t0)
    kept += p.dynamic_filter_info()["clusters_kept"]
res["long_stream_frames"] = N_LONG
res["long_stream_ms_per_frame_median"] = 1e3 * med(t_all[5:])
res["long_stream_ms_per_frame_mean"] = 1e3 * float(np.mean(t_all[5:]))
res["long_stream_fps"] = 1.0 / float(np.mean(t_all[5:]))
res["long_stream_clusters_kept_mean"] = kept / N_LONG
res["long_stream_poses_finite"] = bool(np.isfinite(p.poses()).all())

# 4. context: the CPU restatement (brute-force radius search, one thread)
try:
    import dynref
    t = []
    for f in frames[:5]:
        t0 = time.perf_counter()
        dynref.preprocess(f)
        t.append(1e3 * (time.perf_counter() - t0))
    res["cpu_restatement_ms_context_only"] = med(t)
except Exception as e:  # noqa: BLE001
    res["cpu_restatement_ms_context_only"] = "unavailable: %s" % e

for k, v in res.items():
    print("%-40s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v))
print(json.dumps(res))
