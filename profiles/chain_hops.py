"""The serial chain between two searches of the one-launch loop, hop by hop (-DSAGE_LOOP_TIMING build, LOOP_LIB or
sage-icp_amd/_probe/libsageicp_looptiming.so): last workgroup counted in -> the solving wave saw the counts -> sums in
fp64 -> solved -> exponential -> composed -> ready to publish -> stores issued (and the history written) -> pose held
by the workgroups, over all and per XCD (blockIdx & 7).  Means over the iterations 3..30 of the third registration.
    python profiles/chain_hops.py [workload c2]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import sage_icp_amd as sage  # noqa: E402

sage.LIB_PATH = os.environ.get("LOOP_LIB", os.path.join(os.path.dirname(sage.LIB_PATH), "_probe", "libsageicp_looptiming.so"))
from sage_icp_amd import synthetic as syn  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c2"
p = syn.PARAMS["cold"]
w = syn.make_workload(name, lambda: sage.VoxelHashMap(syn.WORKLOADS[name]["voxel"], 100.0))
f = sage.Frame(w["map"], w["scan"])
os.environ["SAGEICP_LOOP"] = "2"
sage.set_counting(False)
for _ in range(3):
    pose, st = sage.register_frame(f, w["map"], sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"], return_stats=True)
assert st.single_launch == 1
IT, WG = 32, 2048
wg = np.zeros((IT, WG, 4), dtype=np.uint64)
sv = np.zeros((IT, 4), dtype=np.uint64)
s2 = np.zeros((IT, 4), dtype=np.uint64)
sage.lib().sageicp_debug_loop_times(wg.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p))
sage.lib().sageicp_debug_loop_solver2(s2.ctypes.data_as(C.c_void_p))
wg = wg.astype(np.float64) / 100.0
sv = sv.astype(np.float64) / 100.0
s2 = s2.astype(np.float64) / 100.0
used = wg[1, :, 0] > 0
n = min(IT, st.iterations) - 1
its = list(range(3, n))
print("%s: %d queries, %d lanes/query, %d iterations, %d workgroups; iterations 3..%d of an instrumented build, us"
      % (name, len(w["scan"]), st.lanes_per_query, st.iterations, int(used.sum()), n - 1))
period = np.diff(sv[3:n, 2])
print("iteration period (ready to publish -> the next): mean %.2f  p0 %.2f  p50 %.2f  p100 %.2f  | change from one to the next: p50 %.2f p90 %.2f p100 %.2f"
      % (period.mean(), period.min(), np.median(period), period.max(),
         np.median(np.abs(np.diff(period))), np.quantile(np.abs(np.diff(period)), .9), np.abs(np.diff(period)).max()))


def line(label, a):
    a = np.asarray(a)
    print("   %-52s mean %.2f  p0 %.2f  p50 %.2f  p90 %.2f  p100 %.2f" % (label, a.mean(), a.min(), np.median(a), np.quantile(a, .9), a.max()))


last_in = np.array([wg[i, used, 0].max() for i in its])
line("last workgroup counted in -> solver saw the counts", sv[its, 0] - last_in)
line("counts complete -> sums in fp64", sv[its, 1] - sv[its, 0])
line("solve", s2[its, 0] - sv[its, 1])
line("exponential", s2[its, 1] - s2[its, 0])
line("composition + rotation matrix", s2[its, 2] - s2[its, 1])
line("composition -> ready to publish (norm test, hand-over)", sv[its, 2] - s2[its, 2])
line("ready to publish -> stores issued, history written", sv[its, 3] - sv[its, 2])
line("counts complete -> ready to publish", sv[its, 2] - sv[its, 0])
held = np.stack([wg[i, used, 1] - sv[i, 2] for i in its])          # [iteration][workgroup]
print("   ready to publish -> pose held by a workgroup (per iteration's percentile, mean over iterations):")
print("      all      p0 %.2f  p50 %.2f  p90 %.2f  p100 %.2f" % (held.min(1).mean(), np.median(held, 1).mean(), np.quantile(held, .9, 1).mean(), held.max(1).mean()))
b = np.arange(WG)[used]
for x in range(8):
    h = held[:, (b & 7) == x]
    print("      XCD %d    p0 %.2f  p50 %.2f  p90 %.2f  p100 %.2f" % (x, h.min(1).mean(), np.median(h, 1).mean(), np.quantile(h, .9, 1).mean(), h.max(1).mean()))
line("last workgroup counted in -> last workgroup holds the pose", np.array([wg[i, used, 1].max() for i in its]) - last_in)
