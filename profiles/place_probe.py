"""What place recognition costs (csrc/place.hip).  Written to <out>/place_probe_<what>.txt; a host clock around each
synchronous call, the median of --calls calls after --warmup and their range.

  --what describe  a 120 000-point frame (c2's scan) as a float64 (n, 4) tensor on the GPU: sageicp_place_describe_device
                   at 20 x 60 next to sageicp_occupancy_grid_device of the same frame — both one pass over the rows with
                   LDS atomics, the grid pass is the yardstick.
  --what match     databases of 1, 256, 4 096 and 65 536 random descriptors at 20 x 60, a half-occupied query: one
                   sageicp_place_db_match (top_k 4) with the sector index wrapped (the default) and with the entry held
                   twice along S in LDS instead (SAGEICP_PLACE_DOUBLED=1).  The call at 1 entry runs the same
                   copies, launches and wait on a trivial kernel: what a call costs beyond it is the scoring pass.
  --what pipeline  a c3-style stream (synthetic.make_stream, 30 k points per frame), every frame a key frame (overlap
                   threshold above 1), the place database loaded with 4 096 entries first: per frame, the wall time of
                   RegisterFrame with places off and on, alternating frame by frame between two pipelines fed the same
                   frames (poses asserted equal); the difference is describe + match + add per key frame.
  --what icp       the same stream through a plain pipeline: icp_s per frame.  SAGE_TREE=<a checkout> measures that
                   checkout's package and library (the parent's, for the condition set for this feature)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(os.environ.get("SAGE_TREE", ROOT))
sys.path.insert(0, TREE)
import torch                                                    # noqa: E402  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic as syn                       # noqa: E402

NEAR = ((-20.0, 20.0), (-20.0, 20.0), (-4.0, 2.4))
RANK = {c: 1 for c in range(1, 256)}
RANK.update({10: 0, 70: 2, 51: 3, 50: 4, 71: 5, 80: 6, 81: 6})


def timed(fn, calls, warmup):
    t = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i >= warmup:
            t.append(dt * 1e3)
    return np.array(t)


def line(name, t):
    return "  %-66s %8.3f  (min %.3f, p10 %.3f, p90 %.3f, max %.3f)" % (
        name, np.median(t), t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max())


def random_descs(rng, n, R, S, fill=0.5):
    h = rng.integers(1, 256, size=(n, 1, R, S)).astype(np.uint8)
    h[rng.random(h.shape) >= fill] = 0
    c = rng.choice(np.array([40, 44, 50, 70, 71, 80], dtype=np.uint8), size=(n, 1, R, S))
    return np.concatenate([h, c], axis=1)


def describe(a):
    rng = np.random.default_rng(3)
    q = syn.make_scan(rng, 120000, 120.0, syn.T_GT_C2)
    qt = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    torch.cuda.synchronize()
    params = sage.place_params(rank=RANK)
    lines = ["a frame of %d points as a float64 tensor on the GPU; median of %d calls after %d, ms" % (len(q), a.calls, a.warmup)]
    lines.append(line("sageicp_occupancy_grid_device, 128 x 128 (launch-file bounds)", timed(lambda: sage.occupancy_grid(qt), a.calls, a.warmup)))
    lines.append(line("sageicp_occupancy_grid_device, 64 x 64 (near bounds)", timed(lambda: sage.occupancy_grid(qt, NEAR, (64, 64)), a.calls, a.warmup)))
    for R, S in ((20, 60), (64, 256)):
        p = sage.place_params(rings=R, sectors=S, rank=RANK)
        lines.append(line("sageicp_place_describe_device, %d x %d" % (R, S), timed(lambda: sage.place_describe(qt, p), a.calls, a.warmup)))
    h, _ = sage.place_describe(qt, params)
    lines.append("  occupied cells at 20 x 60: %d of 1200" % int((h > 0).sum()))
    return lines


def match(a):
    R, S = 20, 60
    params = sage.place_params(rings=R, sectors=S, rank=RANK)
    rng = np.random.default_rng(4)
    query = random_descs(rng, 1, R, S)[0]
    lines = ["databases of random descriptors at %d x %d (half the cells occupied), top_k 4, h_tol 40; median of %d calls "
             "after %d, ms" % (R, S, a.calls, a.warmup)]
    med = {}
    for n in (1, 256, 4096, 65536):
        db = sage.PlaceDB(params)
        for lo in range(0, n, 4096):
            for d in random_descs(rng, min(4096, n - lo), R, S):
                db.add(d)
        for wrap in (1, 0):
            os.environ["SAGEICP_PLACE_DOUBLED"] = str(1 - wrap)
            t = timed(lambda: db.match(query, top_k=4, h_tol=40), a.calls, a.warmup)
            med[(n, wrap)] = np.median(t)
            lines.append(line("match, %6d entries, %s" % (n, "index wrapped" if wrap else "entry twice in LDS"), t))
        os.environ.pop("SAGEICP_PLACE_DOUBLED")
        del db
    for n in (256, 4096, 65536):
        for wrap in (1, 0):
            k = med[(n, wrap)] - med[(1, wrap)]
            lines.append("  %6d entries, %-18s: %.3f ms beyond the call at 1 entry (%.0f %% of the call); %.1f G cell comparisons / s"
                         % (n, "index wrapped" if wrap else "entry twice in LDS", k, 100 * k / med[(n, wrap)],
                            n * R * S * S * 0.5 / max(k, 1e-6) / 1e6))
    return lines


def stream(a):
    return syn.make_stream(11, a.calls + a.warmup, points_per_frame=30000)[0]


def pipeline(a):
    frames = stream(a)
    params = sage.place_params(rank=RANK)
    off, on = sage.SageICP(sage.make_pipeline_config()), sage.SageICP(sage.make_pipeline_config())
    for p in (off, on):
        p.set_key_frames(True, NEAR, (64, 64), 1.5)            # overlap < 1.5 always: every frame is a key frame
    on.set_places(True, params, top_k=4, h_tol=40, exclude_last=30, min_similarity=0.4)
    db = on.places()
    for d in random_descs(np.random.default_rng(5), 4096, params.rings, params.sectors):
        db.add(d)
    rows = []
    for k, f in enumerate(frames):
        t = {}
        for name, p in ((("off", off), ("on", on)) if k % 2 == 0 else (("on", on), ("off", off))):
            t0 = time.perf_counter()
            out = p.RegisterFrame(f)
            t[name] = ((time.perf_counter() - t0) * 1e3, out[1] * 1e3, out[0])
        assert np.array_equal(t["off"][2], t["on"][2]), "frame %d" % k
        assert on.place_info()["described"] and on.key_frame_info()["is_key_frame"]
        if k >= a.warmup:
            rows.append((t["off"][0], t["on"][0], t["off"][1], t["on"][1]))
    r = np.array(rows)
    return ["c3-style stream, 30000 points per frame, %d frames after %d, every frame a key frame; the place database holds "
            "%d entries at the end; ms per frame" % (len(r), a.warmup, len(db)),
            line("RegisterFrame wall, key frames on, places off", r[:, 0]), line("RegisterFrame wall, key frames on, places on", r[:, 1]),
            line("describe + match + add per key frame (on - off, frame by frame)", r[:, 1] - r[:, 0]),
            line("icp_s, places off", r[:, 2]), line("icp_s, places on (the place step runs outside it)", r[:, 3])]


def icp(a):
    frames = stream(a)
    p = sage.SageICP(sage.make_pipeline_config())
    t = np.array([p.RegisterFrame(f)[1] * 1e3 for f in frames])[a.warmup:]
    return ["tree %s; c3-style stream, 30000 points per frame, %d frames after %d" % ("this" if TREE == ROOT else "SAGE_TREE (the parent)", len(t), a.warmup),
            line("icp_s per frame", t)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=["describe", "match", "pipeline", "icp"])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34"))
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    lines = {"describe": describe, "match": match, "pipeline": pipeline, "icp": icp}[a.what](a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "place_probe_%s%s.txt" % (a.what, "" if TREE == ROOT else "_parent")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
