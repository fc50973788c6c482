"""One Gauss-Newton step of the device, pairs to pose, against extended precision (tests/gnref.py): what neither the
converged poses against the fp64 oracle nor the bit-identity of one device form with another can see — a mistake in
J^T J alone leaves the fixed point of the iteration where it was, and a mistake in the text all device forms are
instantiated from leaves them identical to one another.

a. The stand-alone entry sageicp_align_clouds (k_gn, k_fin over partials, the solve and the exponential under the
   wavefront's lane policy) on the pair sets of tests/gnstep_cases.py: J^T J and J^T r componentwise within gamma x the
   sums of their terms' magnitudes, the pose by its action on eight points within TAU of the budget; where the system is
   rank deficient, the residual of the normal equations at the pose's exact logarithm.
b. The first two iterations of RegisterFrame (the fused epilogue), stopped with SAGEICP_MAX_ITER, in both loops, at
   2 - 16 lanes per query, both scan forms: the cases of tests/gnstep_cases.py, run in ONE child process with a time
   limit per case; the parent ends the child at the first overrun and nothing is tried twice.

Every error is divided by its budget, first order and worst case, derived from the inputs.  TAU = 4 x the worst ratio
of the fp64 oracle (tests/test_gn_step_host.py), rounded up to a power of two.  Measured on an MI355X (worst ratios):
see DESIGN.md section 5.

Needs a real MI355X:  python -m pytest tests -m gpu"""
import json
import os
import queue
import subprocess
import sys
import threading

import numpy as np
import pytest

import gnref
import gnstep_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_CASE_SECONDS = 120.0      # the child's start: imports, the library, the device
CASE_SECONDS = 30.0             # a case takes some tens of milliseconds; a wait inside the launch gives up after seconds
IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


# ---- a. AlignClouds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", cases.PAIR_CASES, ids=cases.PAIR_IDS)
def test_align_clouds_step(gpu_sage, name, n):
    s, q, k, _, _, pts = cases.pair_case(name, n)
    st = cases.pair_truth(name, n)
    T, JTJ, JTr = gpu_sage.align_clouds(s, q, k)
    gamma = gnref.gamma_partials(n)
    sums = st.sums_ratio(JTJ, JTr, gamma)
    fig = dict(case="%s-n%d" % (name, n), sums=sums, full_rank=st.full_rank)
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(JTJ)) and np.all(np.isfinite(JTr))
    if name == "identical":
        assert np.array_equal(T, IDENTITY) and not np.any(JTr)
    if st.full_rank:
        fig["pose"] = st.ratio(T, pts, gamma)
        fig["theta"] = st.theta
    elif st.turn < cases.MAX_TURN:
        fig["residual"] = st.residual_ratio(gnref.log_se3(T), gamma, of_pose=True)
    print(json.dumps(fig))
    if name == "utm":
        return                      # fp64 itself is ill-conditioned at these coordinates: reported only
    assert sums <= 1.0
    assert fig.get("residual", 0.0) <= 1.0
    assert fig.get("pose", 0.0) <= (cases.TAU if cases.PAIR_DETECTOR[name] else 1.0)


# ---- b. the first two iterations of RegisterFrame ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def results(gpu_sage):
    """{case id: the child's record}, plus "__error__" if the child ended early"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "gnstep_cases.py")]
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    lines, err = queue.Queue(), []

    def pump():
        for line in child.stdout:
            lines.put(line)
        lines.put(None)

    threading.Thread(target=pump, daemon=True).start()
    threading.Thread(target=lambda: err.append(child.stderr.read()), daemon=True).start()
    out = {}
    try:
        for i, cid in enumerate(cases.IDS):
            try:
                line = lines.get(timeout=FIRST_CASE_SECONDS if i == 0 else CASE_SECONDS)
            except queue.Empty:
                out["__error__"] = "case %s exceeded its time limit" % cid
                break
            if line is None:
                child.wait()
                out["__error__"] = "the child ended (status %s) before case %s:\n%s" % (child.returncode, cid, "".join(err)[-3000:])
                break
            r = json.loads(line)
            out[r["id"]] = r
    finally:
        if child.poll() is None:
            child.kill()
        child.wait()
    done = {k: r for k, r in out.items() if k != "__error__"}
    print("tests/gnstep_cases.py: %d of %d cases, %.1f s inside them" % (len(done), len(cases.IDS), sum(r["seconds"] for r in done.values())))
    worst = {}
    for r in done.values():
        key = r["id"].split("-n")[0] + " loop%d" % (2 if "-loop2-" in r["id"] else 0)
        w = worst.setdefault(key, dict(ratio1=0.0, ratio2=0.0, step1=0.0, step2=0.0))
        for f in w:
            w[f] = max(w[f], r.get(f, 0.0))
    for key, w in worst.items():
        print("  %-14s %s" % (key, "  ".join("%s=%.3g" % kv for kv in w.items())))
    return out


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_register_frame_first_two_steps(results, case):
    assert case["id"] in results, results.get("__error__", "the child did not reach this case")
    r = results[case["id"]]
    print(json.dumps(r))
    scene = case["scene"]
    bound = cases.TAU if cases.SCENE_DETECTOR[scene] else 1.0
    assert r["same_map"] and r["clear1"]
    # the forms that were asked for ran, and no launch timed out or fell back
    for form in (r["form1"], r["form2"]):
        assert form["single_launch"] == (1 if case["loop"] == 2 else 0) and form["timeouts"] == 0
        assert form["last_fallback"] == 0 or case["loop"] == 0       # (with the one-launch loop switched off: "the form is off")
        assert form["lanes"] == 1 << case["lw"] and form["compact"] == case["filt"]
    assert r["repeat_same"]                       # the pose after one iteration, bit for bit, twice
    assert r["n_corr1"] == r["pairs1"] and r["iterations1"] == 1
    if scene == "far":
        assert r["pairs1"] == 0 and r["pose_is_guess"] and r["same_after_two"]
        return
    assert r["full_rank1"] and r["pairs1"] > case["n"] // 2
    if scene != "utm":
        assert r["ratio1"] <= bound and r["step1"] <= 1.0
    if not r["two"]:
        # the step was below the loop's threshold: it has converged, and a second iteration is not run
        assert r["converged1"] == 1 and r["iterations2"] == 1 and r["same_after_two"]
        return
    assert r["converged1"] == 0 and r["iterations2"] == 2
    assert r["clear2"] and r["full_rank2"] and r["n_corr2"] == [r["pairs1"], r["pairs2"]]
    if scene != "utm":
        assert r["ratio2"] <= bound and r["step2"] <= 1.0
