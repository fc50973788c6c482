"""The one-launch loop's staged first pass (loop_kernel.h, icp_body.h HALF): every wave runs the pose-independent front of
its first pass of an iteration — unit, priority, LDS layout, `perm`, the query's state record — in front of the wait for
the pose, carries it across the barrier, and stages the units it takes beyond the first behind the run before.  What can
go wrong: a wave that runs a pass it never staged (or stages one and drops it), a unit staged from the `perm` of the
iteration before, a row rebuilt from a key that was staged before the closing wave wrote it, a workgroup whose waves
disagree about the number of barriers, a loop that ends after a stage and still writes.

Every case (tests/loopstage_cases.py) registers a small frame against a synthetic map of 4,000 points with the one-launch
loop, shaped by the case's knobs, and with the launch-per-iteration loop at the same lanes per query and scan form: pose,
iteration count, n_corr history, last step and sum_candidates BIT for bit; and against the oracle at the tolerance of
tests/test_loop_kernel.py (1e-7 m, 1e-7 rad, the same iterations, correspondence counts and candidates).

All cases run in ONE child process, started once per session; the parent gives every case its own time limit (the child
prints a line per case as it finishes) and ends the child at the first case that exceeds it — nothing is tried twice.

Needs a real MI355X:  python -m pytest tests -m gpu"""
import json
import os
import queue
import subprocess
import sys
import threading

import pytest

import loopstage_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_CASE_SECONDS = 120.0      # the child's start: imports, the library, the device
CASE_SECONDS = 30.0             # a case takes some tens of milliseconds; a wait inside the launch gives up after seconds


@pytest.fixture(scope="module")
def results(gpu_sage):
    """{case id: the child's record}, plus "__error__" if the child ended early"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "loopstage_cases.py")]
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
    print("tests/loopstage_cases.py: %d of %d cases, %.1f s inside them"
          % (len(out) - ("__error__" in out), len(cases.IDS), sum(r["seconds"] for k, r in out.items() if k != "__error__")))
    return out


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_staged_first_pass_case(results, case):
    assert case["id"] in results, results.get("__error__", "the child did not reach this case")
    r = results[case["id"]]
    print(json.dumps({k: v for k, v in r.items() if k != "hist"}))
    assert r["same_map"]
    # the forms that were asked for ran, and the launch neither timed out nor fell back
    assert r["single_launch"] == [1, 0] and r["timeouts"] == 0 and r["last_fallback"] == 0
    assert r["lanes"] == [1 << case["lw"]] * 2 and r["compact"] == [case["filt"]] * 2
    # the two loops: bit for bit
    assert r["same_pose"]
    assert r["iterations"][0] == r["iterations"][1] and r["converged"][0] == r["converged"][1]
    assert r["hist"][0] == r["hist"][1]
    assert r["n_corr"][0] == r["n_corr"][1] and r["step"][0] == r["step"][1] and r["candidates"][0] == r["candidates"][1]
    # the oracle
    assert r["iterations"][0] == r["iterations"][2] and r["converged"][0] == r["converged"][2]
    assert r["n_corr"][0] == r["n_corr"][2] and r["candidates"][0] == r["candidates"][2]
    assert r["dt"] < 1e-7 and r["dr"] < 1e-7
    if case["scene"] == "far":
        assert r["n_corr"][0] == [0, 0] and r["iterations"][0] == 1
    elif case["scene"] == "near":
        assert r["iterations"][0] == 2 and r["n_corr"][0][1] == case["n"]
    else:
        assert r["iterations"][0] >= 2 and r["n_corr"][0][1] > case["n"] // 2
    if case["guess"] == "off":
        # (by the oracle alone: between consecutive iterations queries did step through faces, edges and corners)
        c = r["crossings"]
        assert c["face"] > 0 and c["edge"] > 0 and c["corner"] > 0, c
