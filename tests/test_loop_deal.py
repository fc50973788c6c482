"""Which unit a wave of the one-launch loop takes first: csrc/loop_deal.h.

CPU half: the header compiled into a host program (tests/loop_deal_check.cpp) — every row a permutation of the ranks
when a workgroup has four waves, below the number of waves otherwise; slots 0-3 the parent's formula; rows 7-9 the rows
4-6; and, with the committed measurements (profiles/r33/deal_inputs.json) under the model of profiles/deal_table.py, a
largest SIMD sum no larger than the formula's for CUs of 5, 6 and 7 workgroups on every input.

GPU half (marked gpu; tests/loopdeal_cases.py, ONE child process, the parent gives every case its own time limit and ends
the child at the first case that exceeds it): pose and statistics bit for bit between the table, the formula, no deal and
the launch-per-iteration loop, on the smallest grids that reach the table's rows.

Needs a real MI355X for the GPU half:  python -m pytest tests -m gpu"""
import importlib.util
import json
import os
import queue
import subprocess
import sys
import threading

import pytest

import loopdeal_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIRST_CASE_SECONDS = 120.0      # the child's start: imports, the library, the device
CASE_SECONDS = 30.0             # a case takes a fraction of a second; a wait inside the launch gives up after seconds


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.fixture(scope="module")
def dealt(tmp_path_factory):
    """{(nw, slot): (table's ranks by SIMD, formula's ranks by SIMD)} from the host program"""
    exe = str(tmp_path_factory.mktemp("loop_deal") / "loop_deal_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sage-icp_amd", "csrc"), os.path.join(HERE, "loop_deal_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        v = list(map(int, line.split()))
        out[(v[0], v[1])] = (tuple(v[2:6]), tuple(v[6:10]))
    assert len(out) == 8 * 16
    return out


def test_every_row_deals_valid_ranks(dealt):
    for (nw, slot), (table, formula) in dealt.items():
        if nw == 4:
            assert sorted(table) == [0, 1, 2, 3], (nw, slot, table)
        else:
            assert all(0 <= r < nw for r in table), (nw, slot, table)
            assert table == formula, (nw, slot, table)       # every other shape: the parent's rule
        assert formula == tuple((s + slot) % nw for s in range(4))


def test_slots_0_to_3_are_the_formula_and_rows_7_to_9_repeat_rows_4_to_6(dealt):
    for slot in range(4):
        assert dealt[(4, slot)][0] == tuple((s + slot) & 3 for s in range(4))
    for slot in (7, 8, 9):
        assert dealt[(4, slot)][0] == dealt[(4, slot - 3)][0]
    for slot in range(10, 16):                                # (the hardware's slot field goes to 9)
        assert dealt[(4, slot)][0] == dealt[(4, slot)][1]


def test_the_table_is_no_worse_than_the_formula_by_the_model_on_every_input(dealt):
    spec = importlib.util.spec_from_file_location("_deal_table", os.path.join(ROOT, "profiles", "deal_table.py"))
    dt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dt)
    with open(os.path.join(ROOT, "profiles", "r33", "deal_inputs.json")) as fh:
        inputs = json.load(fh)
    assert len(inputs) == 4
    a, b = dt.fit(inputs)
    assert a > 0 and b > 0
    table = [dealt[(4, slot)][0] for slot in range(7)]
    formula = [dealt[(4, slot)][1] for slot in range(7)]
    for i in inputs:
        assert i["waves"] == 4
        cost = dt.rank_costs(i, a, b)
        assert cost[0] > cost[1] > cost[2] > cost[3] > 0, cost      # rank 0 is the heaviest
        for pop in (5, 6, 7):
            t, f = max(dt.columns(table, cost, pop)), max(dt.columns(formula, cost, pop))
            print("%s, CU of %d workgroups: largest SIMD sum %.3f (table) %.3f (formula)" % (i["input"], pop, t, f))
            assert t <= f, (i["input"], pop, t, f)
    # the committed rows are the ones the search finds from the committed inputs
    assert [tuple(r) for r in dt.search([dt.rank_costs(i, a, b) for i in inputs])] == table[4:7]


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def results(gpu_sage):
    """{case id: the child's record}, plus "__error__" if the child ended early"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "loopdeal_cases.py")]
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
    print("tests/loopdeal_cases.py: %d of %d cases, %.1f s inside them"
          % (len(out) - ("__error__" in out), len(cases.IDS), sum(r["seconds"] for k, r in out.items() if k != "__error__")))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_the_deal_does_not_reach_a_bit_of_the_result(results, case):
    assert case["id"] in results, results.get("__error__", "the child did not reach this case")
    r = results[case["id"]]
    print(json.dumps({"id": r["id"], "plan": r["plan"], "seconds": r["seconds"], "iterations": [x["iterations"] for x in r["runs"]]}))
    # the grid that was meant ran: lanes per query, workgroups, waves per workgroup, units per workgroup at most
    assert r["plan"] == case["plan"]
    table, formula, none, per_iteration = r["runs"]
    assert [x["single_launch"] for x in r["runs"]] == [1, 1, 1, 0]
    assert all(x["lanes"] == 16 and x["timeouts"] == 0 for x in r["runs"])
    assert all(x["last_fallback"] == 0 for x in (table, formula, none))      # (the launch-per-iteration run was asked for: "does not fit")
    # a registration that does something: several iterations, most of the frame matched
    assert table["iterations"] >= 3 and table["n_corr"][1] > case["n"] // 2
    for other in (formula, none, per_iteration):
        for key in ("pose", "iterations", "converged", "hist", "n_corr", "step", "candidates"):
            assert other[key] == table[key], key
