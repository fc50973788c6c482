"""Chooses the rows of csrc/loop_deal.h's table: which unit (by rank in its workgroup's heaviest-first order) the wave
on SIMD s of a CU's fifth, sixth and seventh workgroup takes first.  CPU only.
    python profiles/deal_table.py profiles/r33/deal_inputs.json > profiles/r33/deal_model.txt
Input: a JSON list of the `deal-input:` records profiles/loop_tail.py prints from a -DSAGE_LOOP_TIMING build — per input
the mean and the spread of a unit's work (the most points one of its queries was handed) for the ranks 0-3 and for the
unit beyond one per wave, how long such a unit lasted against its work, and which rank's wave is free first.

Model.  A SIMD's waves share its issue slots, so a SIMD ends when the issue work of ALL its waves is done, whatever the
order the priorities give them: the cost of a SIMD is the sum of the costs of its units.  A unit costs
    cost = A + B x (points of its heaviest query)
(a pass lasts as long as its longest lane; A is the straight-line work of a pass).  A and B are one weighted
least-squares line through (work, lasts) of the units beyond one per wave, all inputs together, a point per bin of 20
points of work weighted by its count: those units run at one priority and start when their SIMD has emptied, so their
duration is the cleanest measure of what a pass costs.  Only A / B matters to the choice.  The unit beyond one per wave
goes to the wave that is free first: rank r's cost grows by share(workgroups with such a unit) x P(rank r's wave ends
first) x cost(that unit).

Search: rows 0-3 are the Latin square (simd + slot) mod 4 and stay.  All 24^3 permutations for rows 4-6; rows 7-9 repeat
rows 4-6 (k_loop's 7 waves per SIMD: no CU holds more than seven workgroups today).  A CU of P workgroups uses rows
0..P-1.  For every input and P in 5, 6, 7: the largest column (SIMD) sum relative to the mean column sum.  Admitted are
tables that are no worse than the formula on EVERY input and population; among them the one with the smallest worst-input
ratio at P = 7 (the seven-workgroup CUs end the iteration), then at 6, then at 5, then the smallest sum of spreads."""
import itertools
import json
import sys

import numpy as np

PERMS = list(itertools.permutations(range(4)))
FORMULA_ROWS = [tuple((s + r) & 3 for s in range(4)) for r in range(10)]


def fit(inputs):
    """-> (A, B) of lasts = A + B * work over the bins of every input, weighted by count"""
    pts = [b for i in inputs for b in i.get("extra_bins", [])]
    if len(pts) < 2:
        raise SystemExit("no units beyond one per wave in the inputs: nothing to fit the cost model to")
    cnt, x, y = (np.array(c, dtype=float) for c in zip(*pts))
    X = np.stack([np.ones_like(x), x], axis=1) * np.sqrt(cnt)[:, None]
    (a, b), *_ = np.linalg.lstsq(X, y * np.sqrt(cnt), rcond=None)
    return float(a), float(b)


def rank_costs(i, a, b):
    """effective cost of the ranks 0..3 of one input (see the model above)"""
    w = i["work_mean"]
    c = [a + b * w[r] for r in range(4)]
    if len(w) > 4 and w[4] > 0:
        c5 = a + b * w[4]
        c = [c[r] + i["fifth_share"] * i["first_done_by_rank"][r] * c5 for r in range(4)]
    return c


def columns(rows, cost, pop):
    return [sum(cost[rows[r][s]] for r in range(pop)) for s in range(4)]


def ratios(rows, costs):
    """-> {pop: [max column / mean column per input]}"""
    out = {}
    for pop in (5, 6, 7):
        out[pop] = []
        for c in costs:
            col = columns(rows, c, pop)
            out[pop].append(max(col) / (sum(col) / 4.0))
    return out


def search(costs):
    base = ratios(FORMULA_ROWS, costs)
    best, best_key = None, None
    for r4, r5, r6 in itertools.product(PERMS, repeat=3):
        rows = FORMULA_ROWS[:4] + [r4, r5, r6]
        rt = ratios(rows, costs)
        if any(rt[p][k] > base[p][k] + 1e-12 for p in (5, 6, 7) for k in range(len(costs))):
            continue
        spread = sum(max(col) - min(col) for p in (5, 6, 7) for c in costs for col in [columns(rows, c, p)])
        key = (round(max(rt[7]), 9), round(max(rt[6]), 9), round(max(rt[5]), 9), round(spread, 9), (r4, r5, r6))
        if best_key is None or key < best_key:
            best, best_key = [r4, r5, r6], key
    return best


def main():
    inputs = json.load(open(sys.argv[1]))
    a, b = fit(inputs)
    print("cost of a unit = %.3f us + %.5f us x (points of its heaviest query): weighted least squares over %d bins of the units beyond one per wave"
          % (a, b, sum(len(i.get("extra_bins", [])) for i in inputs)))
    print("(a pass's fixed part equals %.0f points of scan)" % (a / b))
    use = [i for i in inputs if i["waves"] == 4]
    for i in inputs:
        if i["waves"] != 4:
            print("%s: %d waves per workgroup — the formula deals this shape; not an input of the table" % (i["input"], i["waves"]))
    costs = [rank_costs(i, a, b) for i in use]
    for i, c in zip(use, costs):
        print("%-20s %d lanes/query, %d workgroups; work by rank %s, sd %s; beyond: %.1f in %.0f %% of the workgroups, taken by rank %s"
              % (i["input"], i["lanes_per_query"], i["workgroups"], " ".join("%.1f" % x for x in i["work_mean"][:4]),
                 " ".join("%.1f" % x for x in i["work_sd"][:4]), i["work_mean"][4] if len(i["work_mean"]) > 4 else 0.0,
                 100.0 * i["fifth_share"], " ".join("%.2f" % x for x in i["first_done_by_rank"])))
        print("%-20s effective cost by rank, us: %s" % ("", " ".join("%.2f" % x for x in c)))
    rows = search(costs)
    if rows is None:
        print("no table is at least as good as the formula on every input and population: the formula stays")
        rows = FORMULA_ROWS[4:7]
    table = FORMULA_ROWS[:4] + rows
    print("rows 4-6 (rank by SIMD 0..3): formula %s | table %s" % (FORMULA_ROWS[4:7], rows))
    for i, c in zip(use, costs):
        for pop in (5, 6, 7):
            for nm, rw in (("formula", FORMULA_ROWS), ("table", table)):
                col = columns(rw, c, pop)
                print("%-20s CU of %d workgroups, %-7s: SIMD sums %s us | largest %.2f, over the mean %.2f, gap largest - smallest %.2f"
                      % (i["input"], pop, nm, " ".join("%.2f" % x for x in col), max(col), max(col) - sum(col) / 4.0, max(col) - min(col)))
    print("for csrc/loop_deal.h:")
    print("constexpr unsigned char kRows[kTableSlots][4] = {%s};" % ", ".join("{%s}" % ", ".join(str(x) for x in r) for r in rows + rows))
    return rows


if __name__ == "__main__":
    main()
