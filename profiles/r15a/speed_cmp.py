"""The listing speed_vs_parent.txt from the results of a speed visit (cmd.sh):

  python3 profiles/r15a/speed_cmp.py DIR ROUNDS

DIR holds bench_<b><r>.json, groups_<b><r>.json, fallback_<b><r>.json and shuffled_<b><r>.json for b in parent /
new and r = 1..ROUNDS: the result line of each run (of sweep.py's child: what follows "RESULT ").  A figure's
value in a run is what the tool reports for it (bench.py: the mean over its 20 steps, the legs' own medians;
fallback_time.py and sweep.py's child: the median over the run's calls).  Band: [parent min - spread, parent
max + spread], spread = parent max - min over the rounds; the verdict is where the new build's median over the
rounds lies."""
import json
import os
import sys

import numpy as np


def result(path):
    return json.load(open(path))


def figures(d, b, r):
    f = {}
    j = result(os.path.join(d, f"bench_{b}{r}.json"))
    dm = j["device_ms"]
    f["bench.py cfg4 ms_per_step"] = j["ms_per_step"]
    f["bench.py device step_total"] = dm["step_total"]
    f["bench.py device volume_stage"] = dm["volume_stage"]
    f["bench.py device volume_fallback"] = dm["fallback"]
    f["bench.py device k_bdy_stream"] = dm["k_bdy_stream"]
    f["bench.py shuffled leg ms_per_step"] = j["shuffled_order"]["ms_per_step"]
    f["bench.py shuffled leg device total"] = j["shuffled_order"]["device_ms_total"]
    f["bench.py shuffled leg, records, ms_per_step"] = j["shuffled_order_records"]["ms_per_step"]
    f["bench.py groups leg ms per group (groups call)"] = j["groups"]["ms_per_group_groups_call"]
    f["bench.py groups leg ms per group (single calls)"] = j["groups"]["ms_per_group_single_calls"]
    j = result(os.path.join(d, f"groups_{b}{r}.json"))
    f["groups_only ms per group (groups call)"] = j["ms_per_group_groups_call"]
    f["groups_only ms per group (single calls)"] = j["ms_per_group_single_calls"]
    j = result(os.path.join(d, f"fallback_{b}{r}.json"))
    f["fallback_time ms_fallback (20 calls)"] = j["ms_fallback"]["median"]
    f["fallback_time ms_bdy (20 calls)"] = j["ms_bdy"]["median"]
    j = result(os.path.join(d, f"shuffled_{b}{r}.json"))
    f["sweep perm=shuffle cfg4 ms_sort (10 calls)"] = float(np.median(j["ms_sort"]))
    f["sweep perm=shuffle cfg4 ms_total (10 calls)"] = float(np.median(j["ms_total"]))
    return f


def main():
    d, rounds = sys.argv[1], int(sys.argv[2])
    runs = {b: [figures(d, b, r) for r in range(1, rounds + 1)] for b in ("parent", "new")}
    print(f"{'figure (ms)':52s}{'parent rounds':40s}{'new rounds':40s}{'parent-median':>14s}{'new-median':>11s}"
          "  band               verdict")
    bad = 0
    for k in runs["parent"][0]:
        p = [x[k] for x in runs["parent"]]
        n = [x[k] for x in runs["new"]]
        spread = max(p) - min(p)
        lo, hi = min(p) - spread, max(p) + spread
        m = float(np.median(n))
        verdict = "inside" if lo <= m <= hi else ("below (faster)" if m < lo else "ABOVE")
        bad += verdict == "ABOVE"
        print(f"{k:52s}{str([round(x, 4) for x in p]):40s}{str([round(x, 4) for x in n]):40s}"
              f"{float(np.median(p)):14.4f}{m:11.4f}  [{lo:.4f}, {hi:.4f}]  {verdict}")
    print(f"\n{bad} figure(s) above the parent's band")


if __name__ == "__main__":
    main()
