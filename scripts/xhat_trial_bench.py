"""Time one scenario-donor xhat trial against the x-bar-style path it replaces.

farmer, one GPU.  A trial fixes every scenario's nonants at one donor
scenario's Iter0 values and re-solves the recourse problems:

  new     XhatBase._try_one(restore_nonants=False): phx_donor_gather ->
          phx_fix_nonants -> the fixed-nonant lane module -> infeas_prob /
          Eobjective
  parent  the same candidate through SPOpt._fix_nonants + solve_loop +
          infeas_prob + Eobjective (what XhatXbar.xhat_tryit does: host bound
          arrays, phx_set_bounds, the generic path), and through
          Xhat_Eval.evaluate (the same plus its per-scenario objective dict)

Each figure is the median over --trials distinct donors, device-synchronised
around every trial, after two warm-up trials; the paths alternate --pairs
times.  --no-fix-lane sets PHX_FIX_LANE=0 (the device-side fixing with the
generic solve: what the lane module itself contributes).  Prints one JSON line.
The fixed module's register / scratch figures come from
scripts/fixed_module_resources.py (an offline compile, no GPU needed).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scens", type=int, default=100000)
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--no-fix-lane", action="store_true")
    ap.add_argument("--skip-parent", action="store_true")
    a = ap.parse_args()
    if a.no_fix_lane:
        os.environ["PHX_FIX_LANE"] = "0"
    import torch
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.extensions.xhatbase import XhatBase
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval

    S = a.scens
    opts = {"iter0_solver_options": None, "iterk_solver_options": None, "display_timing": False,
            "solver_name": "phx", "verbose": False, "solver_options": None}
    ev = Xhat_Eval(opts, farmer.scenario_names_creator(S), farmer.scenario_creator,
                   scenario_creator_kwargs={"num_scens": S})
    ev.solve_loop()
    ev._save_original_nonants()
    ev._save_nonants()
    xb = XhatBase(ev)
    rng = np.random.default_rng(7)
    donors = [int(k) for k in rng.choice(S, size=a.trials + 2, replace=False)]
    sync = torch.cuda.synchronize

    def timed(fn, ks):
        out = []
        for k in ks:
            sync()
            t0 = time.perf_counter()
            v = fn(k)
            sync()
            out.append((time.perf_counter() - t0) * 1e3)
            assert v is not None
        return out

    def new(k):
        return xb._try_one({"ROOT": "scen%d" % k}, restore_nonants=False)

    def parent_tryit(k):
        ev._fix_nonants({"ROOT": ev.nonant_cache[k]})
        ev.solve_loop()
        if ev.infeas_prob() != 0.:
            return None
        return ev.Eobjective()

    def parent_evaluate(k):
        return ev.evaluate({"ROOT": ev.nonant_cache[k]})

    res = {"scens": S, "trials": a.trials, "fix_lane": not a.no_fix_lane, "pairs": []}
    vals = {}
    for p in range(a.pairs):
        rec = {}
        timed(new, donors[:2])
        t = timed(new, donors[2:])
        rec["new_ms"] = float(np.median(t))
        rec["new_min_max_ms"] = [float(min(t)), float(max(t))]
        rec["new_stats"] = {k: ev.solve_stats[-1][k] for k in ("lane_certified", "stragglers", "lane_warm_certified")}
        vals["new"] = new(donors[2])
        if not a.skip_parent:
            timed(parent_tryit, donors[:2])
            t = timed(parent_tryit, donors[2:])
            rec["parent_tryit_ms"] = float(np.median(t))
            rec["parent_tryit_min_max_ms"] = [float(min(t)), float(max(t))]
            vals["parent"] = parent_tryit(donors[2])
            t = timed(parent_evaluate, donors[2:2 + max(3, a.trials // 4)])
            rec["parent_evaluate_ms"] = float(np.median(t))
        res["pairs"].append(rec)
    res["jit_info"] = ev._native.jit_info(ev._ctx).decode()
    if "parent" in vals:
        res["same_value_rel"] = abs(vals["new"] - vals["parent"]) / max(1.0, abs(vals["parent"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
