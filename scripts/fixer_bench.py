"""Measurements of the Fixer's device path, farmer on one GPU,
host loop: per-iteration solve time on the PH lane module, on the fixed-subset
module with one and two slots fixed, and through the generic path
(PHX_FIX_LANE=0); the wall time of a subset-module build; the time of
phx_fixer_step plus the pinned-word copy.  Each solve is timed by a host clock
around solve_loop + a device synchronise; lane_warm_ms is the library's own
event pair around the warm pass.  One JSON line per measurement.

    python scripts/fixer_bench.py --scens 100000 --iters 10 > profiles/fixer_bench.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpisppy_amd  # noqa: E402,F401
from mpisppy_amd.examples import farmer  # noqa: E402
from mpisppy_amd.extensions.fixer import Fixer, Fixer_tuple  # noqa: E402
from mpisppy_amd.opt.ph import PH  # noqa: E402


def never(s):
    """Tuples that count but never fix (no lag set)."""
    return [], [Fixer_tuple(v, th=1.0) for v in s._mpisppy_data.nonant_indices.values()]


def make(S, fct=never, iters=1000):
    opts = {"solver_name": "phx", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": 1e-8, "verbose": False,
            "display_progress": False, "iter0_solver_options": {}, "iterk_solver_options": {},
            "fixeroptions": {"verbose": False, "boundtol": 1e-2, "id_fix_list_fct": fct}}
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator,
              scenario_creator_kwargs={"num_scens": S}, extensions=Fixer, _device="cuda:0")


def ph_steps(ph, n):
    """n PH iterations of the host loop without the extension; per-solve (wall ms, lane_warm_ms, stragglers)."""
    out = []
    for _ in range(n):
        ph.Compute_Xbar(False)
        ph.Update_W(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ph.solve_loop(solver_options=ph.current_solver_options)
        ph._settle()
        torch.cuda.synchronize()
        st = ph.solve_stats[-1]
        out.append(((time.perf_counter() - t0) * 1e3, st["lane_warm_ms"], st["stragglers"], st["lane_certified"],
                    st["not_optimal"]))
    return out


def report(what, rows, **kw):
    a = np.array(rows, dtype=np.float64)
    rec = {"what": what, "solves": len(rows), "wall_ms_median": float(np.median(a[:, 0])),
           "wall_ms_min": float(a[:, 0].min()), "wall_ms_first": float(a[0, 0]),
           "lane_warm_ms_median": float(np.median(a[:, 1])), "stragglers": int(a[:, 2].sum()),
           "lane_certified_min": int(a[:, 3].min()), "not_optimal": int(a[:, 4].sum())}
    rec.update(kw)
    print(json.dumps(rec), flush=True)


def fix(ph, slots):
    """Force the slots fixed at their x-bar; returns the call's wall time (ms, synchronised)."""
    how = torch.zeros(ph.NNS, dtype=torch.int32, device=ph.device)
    how[list(slots)] = 1
    vals = ph._xbar_node[:ph.NNS].clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ph._fix_where_device(how, vals)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scens", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    S, K = a.scens, a.iters
    ph = make(S)
    ph.PH_Prep()
    ph.Iter0()
    ph_steps(ph, 5)                                               # warm-up
    report("a: PH module, nothing fixed", ph_steps(ph, K), S=S)
    # e: the decision step and its pinned word, per call
    ext = ph.extobject
    ext._step(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        ext._step(False)
    print(json.dumps({"what": "e: phx_fixer_step + pinned word + stream wait, per call",
                      "us": (time.perf_counter() - t0) / 200 * 1e6, "NNS": int(ph.NNS)}), flush=True)
    ms = fix(ph, [2])
    info = ph._native.jit_info(ph._ctx).decode().split("; ")[-1]
    rows = ph_steps(ph, K + 1)
    report("b1: subset module, slot 2 fixed", rows[1:], S=S, fix_call_ms=ms, first_cold_solve_ms=rows[0][0], info=info)
    ms = fix(ph, [1, 2])
    info = ph._native.jit_info(ph._ctx).decode().split("; ")[-1]
    rows = ph_steps(ph, K + 1)
    report("b2: subset module, slots 1 and 2 fixed", rows[1:], S=S, fix_call_ms=ms, first_cold_solve_ms=rows[0][0],
           info=info)
    ms = fix(ph, [2])
    print(json.dumps({"what": "d': back to the {2} mask (compile cached by source text)", "fix_call_ms": ms}),
          flush=True)
    del ph
    os.environ["PHX_FIX_LANE"] = "0"
    ph = make(S)
    ph.PH_Prep()
    ph.Iter0()
    ph_steps(ph, 5)
    ms = fix(ph, [2])
    info = ph._native.jit_info(ph._ctx).decode().split("; ")[-1]
    rows = ph_steps(ph, 4)
    report("c: generic path (PHX_FIX_LANE=0), slot 2 fixed", rows[1:], S=S, fix_call_ms=ms, info=info)
    del os.environ["PHX_FIX_LANE"]
    # d: builds in the farmer-3 run of the tests (th 2.2, nb 3, 25 iterations)
    builds = []

    def fct(s):
        return [], [Fixer_tuple(v, th=2.2, nb=3) for v in s._mpisppy_data.nonant_indices.values()]
    p3 = make(3, fct, iters=25)
    orig = p3._fix_where_device

    def timed(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        orig(*args, **kw)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    p3._fix_where_device = timed
    p3.ph_main()
    print(json.dumps({"what": "d: farmer-3 run, fix calls (each a subset-module build)", "calls": len(builds),
                      "ms": builds, "events": p3.extobject.events}), flush=True)


if __name__ == "__main__":
    main()
