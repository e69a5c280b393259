"""Measurements of cost-proportional rho, farmer on one GPU.

  --update S[,S...]   one full rho update (Find_Rho.compute_rho_device: the
                      scenario denominators, the statistics, two all-reduces --
                      none on one rank --, the rule and the broadcast) timed by a
                      device event pair around each call, after warm-up: median,
                      min, max over --reps calls; its launches and algorithmic
                      bytes.  Under `rocprofv3 --kernel-trace --stats` the same
                      mode gives the kernels' own times (a run of its own).
  --conv S            PH iterations and seconds (host clock around ph_main, which
                      ends in a device synchronise) to conv < 1e-4 from rho = 1:
                      fixed rho on the device loop and on the host loop,
                      NormRhoUpdater, Gradient_extension at order_stat 0.4 and 0.5.

One JSON line per measurement.

    python scripts/cost_rho_bench.py --update 12500,100000,1000000 --conv 100000
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
from mpisppy_amd.extensions.extension import Extension  # noqa: E402
from mpisppy_amd.extensions.gradient_extension import Gradient_extension  # noqa: E402
from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater  # noqa: E402
from mpisppy_amd.opt.ph import PH  # noqa: E402
from mpisppy_amd.utils.find_rho import Find_Rho, rho_cfg  # noqa: E402
from mpisppy_amd.utils.gradient import Find_Grad  # noqa: E402

HOST = {"native_loop": 0}


class HostLoop(Extension):
    """a hook that does nothing: the host loop as it is without an updater"""

    def miditer(self):
        pass


def make(S, iters, ext=None, host=False, order_stat=0.4, convthresh=1e-4):
    so = dict(HOST) if host else {}
    opts = {"solver_name": "phx", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": convthresh,
            "verbose": False, "display_progress": False, "iter0_solver_options": dict(so),
            "iterk_solver_options": dict(so),
            "gradient_extension_options": {"cfg": rho_cfg(order_stat=order_stat)}}
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator,
              scenario_creator_kwargs={"num_scens": S}, extensions=ext, _device="cuda:0")


def update_cost(S, reps):
    ph = make(S, 5, ext=HostLoop, host=True, convthresh=0.0)
    ph.ph_main()                                           # x, x-bar of a run in progress
    fr = Find_Rho(ph, rho_cfg(order_stat=0.4))
    cost_t = Find_Grad(ph, rho_cfg()).grad_cost_device()
    for _ in range(10):
        fr.compute_rho_device(cost_t)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fr.compute_rho_device(cost_t)
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    N = ph.batch.nonant.N
    # k_cost_rho_denom reads x's nonant rows and xbar_idx and writes [S]; k_cost_rho_stats reads
    # cost and [S]; k_cost_rho_bcast reads xbar_idx and writes rho
    stats_bytes = N * S * 8 + S * 8
    total = (N * S * (8 + 4) + S * 8) + stats_bytes + N * S * (4 + 8)
    print(json.dumps({"what": "one rho update (scenario-dependent denominator)", "S": S, "N": N, "reps": reps,
                      "us_median": float(np.median(us)), "us_min": float(us.min()), "us_max": float(us.max()),
                      "us_p10": float(np.percentile(us, 10)), "us_p90": float(np.percentile(us, 90)),
                      "launches": 4, "algorithmic_bytes": int(total), "stats_kernel_bytes": int(stats_bytes),
                      "kept": int(fr.kept.sum().item()), "tiles": len(ph._tiles)}), flush=True)


def to_conv(S, what, ext, host, order_stat=0.4, limit=6000):
    ph = make(S, limit, ext=ext, host=host, order_stat=order_stat)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    conv, Eobj, tb = ph.ph_main()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rho = ph._rho.view(-1, ph._S)[:, 0].cpu().tolist()
    rec = {"what": what, "S": S, "iterations": int(ph._PHIter), "seconds": dt, "conv": float(conv),
           "converged": bool(conv < 1e-4), "Eobj": float(Eobj), "rho_scen0": rho}
    if isinstance(getattr(ph, "extobject", None), Gradient_extension):
        d = ph.extobject.dual_conv_cache
        fired = [k for k in range(2, len(d)) if d[k - 1] != 0 and abs((d[k - 1] - d[k]) / d[k - 1]) <= 0.05]
        rec["rho_updates"] = len(fired)
        rec["first_updates"] = fired[:8]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--update", default="")
    ap.add_argument("--conv", type=int, default=0)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for S in [int(v) for v in a.update.split(",") if v]:
        update_cost(S, a.reps)
    if a.conv:
        S = a.conv
        to_conv(S, "warm-up (fixed rho, device loop; not a measurement)", None, False, limit=200)
        for rep in range(2):
            to_conv(S, "fixed rho = 1, device loop", None, False)
            to_conv(S, "fixed rho = 1, host loop (no-op hook)", HostLoop, True)
            to_conv(S, "NormRhoUpdater, default options", NormRhoUpdater, True)
            to_conv(S, "Gradient_extension, order_stat 0.4", Gradient_extension, True, 0.4)
            to_conv(S, "Gradient_extension, order_stat 0.5", Gradient_extension, True, 0.5)


if __name__ == "__main__":
    main()
