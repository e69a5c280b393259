"""Measurements of NormRhoUpdater inside the device loop, farmer
on one GPU, rho = 1, default norm_rho_options.

  --iter S[,S...]   wall time per PH iteration: after Iter0 and 5 warm-up
                    iterations, 20 iterations timed by a host clock between two
                    device synchronisations.  Alternating pairs (--pairs, 5): the
                    host loop with the updater (native_loop 0) and the device
                    loop (phx_iterk_norm_rho); the median and every sample.
  --fixed S[,S...]  the same window for the fixed-rho device loop (no extension;
                    phx_iterk's fused mode): the regression figure.  --root names
                    another checkout of the project to import instead of this one
                    (the parent commit, built); run the two in alternation.
  --conv S          PH iterations and seconds (host clock around ph_main, which
                    ends in a device synchronise) to conv < 1e-4: the updater on
                    the host loop and on the device loop, alternating, twice.

One JSON line per measurement.

    python scripts/iterk_rho_bench.py --iter 100000,1000000 --conv 100000 --fixed 100000
"""
import argparse
import gc
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--iter", default="")
ap.add_argument("--fixed", default="")
ap.add_argument("--conv", type=int, default=0)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--timed", type=int, default=20)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpisppy_amd  # noqa: E402,F401
from mpisppy_amd.examples import farmer  # noqa: E402
from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater  # noqa: E402
from mpisppy_amd.opt.ph import PH  # noqa: E402


def make(S, iters, ext, host, convthresh):
    so = {"native_loop": 0} if host else {}
    opts = {"solver_name": "phx", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": convthresh,
            "verbose": False, "display_progress": False, "iter0_solver_options": dict(so),
            "iterk_solver_options": dict(so)}
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator,
              scenario_creator_kwargs={"num_scens": S}, extensions=ext, _device="cuda:0")


def window(ph):
    """microseconds per PH iteration over ARGS.timed iterations after Iter0 and ARGS.warm iterations"""
    ph.PH_Prep()
    ph.subproblem_creation(False)
    if ph.extensions is not None:
        ph.extobject._have_prev = False
    ph.options["PHIterLimit"] = ARGS.warm
    ph.Iter0()
    ph.iterk_loop()
    ph._settle()
    ph.options["PHIterLimit"] = ARGS.timed
    gc.collect()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ph.iterk_loop()
    ph._settle()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    assert ph._PHIter == ARGS.timed
    return dt / ARGS.timed * 1e6


def stats(us):
    us = np.array(us)
    return {"us_median": float(np.median(us)), "us_min": float(us.min()), "us_max": float(us.max()),
            "samples_us": [round(float(v), 2) for v in us]}


def per_iteration(S):
    host = make(S, ARGS.timed, NormRhoUpdater, True, 0.0)
    dev = make(S, ARGS.timed, NormRhoUpdater, False, 0.0)
    window(host), window(dev)                        # (code objects, lane module, buffers: not measurements)
    h, d = [], []
    for _ in range(ARGS.pairs):
        h.append(window(host))
        d.append(window(dev))
    assert not hasattr(host, "iterk_stats") and dev.iterk_stats["fused"] is False
    assert dev.iterk_stats["rho_updates"] == ARGS.timed
    # the two loops walked the same trajectory (the last window's state)
    same = bool(torch.equal(host._rho, dev._rho) and torch.equal(host._W, dev._W))
    base = {"S": S, "warm": ARGS.warm, "timed": ARGS.timed, "pairs": ARGS.pairs, "same_rho_and_W": same}
    print(json.dumps(dict(base, what="NormRhoUpdater, host loop, per PH iteration", **stats(h))), flush=True)
    print(json.dumps(dict(base, what="NormRhoUpdater, device loop, per PH iteration", **stats(d))), flush=True)


def fixed_rho(S):
    ph = make(S, ARGS.timed, None, False, 0.0)
    window(ph)
    us = [window(ph) for _ in range(ARGS.pairs)]
    print(json.dumps(dict({"what": "fixed rho, device loop, per PH iteration", "root": os.path.abspath(ARGS.root),
                           "S": S, "warm": ARGS.warm, "timed": ARGS.timed, "fused": ph.iterk_stats["fused"]},
                          **stats(us))), flush=True)


def to_conv(S, host, limit=6000):
    ph = make(S, limit, NormRhoUpdater, host, 1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    conv, Eobj, tb = ph.ph_main()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "NormRhoUpdater to conv < 1e-4, %s loop" % ("host" if host else "device"), "S": S,
                      "iterations": int(ph._PHIter), "seconds": dt, "conv": float(conv), "converged": bool(conv < 1e-4),
                      "Eobj": float(Eobj), "rho_scen0": ph._rho.view(-1, ph._S)[:, 0].cpu().tolist(),
                      "rho_updates": getattr(ph, "iterk_stats", {}).get("rho_updates")}), flush=True)
    return int(ph._PHIter)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    for S in [int(v) for v in ARGS.iter.split(",") if v]:
        per_iteration(S)
    for S in [int(v) for v in ARGS.fixed.split(",") if v]:
        fixed_rho(S)
    if ARGS.conv:
        its = []
        for rep in range(2):
            its.append((to_conv(ARGS.conv, True), to_conv(ARGS.conv, False)))
        assert all(a == b for a, b in its), its


if __name__ == "__main__":
    main()
