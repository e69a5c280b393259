"""Non-uniform probabilities, unequal node probabilities, a per-slot rho and
variable_probability on the HIP kernels (weight_cases.py).  The hot path's own copies
of the weighted arithmetic run here and nowhere else in the suite:

* S = 70: phx_lane_warm_fz1 with a full and a partial wavefront (the default loop,
  two-stage trees), k_small_xw (iterk_fused 0, and the three-stage tree, which is
  never fused), k_iter0_keep1 (the adopted Iter0 of the probabilities-only runs);
* S = 1,100: above k_small_xw's 1,024, k_xbar + k_update_w_seg unfused; fused, 18
  blocks with a ragged last one;
* S = 8,200: above 8,192 the adopted Iter0's expectations come from k_iter0_keep;
* S = 65,600: 1,025 blocks, the smallest batch on phx_lane_warm_fzr2.

The structures are those test_synth_structures_gpu.py compiles (the weights are data:
none appears in the emitted source), so each lane module is compiled once per process."""
import math
import time

import numpy as np
import pytest
import torch

import test_synth_structures as ts
import weight_cases as wc
from helpers import rel

pytestmark = pytest.mark.gpu

_COMPILED = set()


def first_context(gpu_lib, cs):
    """The structure's first context of this process pays its hipRTC compile: printed,
    not asserted."""
    if cs.key in _COMPILED:
        return
    _COMPILED.add(cs.key)
    t0 = time.perf_counter()
    first = ts.run(gpu_lib, None, cs.base, 0)[0]
    t1 = time.perf_counter()
    ts.run(gpu_lib, None, cs.base, 0)
    t2 = time.perf_counter()
    info = first._native.jit_info(first._ctx).decode()
    print("%s: %s; first context %.1f s, second %.2f s (the difference: the hipRTC compile, if this process "
          "had not compiled the structure yet)" % (cs.key, info, t1 - t0, t2 - t1))
    assert info.startswith("on: register-resident lane solver"), info


@pytest.mark.parametrize("mode", list(wc.MODES))
@pytest.mark.parametrize("key", wc.FAMILIES)
def test_weighted_case_gpu(gpu_lib, key, mode):
    """S = 70: checks B, C and D.  Two-stage trees: the default loop is fused
    (phx_lane_warm_fz1), iterk_fused 0 is not (k_small_xw); the three-stage tree is never
    fused and is held to the oracle and the recheck all the same.  Iter0 is deferred
    (k_iter0_keep1 forms the trivial bound) in the probabilities-only runs only; its
    sums equal phx_expect's on the kept objectives and statuses bit for bit."""
    cs = wc.case(key, mode)
    first_context(gpu_lib, cs)
    t0 = time.perf_counter()
    runs = wc.check_case(gpu_lib, None, cs, fused=cs.base.bf is None)[0]
    if mode == "p":
        # k_iter0_keep1's sums are phx_expect's (k_expect) bit for bit on what it kept
        left, again = runs[wc.ITERS]["iter0_exp"]
        print("%s/%s adopted Iter0 expectations %r, phx_expect %r" % (key, mode, left.tolist(), again.tolist()))
        assert np.array_equal(left, again)
    print("%s/%s: %.1f s" % (key, mode, time.perf_counter() - t0))


def test_s1100_fused_and_unfused_gpu(gpu_lib):
    """S = 1,100, probabilities and the rho setter: check C fused (18 blocks, the last
    ragged; last-arriving-block folds) and unfused (k_xbar + k_update_w_seg), check B on
    34 scenarios re-solved by the oracle, and the two loops against each other at
    check D's tolerances."""
    cs = wc.case("vary_all", "p_rho", S=1100)
    first_context(gpu_lib, cs)
    out = {}
    for name, so, fused in (("fused", None, True), ("unfused", {"iterk_fused": 0}, False)):
        t0 = time.perf_counter()
        runs = out[name] = wc.prefix_runs(gpu_lib, None, cs, so)
        last = runs[-1]
        assert last["stats"]["fused"] is fused and last["stats"]["iters"] == wc.ITERS, last["stats"]
        assert not last["deferred"]
        wc.check_prefix(cs, runs)
        wc.check_sampled_oracle(cs, last)
        print("S = 1100 %s: %.1f s, stats %s" % (name, time.perf_counter() - t0, last["stats"]))
    a, b = out["fused"][-1], out["unfused"][-1]
    errs = (rel(b["W"], a["W"]), rel(wc.xbar_SN(cs, b), wc.xbar_SN(cs, a)), rel(b["Eobj"], a["Eobj"]),
            rel(b["tb"], a["tb"]))
    print("S = 1100 unfused vs fused", ["%.1e" % e for e in errs])
    assert errs[0] < 1e-8 and errs[1] < 1e-9 and errs[2] < 1e-9 and errs[3] < 1e-9


def test_s8200_adopted_iter0_gpu(gpu_lib):
    """S = 8,200, probabilities only, default options: the adopted Iter0's sum p obj
    (k_iter0_keep: chunked, last-block fold) against math.fsum over the engine's own
    Iter0 objectives to 1e-12, its total probability likewise, and check C.  The three
    sums equal phx_expect's on the kept objectives and statuses bit for bit."""
    cs = wc.case("vary_all", "p", S=8200)
    first_context(gpu_lib, cs)
    runs = wc.prefix_runs(gpu_lib, None, cs, creator=cs.fam.batch_creator_fn(), K=3)
    wc.check_prefix(cs, runs)
    assert not runs[0]["deferred"]
    for k, r in enumerate(runs):
        if k:
            assert r["deferred"] and r["stats"]["fused"], r["stats"]
            # k_iter0_keep's sums (9 blocks) are phx_expect's (k_expect_part, k_expect_fold)
            # bit for bit on what it kept
            left, again = r["iter0_exp"]
            print("S = 8200 run %d adopted Iter0 expectations %r, phx_expect %r" % (k, left.tolist(), again.tolist()))
            assert np.array_equal(left, again), k
        tb = math.fsum(cs.p * r["iter0_obj"]) + math.fsum(cs.p * cs.fam.c0)
        print("S = 8200 run %d: deferred %s trivial bound %.15g host %.15g (relative %.1e) E1 - 1 = %.1e"
              % (k, r["deferred"], r["tb"], tb, abs(r["tb"] - tb) / max(1.0, abs(tb)), r["E1"] - 1.0))
        assert abs(r["tb"] - tb) <= 1e-12 * max(1.0, abs(tb)), k
        # (a sum of S terms in any order: at most (S + 2) u sum|term|, as reduction_cases.py derives)
        assert abs(r["E1"] - math.fsum(cs.p)) <= (cs.S + 2) * 2.0 ** -53, k
        # (the prefixes share one Iter0)
        assert np.array_equal(r["iter0_obj"], runs[0]["iter0_obj"]), k
    wc.check_sampled_oracle(cs, runs[-1])


def test_s65600_two_waves_per_simd_gpu(gpu_lib):
    """S = 65,600 through a vectorised batch_creator: 1,025 blocks, one more than the
    1,024 SIMDs, so the fused loop takes phx_lane_warm_fzr2.  rho is written in one
    device copy after Iter0 (PublishRho overrides no in-loop hook: the device loop
    runs).  Check C, the sampled oracle re-solve, fused, every lane certified."""
    cs = wc.case("vary_all", "p_rho", S=65600)
    first_context(gpu_lib, cs)
    t0 = time.perf_counter()
    runs = wc.prefix_runs(gpu_lib, None, cs, creator=cs.fam.batch_creator_fn(), extension=True, K=3)
    last = runs[-1]
    print("S = 65600: 4 runs in %.1f s, stats %s" % (time.perf_counter() - t0, last["stats"]))
    assert last["stats"]["fused"] and last["stats"]["iters"] == 3 and last["certified"], last["stats"]
    wc.check_prefix(cs, runs)
    wc.check_sampled_oracle(cs, last)
    del runs
    torch.cuda.empty_cache()


@pytest.mark.parametrize("zero", [None, (5, 1)])
def test_variable_probability_gpu(gpu_lib, zero):
    """variable_probability on the kernels (the host loop's phx_xbar / phx_update_w under
    per-slot probabilities and the W mask): S = 70, as is and with one zero entry."""
    cs = wc.case("vary_all", "p")
    first_context(gpu_lib, cs)
    wc.check_variable_probability(gpu_lib, None, zero=zero)
