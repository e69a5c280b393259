"""Direct checks of the cost-proportional-rho entry points (phx_cost_rho_stats,
phx_cost_rho_apply, phx_w_absdiff) and of the host layer on top of them
(utils/find_rho.py, utils/gradient.py, extensions/gradient_extension.py).  The
PH objects, values, bounds and sentinel conventions are those of
reduction_cases.py (imported, not copied); test_cost_rho.py runs each check on
the host emulation, test_cost_rho_gpu.py on the HIP kernels.

phx_cost_rho_stats: the candidates ``|cost| / d`` are formed in numpy (one IEEE
division, as the kernel's), so count, max, -min and the per-scenario
denominators must be equal bit for bit; the sum is compared with ``math.fsum``
under reduction_cases' any-order bound ``(n + 2) u sum|term|`` (derived there;
u = 2**-53).  An entry whose candidates include +inf must read +inf exactly.
Every call is made twice into sentinel-filled buffers and must repeat bit for
bit.

phx_cost_rho_apply, exact comparison: min, mean and max are dyadic with
``mean - min`` and ``max - mean`` powers of two and count a power of two, so
``sum / count``, ``2 mean - max`` and the product ``alpha*2*(...)`` are exact
(for alpha = 0.4 and 0.6 too: a scaling by a power of two) and the final
addition rounds once, to the same value whether or not the compiler contracts
it with the product.  On random inputs: ``8 u (|min| + |mean| + |max|)``, at
most four roundings of intermediates no larger than twice that sum.

The bounds were fixed against the host emulation only.  Worst error / bound
there: statistics 0.21 per entry (T3u), slices 0.28 on their own and added up
(T3u); the rule on random inputs 0 (the host does not contract, as numpy); W
difference 0.017 (N=1, S=1023).  First measurement on the MI355X: statistics
0.21 (T3u; 0.027 at most in the one-node cases), slices 0.031 on their own and
combined; the rule on random inputs 0.12 (S65: the product and the addition are
contracted there); W difference 0.0018.
"""
import csv
import ctypes
import math
import os
import types

import numpy as np
import torch

from mpisppy_amd import _native
from mpisppy_amd.examples import farmer, hydro
from mpisppy_amd.extensions.gradient_extension import Gradient_extension
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.utils import sputils
from mpisppy_amd.utils.find_rho import Find_Rho, Set_Rho, rho_cfg
from mpisppy_amd.utils.gradient import Find_Grad
from helpers import ph_options, rel
from oracle import models as om, ph as oph
import reduction_cases as rc
from reduction_cases import build_ph, values, _ratio, _sum_ref, T3U, XBAR_CASES, SLICE_CASES, EXPECT_SIZES
from residual_cases import _dev, _one_slot_creator

U = rc.U
SENTINEL = rc.SENTINEL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = math.inf


# ---------------------------------------------------------------- phx_cost_rho_stats
STATS_CASES = {}
for _S in (1, 63, 64, 65, 1024, 1025, 1300):
    for _N in (1, 8):
        STATS_CASES["S%d-N%d" % (_S, _N)] = dict(k1=_N, S=_S)
STATS_CASES["T3u"] = dict(T3U)
for _c in ("300-nodes", "S1300-N70"):
    STATS_CASES[_c] = dict(XBAR_CASES[_c])
ZERO_DENOM_CASE, ZERO_COST_CASE = "S65-N8", "S1300-N8"


def scen_denom_reference(xbar_idx, X, xbar):
    """max over every slot of max(|x - xbar|, 2 (x - xbar)^2): one scalar per scenario"""
    diff = X - xbar[xbar_idx]
    return np.max(np.maximum(np.abs(diff), 2 * np.square(diff)), axis=0)


def candidates(xbar_idx, cost, X, xbar, denom_node):
    """(N, S) |cost| / d, +inf where d == 0; and the scenario denominators (None with denom_node)"""
    if denom_node is not None:
        sd, d = None, denom_node[xbar_idx]
    else:
        sd = scen_denom_reference(xbar_idx, X, xbar)
        d = np.broadcast_to(sd[None, :], cost.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, INF, np.abs(cost) / d)
    return r, sd


def stats_reference(xbar_idx, NNS, r):
    """[sum | count | max | -min] per entry over the given scenarios (absent
    entries 0, 0, -inf, -inf), the bound of the sum and the present mask"""
    ref = np.concatenate([np.zeros(2 * NNS), np.full(2 * NNS, -INF)])
    bnd = np.zeros(NNS)
    present = np.zeros(NNS, dtype=bool)
    for j in range(xbar_idx.shape[0]):
        idx = xbar_idx[j]
        for e in np.unique(idx):
            t = r[j, idx == e]
            if np.isfinite(t).all():
                ref[e], bnd[e] = _sum_ref(t)
            else:
                ref[e], bnd[e] = INF, 0.0
            ref[NNS + e], ref[2 * NNS + e], ref[3 * NNS + e] = t.size, t.max(), -t.min()
            present[e] = True
    return ref, bnd, present


def _stats_call(lib, ph, cost_t, xbar_t, denom_t, prefill, fill=SENTINEL):
    """phx_cost_rho_stats into buffers of the test's own, prefilled: (out [4 NNS], scen_denom [S])"""
    NNS, S = ph.NNS, ph._S
    out_t = _dev(ph, prefill)
    assert out_t.numel() == 4 * NNS + 1
    sd_t = torch.full((S + 1,), fill, dtype=torch.float64, device=ph.device)
    part_t = torch.full((2 * max(int(ph._tree.npart), 1) + 1,), fill, dtype=torch.float64, device=ph.device)
    lib.check(ph._ctx, lib.cost_rho_stats(ph._ctx, ctypes.byref(ph._tree), cost_t.data_ptr(), ph._x.data_ptr(),
                                          xbar_t.data_ptr(), ph._xbar_idx_t.data_ptr(),
                                          denom_t.data_ptr() if denom_t is not None else None,
                                          part_t.data_ptr(), sd_t.data_ptr(), out_t.data_ptr(), ph._stream()),
              "cost_rho_stats")
    got, sd, part = rc._get(out_t), rc._get(sd_t), rc._get(part_t)
    assert got[4 * NNS] == prefill[4 * NNS], "wrote past out[4 NNS]"
    assert sd[S] == fill, "wrote past scen_denom_out[S]"
    assert part[-1] == fill, "wrote past partial[2 npart]"
    if denom_t is not None:
        assert np.all(sd == fill), "scen_denom_out written with a node denominator"
    return got[:4 * NNS], sd[:S]


def _compare_stats(got, ref, bnd, NNS, tag):
    """count, max, -min equal; an infinite sum equal, a finite one within its bound"""
    assert np.array_equal(got[NNS:], ref[NNS:]), (tag, got[NNS:], ref[NNS:])
    fin = np.isfinite(ref[:NNS])
    assert np.array_equal(got[:NNS][~fin], ref[:NNS][~fin]), tag
    r = _ratio(got[:NNS][fin], ref[:NNS][fin], bnd[fin])
    assert r <= 1.0, (tag, r)
    return r


def _stats_inputs(rng, N, S, NNS, idx, case=None):
    X, xbar, cost = values(rng, (N, S)), values(rng, NNS), values(rng, (N, S))
    denom_node = rng.uniform(0.5, 50.0, size=NNS)
    if case == ZERO_DENOM_CASE:
        X[:, 7] = xbar[idx[:, 7]]                  # x == xbar in every slot: d = 0, r = +inf
        cost[3, 7] = 0.0                           # ... whatever the cost
        denom_node[2] = 0.0
    if case == ZERO_COST_CASE:
        cost[2, 100] = 0.0                         # r = 0: the entry's minimum
    return X, xbar, cost, denom_node


def check_stats(lib, device, case):
    ph = build_ph(lib, device, **dict(STATS_CASES[case]))
    N, S, NNS = ph.batch.nonant.N, ph._S, ph.NNS
    idx = ph._xbar_idx
    rng = np.random.default_rng(6000 + S + 7 * N)
    X, xbar, cost, denom_node = _stats_inputs(rng, N, S, NNS, idx, case)
    rc._fill_x_pc(ph, X, np.ones((N, S)))
    xbar_t, cost_t = _dev(ph, xbar), _dev(ph, cost)
    worst = 0.0
    for dn in (None, denom_node):
        denom_t = None if dn is None else _dev(ph, dn)
        r, sd = candidates(idx, cost, X, xbar, dn)
        ref, bnd, present = stats_reference(idx, NNS, r)
        assert present.all()
        got, gsd = _stats_call(lib, ph, cost_t, xbar_t, denom_t, np.full(4 * NNS + 1, SENTINEL))
        if dn is None:
            assert np.array_equal(gsd, sd), case
        if case == ZERO_DENOM_CASE:
            assert np.isinf(ref[:NNS]).any() and not np.isnan(got).any()
            if dn is None:
                assert sd[7] == 0.0 and np.all(got[2 * NNS:3 * NNS] == INF)
        if case == ZERO_COST_CASE:
            assert ref[3 * NNS + idx[2, 100]] == 0.0
        worst = max(worst, _compare_stats(got, ref, bnd, NNS, (case, dn is None)))
        again, asd = _stats_call(lib, ph, cost_t, xbar_t, denom_t, np.full(4 * NNS + 1, -SENTINEL), -SENTINEL)
        assert np.array_equal(got, again) and (dn is not None or np.array_equal(gsd, asd)), case
    print("[cost_rho_stats %s] S=%d N=%d NNS=%d tiles=%d worst error/bound = %.3g"
          % (case, S, N, NNS, len(ph._tiles), worst))
    return worst


def check_stats_slices(lib, device, case):
    """Each slice as one rank of several sees it: entries of absent nodes read
    exactly 0, 0, -inf, -inf, also on a second call into a buffer that holds
    all-reduced values, and the slices SUM / MAX-combined give the whole."""
    cfg, slices = SLICE_CASES[case]
    S = int(sum(cfg["counts"]))
    N = cfg["k1"] + cfg["k2"]
    rng = np.random.default_rng(277 + S)
    whole = build_ph(lib, device, **cfg)
    NNS = whole.NNS
    X, xbar, cost, denom_node = _stats_inputs(rng, N, S, NNS, whole._xbar_idx)
    worst = wt = 0.0
    for dn in (None, denom_node):
        r, _ = candidates(whole._xbar_idx, cost, X, xbar, dn)
        gref, gbnd, gpresent = stats_reference(whole._xbar_idx, NNS, r)
        assert gpresent.all()
        runs, gots = [], []
        for lo, hi in slices:
            ph = build_ph(lib, device, lo=lo, hi=hi, **cfg)
            assert ph.NNS == NNS and ph._tree.nnodes_cover < NNS
            rc._fill_x_pc(ph, X[:, lo:hi], np.ones((N, hi - lo)))
            xbar_t, cost_t = _dev(ph, xbar), _dev(ph, cost[:, lo:hi])
            denom_t = None if dn is None else _dev(ph, dn)
            ref, bnd, present = stats_reference(ph._xbar_idx, NNS, r[:, lo:hi])
            assert not present.all()
            got, _ = _stats_call(lib, ph, cost_t, xbar_t, denom_t, np.full(4 * NNS + 1, SENTINEL))
            absent = np.tile(~present, 4)
            assert np.array_equal(got[absent], ref[absent]), (
                "slice [%d,%d): entries of absent nodes are not 0, 0, -inf, -inf" % (lo, hi))
            worst = max(worst, _compare_stats(got, ref, bnd, NNS, (case, lo, hi)))
            runs.append((ph, xbar_t, cost_t, denom_t))
            gots.append(got)
        total = np.concatenate([np.sum([g[:2 * NNS] for g in gots], axis=0),
                                np.max([g[2 * NNS:] for g in gots], axis=0)])
        wt = max(wt, _compare_stats(total, gref, gbnd, NNS, (case, "combined")))
        # the second call of a host loop: the buffer holds the all-reduced values
        for (ph, xbar_t, cost_t, denom_t), got in zip(runs, gots):
            again, _ = _stats_call(lib, ph, cost_t, xbar_t, denom_t, np.concatenate([total, [SENTINEL]]))
            assert np.array_equal(again, got), "stale statistics were kept or combined again"
    print("[cost_rho_stats slices %s] worst error/bound: slices %.3g, combined %.3g" % (case, worst, wt))
    return worst, wt


# ---------------------------------------------------------------- phx_cost_rho_apply
ALPHAS = (0.0, 0.4, 0.5, 0.6, 1.0)
APPLY_CASES = {"S%d" % _S: dict(k1=6, S=_S) for _S in (1, 65, 1025)}
APPLY_CASES["T3u-slice"] = dict(T3U, lo=0, hi=200)           # no local scenario for the last node


def order_stat_reference(alpha, stats, NNS):
    """Find_Rho._order_stat on the statistics, in float64 with its association: (rho_e, kept)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        cnt = stats[NNS:2 * NNS]
        mean, hi, lo = stats[:NNS] / cnt, stats[2 * NNS:3 * NNS], -stats[3 * NNS:]
        if alpha == 0.5:
            r = mean
        elif alpha < 0.5:
            r = lo + alpha * 2 * (mean - lo)
        else:
            r = (2 * mean - hi) + alpha * 2 * (hi - mean)
    kept = ~((cnt > 0) & np.isfinite(r))
    return r, kept, (np.abs(lo) + np.abs(mean) + np.abs(hi))


def _apply_call(lib, ph, alpha, stats, rho):
    NNS = ph.NNS
    stats_t, rho_t = _dev(ph, stats), _dev(ph, rho)
    rn_t = torch.full((NNS + 1,), SENTINEL, dtype=torch.float64, device=ph.device)
    kept_t = torch.full((NNS + 1,), 9, dtype=torch.int32, device=ph.device)
    o = _native.CostRhoOpts()
    o.order_stat = alpha
    lib.check(ph._ctx, lib.cost_rho_apply(ph._ctx, ctypes.byref(ph._tree), ctypes.byref(o), stats_t.data_ptr(),
                                          ph._xbar_idx_t.data_ptr(), rho_t.data_ptr(), rn_t.data_ptr(),
                                          kept_t.data_ptr(), ph._stream()), "cost_rho_apply")
    rn, kept = rc._get(rn_t), rc._get(kept_t)
    assert rn[NNS] == SENTINEL and kept[NNS] == 9
    assert np.array_equal(rc._get(stats_t), stats, equal_nan=True)
    return rn[:NNS], kept[:NNS], rc._get(rho_t).reshape(rho.shape)


def check_apply(lib, device, case):
    ph = build_ph(lib, device, **dict(APPLY_CASES[case]))
    N, S, NNS = ph.batch.nonant.N, ph._S, ph.NNS
    idx = ph._xbar_idx
    rng = np.random.default_rng(7000 + S)
    rho = rng.uniform(0.1, 10.0, size=(N, S))                  # non-uniform incoming rho
    # exact inputs: dyadic min, mean - min and max - mean powers of two, count a power of two
    lo = np.array([0.25 * (e % 9) for e in range(NNS)])
    mean = lo + 2.0 ** np.array([(e % 5) - 2 for e in range(NNS)])
    hi = mean + 2.0 ** np.array([(e % 4) - 1 for e in range(NNS)])
    cnt = 2.0 ** np.array([e % 4 for e in range(NNS)])
    lo[0] = mean[0] = hi[0] = 0.0                              # a zero cost in every scenario: rho 0
    stats = np.concatenate([mean * cnt, cnt, hi, -lo])
    special = {}
    if NNS >= 6:
        stats[1], stats[NNS + 1], stats[2 * NNS + 1], stats[3 * NNS + 1] = 0.0, 0.0, -INF, -INF   # count == 0
        stats[3], stats[2 * NNS + 3] = INF, INF                                                   # an inf candidate
        stats[5] = math.nan                                                                       # a nan
        special = {1, 3, 5}
    worst = 0.0
    for alpha in ALPHAS:
        ref, kept, _ = order_stat_reference(alpha, stats, NNS)
        assert set(np.nonzero(kept)[0]) == special
        rn, gk, new_rho = _apply_call(lib, ph, alpha, stats, rho)
        assert np.array_equal(gk, kept.astype(np.int32)), (case, alpha)
        assert np.array_equal(rn[~kept], ref[~kept]), (case, alpha, rn, ref)
        assert not np.isfinite(rn[kept]).any()
        want = np.where(kept[idx], rho, ref[idx])
        assert np.array_equal(new_rho, want), (case, alpha)      # kept entries: rho bit-unchanged
        assert rn[0] == 0.0
    # random statistics of random candidate lists
    for alpha in ALPHAS:
        lists = [10.0 ** rng.uniform(-3, 3, size=int(rng.integers(1, 40))) for _ in range(NNS)]
        st = np.concatenate([[np.sum(v) for v in lists], [float(v.size) for v in lists],
                             [v.max() for v in lists], [-v.min() for v in lists]])
        ref, kept, scale = order_stat_reference(alpha, st, NNS)
        assert not kept.any()
        rn, gk, new_rho = _apply_call(lib, ph, alpha, st, rho)
        assert not gk.any()
        worst = max(worst, _ratio(rn, ref, 8 * U * scale))
        assert np.array_equal(new_rho, rn[idx]), (case, alpha)
    assert worst <= 1.0, (case, worst)
    print("[cost_rho_apply %s] S=%d NNS=%d worst error/bound on random inputs = %.3g" % (case, S, NNS, worst))
    return worst


def check_apply_rejects_order_stat(lib, device):
    ph = build_ph(lib, device, k1=2, S=3)
    NNS = ph.NNS
    stats_t = _dev(ph, np.ones(4 * NNS))
    rho_t = _dev(ph, np.ones((2, 3)))
    rn_t, kept_t = _dev(ph, np.zeros(NNS)), _dev(ph, np.zeros(NNS), torch.int32)
    for bad in (-1.0, 1.5, math.nan):
        o = _native.CostRhoOpts()
        o.order_stat = bad
        assert lib.cost_rho_apply(ph._ctx, ctypes.byref(ph._tree), ctypes.byref(o), stats_t.data_ptr(),
                                  ph._xbar_idx_t.data_ptr(), rho_t.data_ptr(), rn_t.data_ptr(),
                                  kept_t.data_ptr(), ph._stream()) != 0
        assert b"order_stat" in lib.last_error(ph._ctx)
    assert np.all(rc._get(rho_t) == 1.0)


# ---------------------------------------------------------------- phx_w_absdiff
W_ABSDIFF_CASES = [(N, S) for N in (1, 3) for S in EXPECT_SIZES]


def check_w_absdiff(lib, device, N, S):
    names = farmer.scenario_names_creator(S)
    creator = farmer.scenario_creator if N == 3 else _one_slot_creator
    ph = PH(ph_options(1), names, creator, scenario_creator_kwargs={"num_scens": S}, _native_lib=lib,
            _device=device)
    assert ph._S == S and ph.batch.nonant.N == N
    rng = np.random.default_rng(9200 + S + N)
    W, Wp = values(rng, (N, S)), values(rng, (N, S))
    ref, bnd = _sum_ref(np.abs(W - Wp))
    outs = []
    for fill in (SENTINEL, -SENTINEL):
        W_t, Wp_t = _dev(ph, W), _dev(ph, Wp)
        out_t = torch.full((2,), fill, dtype=torch.float64, device=ph.device)
        lib.check(ph._ctx, lib.w_absdiff(ph._ctx, W_t.data_ptr(), Wp_t.data_ptr(), out_t.data_ptr(), ph._stream()),
                  "w_absdiff")
        out = rc._get(out_t)
        assert out[1] == fill
        assert np.array_equal(rc._get(Wp_t).reshape(N, S), W), "W_prev is not W afterwards"
        assert np.array_equal(rc._get(W_t).reshape(N, S), W), "W was written"
        # a second pass over the updated snapshot: no difference left
        lib.check(ph._ctx, lib.w_absdiff(ph._ctx, W_t.data_ptr(), Wp_t.data_ptr(), out_t.data_ptr(), ph._stream()),
                  "w_absdiff")
        assert rc._get(out_t)[0] == 0.0
        outs.append(out[0])
    assert outs[0] == outs[1]
    r = _ratio(outs[0], ref, bnd)
    print("[w_absdiff N=%d S=%d] error/bound = %.3g" % (N, S, r))
    assert r <= 1.0, (N, S, r)
    return r


# ---------------------------------------------------------------- the reference's pins, farmer-3
PINS = {
    "grad_denom0": 21.48148148148148,
    "indep": (6.982758620689654, 5.175, 7.977272727272727),
    "corn_xbar_computed": 0.05230103406621424,
    "corn_xbar0": 0.0007911111111111111,
    "wheat_xbar0": 0.0013712592592592591,
    "w_denom": 25.0, "prox_denom": 1250.0,
    "order_stat": 2.6,
}
CORN, BEETS, WHEAT = ("DevotedAcreage[%s0]" % c for c in ("CORN", "SUGAR_BEETS", "WHEAT"))


def _close(a, b, tol=1e-12):
    assert abs(a - b) <= tol * abs(b), (a, b)


def farmer_ph(lib, device, S=3, iters=0, rho=1.0, options=None, extensions=None, mpicomm=None):
    opts = ph_options(iters, rho)
    opts.update(options or {})
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator,
              scenario_creator_kwargs={"num_scens": S}, extensions=extensions, mpicomm=mpicomm,
              _native_lib=lib, _device=device)


def _zero_xbar(ph):
    ph._node_buf.zero_()
    ph._bump()


def _read_rho_csv(path):
    with open(path) as f:
        return {row[0]: float(row[1]) for row in csv.reader(f) if row and not row[0].startswith("#")}


def check_reference_pins(lib, device, tmp_path):
    ph = farmer_ph(lib, device)
    ph.ph_main()                                   # PHIterLimit = 0: x from Iter0, x-bar 0, rho default
    assert not ph._host("xbar").any() and np.all(ph._host("rho") == 1.0)
    what = os.path.join(GOLDEN, "ref_grad_cost.csv")
    cfg = rho_cfg(whatpath=what, rho_file=str(tmp_path / "rho_out.csv"), order_stat=0.4)
    fr = Find_Rho(ph, cfg)
    assert fr.c[("scen0", CORN)] == -150.0 and len(fr.c) == 9
    s0 = ph.local_scenarios["scen0"]
    node = types.SimpleNamespace(name="ROOT")
    _close(fr._w_denom(s0, node)[0], PINS["w_denom"])
    _close(fr._prox_denom(s0, node)[0], PINS["prox_denom"])
    _close(fr._order_stat([4, 3, 1, 5, 2]), PINS["order_stat"])
    rho0 = fr.compute_rho()                        # x-bar = 0
    assert list(rho0) == [CORN, BEETS, WHEAT]
    _close(rho0[CORN], PINS["corn_xbar0"])
    _close(rho0[WHEAT], PINS["wheat_xbar0"])
    assert np.all(ph._host("rho") == 1.0), "the dict API must not install rho"
    ph.Compute_Xbar()
    _close(fr.compute_rho()[CORN], PINS["corn_xbar_computed"])
    _zero_xbar(ph)
    _close(fr._grad_denom()[0], PINS["grad_denom0"])          # (computes x-bar, as the reference's)
    _zero_xbar(ph)
    indep = fr.compute_rho(indep_denom=True)
    ref_rho = _read_rho_csv(os.path.join(GOLDEN, "ref_rho.csv"))
    assert list(ref_rho) == [CORN, BEETS, WHEAT]
    for k, name in enumerate((CORN, BEETS, WHEAT)):
        _close(indep[name], PINS["indep"][k])
        _close(indep[name], ref_rho[name])
    assert fr.kept is not None and not rc._get(fr.kept).any()
    # the order statistic must be set
    try:
        Find_Rho(ph, rho_cfg(whatpath=what, rho_file="x")).compute_rho()
        raise RuntimeError("order_stat = -1 accepted")
    except AssertionError as e:
        assert "you need to set the order statistic parameter for rho using --order-stat" in str(e)
    try:
        Find_Rho(ph, rho_cfg(whatpath=str(tmp_path / "missing.csv"), rho_file="x"))
        raise AssertionError("a missing What file accepted")
    except RuntimeError as e:
        assert "Could not find file" in str(e)
    # Set_Rho on the reference's rho file
    m = farmer.scenario_creator("scen0", num_scens=3)
    pairs = Set_Rho(rho_cfg(rho_path=os.path.join(GOLDEN, "ref_rho.csv"))).rho_setter(m)
    assert len(pairs) == ph.local_scenarios["scen0"]._mpisppy_data.nlens["ROOT"] == 3
    assert isinstance(pairs[0][0], int) and pairs[0] == (id(m.DevotedAcreage["CORN0"]), 6.982758620689654)
    # the gradient cost: the model's own coefficients
    fg = Find_Grad(ph, rho_cfg(grad_cost_file=str(tmp_path / "grad_cost.csv"),
                               grad_rho_file=str(tmp_path / "grad_rho.csv"), order_stat=0.4))
    g = fg.compute_grad("scen0", s0)
    assert [g[("ROOT", i)] for i in range(3)] == [-230.0, -260.0, -150.0]
    assert np.array_equal(rc._get(fg.grad_cost_device()).reshape(3, 3), np.array([[-230.0] * 3, [-260.0] * 3,
                                                                                 [-150.0] * 3]))
    # the writers, parsed back by the reader side
    ph.Compute_Xbar()
    fg.write_grad_cost()
    back = Find_Rho(ph, rho_cfg(whatpath=fg.cfg.grad_cost_file, rho_file="x", order_stat=0.4))
    assert back.c == fg.c and len(back.c) == 9 and back.c[("scen1", BEETS)] == -260.0
    want = back.compute_rho()
    fg.write_grad_rho()
    assert _read_rho_csv(fg.cfg.grad_rho_file) == want
    pairs = Set_Rho(rho_cfg(rho_path=fg.cfg.grad_rho_file)).rho_setter(m)
    assert [p[1] for p in pairs] == [want[n] for n in (CORN, BEETS, WHEAT)]
    fr.write_rho()
    assert _read_rho_csv(cfg.rho_file) == fr.compute_rho()
    return ph


# ---------------------------------------------------------------- end to end against the oracle
class RecordingGradient(Gradient_extension):
    """Gradient_extension that keeps (iteration, per-entry rho, kept) of every firing"""

    def __init__(self, ph):
        super().__init__(ph)
        self.fired = []

    def _update_rho(self):
        out = super()._update_rho()
        self.fired.append((self.opt._PHIter, rc._get(out), rc._get(self.rho_object.kept)[:self.opt.NNS]))
        return out


class SyntheticCostGradient(RecordingGradient):
    """RecordingGradient with a cost of the test's own, 1 + (7 j + 3 s) % 5 for slot
    j and global scenario s.  hydro's nonants (generation, volumes) carry no
    objective coefficient -- its cost sits on the StageCost variables -- so its
    gradient cost, and with it every rho of the rule, is 0, in the reference too;
    the multi-rank hydro run needs candidates that differ between scenarios."""

    def __init__(self, ph):
        super().__init__(ph)
        j = np.arange(ph.batch.nonant.N)[:, None]
        s = ph._local_lo + np.arange(ph._S)[None, :]
        cost = 1.0 + ((7 * j + 3 * s) % 5)
        self.grad_object.grad_cost_device = lambda: torch.as_tensor(cost.astype(np.float64)).to(ph.device)


class OracleGradientPH(oph.OraclePH):
    """OraclePH with Gradient_extension restated in numpy between update_w and
    solve_loop: the W difference, the trigger, and the rule with the
    scenario-dependent denominator per (node name, slot)."""

    def __init__(self, scens, order_stat, **kw):
        super().__init__(scens, **kw)
        self.alpha = order_stat
        self.cost = -np.array([s.c[self.ncol[k]] for k, s in enumerate(scens)])       # (S, N)
        self.keys = sorted({(self.node_of[k][j], j) for k in range(self.S) for j in range(self.N)})
        self.members = {key: [k for k in range(self.S) if self.node_of[k][key[1]] == key[0]] for key in self.keys}
        self.W_prev = None
        self.dual = []
        self.fired, self.declined, self.ratios, self.kept = [], [], [], 0

    def w_diff(self):
        if self.W_prev is None:
            self.W_prev = self.W.copy()
            return 0.0
        d = 0.0
        for sl in oph.rank_slices(self.S, self.n_proc):
            d += float(np.mean(np.abs(self.W[sl] - self.W_prev[sl])))
        self.W_prev = self.W.copy()
        return d / self.n_proc

    def order_stat(self, v):
        a, mean, lo, hi = self.alpha, np.mean(v), np.min(v), np.max(v)
        if a == 0.5:
            return mean
        return lo + a * 2 * (mean - lo) if a < 0.5 else (2 * mean - hi) + a * 2 * (hi - mean)

    def rho_update(self, it):
        diff = self.xn() - self.xbar
        d = np.max(np.maximum(np.abs(diff), 2 * np.square(diff)), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d[:, None] == 0.0, INF, np.abs(self.cost) / d[:, None])
        new = {}
        for key in self.keys:
            mem = self.members[key]
            v = self.order_stat(r[mem, key[1]])
            if np.isfinite(v):
                self.rho[mem, key[1]] = v
            else:
                self.kept += 1
            new[key] = v
        self.fired.append((it, new))

    def miditer(self, it):
        self.dual.append(self.w_diff())
        last, curr = self.dual[-2], self.dual[-1]
        if last == 0:
            return
        ratio = abs((last - curr) / last)
        self.ratios.append(ratio)
        if ratio <= 0.05:
            self.rho_update(it)
        else:
            self.declined.append(it)

    def iter0(self):
        tb = super().iter0()
        self.dual.append(self.w_diff())
        return tb

    def iterk(self, max_iterations, convthresh):
        self.conv = None
        for it in range(1, max_iterations + 1):
            self.iter = it
            self.compute_xbar()
            self.update_w()
            self.conv = self.convergence_diff()
            self.history.append(self.conv)
            self.miditer(it)
            if self.conv < convthresh:
                return it
            self.solve_loop()
        return max_iterations


E2E_CASES = {"farmer-3": (3, 20, 1.0), "farmer-6": (6, 20, 1.0)}     # S, iterations, default rho
ORDER_STAT = 0.4
_ORACLE_RUNS = {}


def oracle_gradient_run(case, n_proc=1):
    """The oracle's run (computed once), with the conditions the comparison needs"""
    if (case, n_proc) not in _ORACLE_RUNS:
        S, iters, rho = E2E_CASES[case]
        o = OracleGradientPH([om.farmer("scen%d" % i, num_scens=S) for i in range(S)], ORDER_STAT, rho=rho,
                             n_proc=n_proc)
        o.iter0()
        o.last_iter = o.iterk(iters, 1e-10)
        print("[oracle %s] fired at %s, declined at %s, closest ratio to 0.05: %.3g, kept %d, conv %.3g"
              % (case, [f[0] for f in o.fired], o.declined, min(abs(r - 0.05) for r in o.ratios), o.kept, o.conv))
        assert len(o.fired) >= 2 and len(o.declined) >= 2
        assert min(abs(r - 0.05) for r in o.ratios) > 1e-6
        assert o.kept == 0 and o.last_iter == iters
        _ORACLE_RUNS[(case, n_proc)] = o
    return _ORACLE_RUNS[(case, n_proc)]


HOST_LOOP = {"iter0_solver_options": {"native_loop": 0}, "iterk_solver_options": {"native_loop": 0}}


def gradient_options(order_stat=ORDER_STAT):
    return dict(HOST_LOOP, gradient_extension_options={"cfg": rho_cfg(order_stat=order_stat)})


def check_end_to_end(lib, device, case):
    S, iters, rho = E2E_CASES[case]
    o = oracle_gradient_run(case)
    ph = farmer_ph(lib, device, S=S, iters=iters, rho=rho, options=gradient_options(), extensions=RecordingGradient)
    conv, Eobj, tb = ph.ph_main()
    assert not hasattr(ph, "iterk_stats"), "a per-iteration hook: the host loop"
    assert all(s["not_optimal"] == 0 for s in ph.solve_stats)
    ext = ph.extobject
    assert [f[0] for f in ext.fired] == [f[0] for f in o.fired], ([f[0] for f in ext.fired], o.fired)
    nn = ph.batch.nonant
    for (it, got, kept), (_, want) in zip(ext.fired, o.fired):
        assert not kept.any()
        for j in range(nn.N):
            _close(got[ph._xbar_idx[j, 0]], want[("ROOT", j)], 1e-9)
    assert ph._PHIter == o.last_iter
    assert rel(conv, o.conv) < 1e-6
    xb, W = ph._host("xbar"), ph.W_array()
    for k in range(ph._S):
        assert rel(xb[ph._xbar_idx[:, k]], o.xbar[k]) < 1e-6
        assert rel(W[k], o.W[k]) < 1e-6
        assert rel(ph._host("rho")[:, k], o.rho[k]) < 1e-9
    assert rel(ext.dual_conv_cache, o.dual) < 1e-6 and len(ext.primal_conv_cache) == iters + 1
    return ph


def check_bundles_refused(lib, device):
    opts = gradient_options()
    opts["bundles_per_rank"] = 1
    try:
        farmer_ph(lib, device, S=6, iters=2, options=opts, extensions=Gradient_extension)
    except NotImplementedError as e:
        assert "bundles_per_rank" in str(e)
    else:
        raise AssertionError("bundles_per_rank accepted")


# ---------------------------------------------------------------- multistage
BFS = [3, 3]


def hydro_ph(lib, device, iters=0, options=None, extensions=None, mpicomm=None):
    opts = ph_options(iters, 1.0)
    opts.update(options or {})
    return PH(opts, hydro.scenario_names_creator(9), hydro.scenario_creator,
              scenario_creator_kwargs={"branching_factors": BFS},
              all_nodenames=sputils.create_nodenames_from_branching_factors(BFS), extensions=extensions,
              mpicomm=mpicomm, _native_lib=lib, _device=device)


def check_multistage(lib, device):
    """hydro (9 scenarios, 3 stages): compute_rho_device in both modes against
    per-node numpy on the host copies; the dict API keeps the two-stage assertion."""
    ph = hydro_ph(lib, device)
    ph.ph_main()
    ph.Compute_Xbar()
    nn = ph.batch.nonant
    N, S, NNS, idx = nn.N, ph._S, ph.NNS, ph._xbar_idx
    assert NNS > N and ph.multistage
    rng = np.random.default_rng(31)
    cost = values(rng, (N, S))
    cost_t = torch.as_tensor(cost).to(ph.device)
    X = ph._host("x")[nn.slot_col].copy()
    xbar = ph._host("xbar").copy()
    rho_before = ph._host("rho").copy()
    for alpha in (0.4, 0.5, 0.6):
        fr = Find_Rho(ph, rho_cfg(order_stat=alpha))
        for indep in (False, True):
            dn = None
            if indep:
                dn = np.zeros(NNS)
                np.add.at(dn, idx, ph._prob_coeff * np.abs(X - xbar[idx]))
                dn = np.maximum(dn, 1e-3)
            r, _ = candidates(idx, cost, X, xbar, dn)
            st, _, present = stats_reference(idx, NNS, r)
            assert present.all()
            ref, kept, _ = order_stat_reference(alpha, st, NNS)
            got = rc._get(fr.compute_rho_device(cost_t, indep_denom=indep, install=False))
            assert not kept.any() and not rc._get(fr.kept).any()
            assert rel(got, ref) < 1e-12 and np.max(np.abs(got - ref) / np.abs(ref)) < 1e-12, (alpha, indep)
            assert np.array_equal(ph._host("rho"), rho_before)
    inst = rc._get(fr.compute_rho_device(cost_t))      # installed: every scenario of a node gets its entry's rho
    assert np.array_equal(ph._host("rho"), inst[idx]) and not np.array_equal(inst[idx], rho_before)
    try:
        Find_Rho(ph, rho_cfg(order_stat=0.4)).compute_rho()
    except AssertionError as e:
        assert "compute rho only works for two stage for now" in str(e)
    else:
        raise RuntimeError("the dict API accepted a multistage tree")
    return ph
