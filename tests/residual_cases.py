"""Direct checks of the adaptive-rho entry points (phx_node_absdev,
phx_norm_rho, phx_rho_sums) on chosen inputs, at the sizes where their host
entry points change kernels.  The PH objects, values and bounds are those of
reduction_cases.py (imported, not copied); ``test_residuals.py`` runs each
check on the host emulation and on the HIP kernels.

Reference of the two reductions: ``math.fsum`` over the float64 terms formed
in numpy -- ``w*|x - xbar|`` with the difference rounded once, ``p*(sum_j
rho)`` with the inner sum in slot order (as the entry point states it) and
``rho*|xbar - prev|`` -- with reduction_cases' any-order bound
``(n + 2) u sum|term|`` per entry (derived there; u = 2**-53).  The total slot
of phx_node_absdev must equal the entries added in index order, exactly.
Every call is made twice into sentinel-filled buffers and must repeat bit for
bit.

phx_norm_rho is compared exactly (``np.array_equal``) with a numpy restatement
of the rule on inputs built from exactly representable numbers that hit every
branch with margin and on its boundaries.

The bounds were fixed against the host emulation only (worst error / bound
there: absdev 0.19 per entry, 0.17 for the slices, on their own and added up;
rho sums 0.015 and 0.0077).  First measurement on the MI355X: absdev 0.28
(k_absdev_small, T3u) and 0.047 (k_absdev), slices 0.021; rho sums 0.0016
and 0.0029.
"""
import ctypes

import numpy as np
import torch

from mpisppy_amd import _native
from mpisppy_amd import model as lm
from mpisppy_amd.batch import BatchData, NonantSpec
from mpisppy_amd.examples import farmer
from mpisppy_amd.opt.ph import PH
from helpers import ph_options
import reduction_cases as rc
from reduction_cases import build_ph, values, _ratio, _sum_ref, T3U, XBAR_CASES, SLICE_CASES, EXPECT_SIZES

U = rc.U
SENTINEL = rc.SENTINEL


def _dev(ph, a, dtype=torch.float64):
    """a device copy (on the cpu too: the calls write into some of these)"""
    return torch.tensor(np.ascontiguousarray(a).ravel(), dtype=dtype).to(ph.device)


# ---------------------------------------------------------------- phx_node_absdev
ABSDEV_CASES = {}
for _S in (1, 63, 64, 65, 1023, 1024, 1025, 1300):
    for _N in (1, 8):
        ABSDEV_CASES["S%d-N%d" % (_S, _N)] = dict(k1=_N, S=_S)
ABSDEV_CASES["T3u"] = dict(T3U)
for _c in ("300-nodes", "S1300-N5-tile16", "S1300-N70", "20-nodes-S1100"):
    ABSDEV_CASES[_c] = dict(XBAR_CASES[_c])


def absdev_reference(xbar_idx, NNS, X, xbar, wt):
    """sum w |x - xbar| per (node, slot) entry over the given scenarios:
    (ref, bound, present) arrays of length NNS.  wt: (S,) or (N, S)."""
    ref = np.zeros(NNS)
    bnd = np.zeros(NNS)
    present = np.zeros(NNS, dtype=bool)
    w = np.broadcast_to(wt, X.shape)
    terms = w * np.abs(X - xbar[xbar_idx])          # the difference rounded once, in float64
    for j in range(xbar_idx.shape[0]):
        idx = xbar_idx[j]
        for e in np.unique(idx):
            ref[e], bnd[e] = _sum_ref(terms[j, idx == e])
            present[e] = True
    return ref, bnd, present


def _absdev_call(lib, ph, xbar_t, wt_t, per_slot, prefill):
    """phx_node_absdev into buffers of the test's own, prefilled"""
    NNS = ph.NNS
    out_t = _dev(ph, prefill)
    part_t = torch.full((max(int(ph._tree.npart), 1),), SENTINEL, dtype=torch.float64, device=ph.device)
    assert part_t.data_ptr() != ph._partial.data_ptr()
    lib.check(ph._ctx, lib.node_absdev(ph._ctx, ctypes.byref(ph._tree), ph._x.data_ptr(), xbar_t.data_ptr(),
                                       wt_t.data_ptr(), int(per_slot), part_t.data_ptr(), out_t.data_ptr(),
                                       ph._stream()), "node_absdev")
    got = rc._get(out_t)
    assert got[NNS + 1] == prefill[NNS + 1], "wrote past out[NNS]"
    return got[:NNS + 1]


def _index_order_sum(v):
    t = 0.0
    for a in v:
        t += float(a)
    return t


def check_absdev(lib, device, case):
    ph = build_ph(lib, device, **dict(ABSDEV_CASES[case]))
    N, S, NNS = ph.batch.nonant.N, ph._S, ph.NNS
    rng = np.random.default_rng(3000 + S + 7 * N)
    X, xbar = values(rng, (N, S)), values(rng, NNS)
    p = rng.uniform(0.05, 1.0, size=S) / S
    PC = rng.uniform(0.05, 1.0, size=(N, S)) / S
    rc._fill_x_pc(ph, X, PC)
    xbar_t = _dev(ph, xbar)
    worst = 0.0
    for per_slot, wt in ((0, p), (1, PC)):
        wt_t = _dev(ph, wt)
        ref, bnd, present = absdev_reference(ph._xbar_idx, NNS, X, xbar, wt)
        assert present.all()
        got = _absdev_call(lib, ph, xbar_t, wt_t, per_slot, np.full(NNS + 2, SENTINEL))
        r = _ratio(got[:NNS], ref, bnd)
        assert got[NNS] == _index_order_sum(got[:NNS]), (case, per_slot, got[NNS])
        again = _absdev_call(lib, ph, xbar_t, wt_t, per_slot, np.full(NNS + 2, -SENTINEL))
        assert np.array_equal(got, again), (case, per_slot)
        assert r <= 1.0, (case, per_slot, r)
        worst = max(worst, r)
    print("[absdev %s] S=%d N=%d NNS=%d tiles=%d worst error/bound = %.3g" % (case, S, N, NNS, len(ph._tiles), worst))
    return worst


def check_absdev_slices(lib, device, case):
    """Each slice as one rank of several sees it: entries of absent nodes read
    exactly zero, also on a second call into a buffer that holds all-reduced
    values, and the slices add up to the whole."""
    cfg, slices = SLICE_CASES[case]
    S = int(sum(cfg["counts"]))
    N = cfg["k1"] + cfg["k2"]
    rng = np.random.default_rng(177 + S)
    X = values(rng, (N, S))
    p = rng.uniform(0.05, 1.0, size=S) / S
    whole = build_ph(lib, device, **cfg)
    NNS = whole.NNS
    xbar = values(rng, NNS)
    gref, gbnd, gpresent = absdev_reference(whole._xbar_idx, NNS, X, xbar, p)
    assert gpresent.all()
    runs, gots, worst = [], [], 0.0
    for lo, hi in slices:
        ph = build_ph(lib, device, lo=lo, hi=hi, **cfg)
        assert ph.NNS == NNS and ph._tree.nnodes_cover < NNS
        rc._fill_x_pc(ph, X[:, lo:hi], np.ones((N, hi - lo)))
        xbar_t, wt_t = _dev(ph, xbar), _dev(ph, p[lo:hi])
        ref, bnd, present = absdev_reference(ph._xbar_idx, NNS, X[:, lo:hi], xbar, p[lo:hi])
        assert not present.all()
        got = _absdev_call(lib, ph, xbar_t, wt_t, 0, np.full(NNS + 2, SENTINEL))
        assert np.all(got[:NNS][~present] == 0.0), (
            "slice [%d,%d): entries of absent nodes are not zero: %s" % (lo, hi, got[:NNS][~present][:8]))
        assert got[NNS] == _index_order_sum(got[:NNS])
        worst = max(worst, _ratio(got[:NNS][present], ref[present], bnd[present]))
        runs.append((ph, xbar_t, wt_t))
        gots.append(got)
    total = np.sum(gots, axis=0)
    rt = _ratio(total[:NNS], gref, gbnd)
    print("[absdev slices %s] worst error/bound: slices %.3g, summed over slices %.3g" % (case, worst, rt))
    assert worst <= 1.0 and rt <= 1.0, (case, worst, rt)
    # the second call of a host loop: the buffer holds the all-reduced values
    for (ph, xbar_t, wt_t), got in zip(runs, gots):
        again = _absdev_call(lib, ph, xbar_t, wt_t, 0, np.concatenate([total, [SENTINEL]]))
        assert np.array_equal(again, got), "stale residuals were kept or re-added"
    return worst, rt


# ---------------------------------------------------------------- phx_norm_rho
# tol 0.5, factor 4: (primal, dual, expected action with decreases allowed)
TOL, FACTOR, INC, DEC, CDEC = 0.5, 4.0, 1.5, 3.0, 1.1
PATTERNS = [
    (8.0, 1.0, 1),         # primal > factor dual, with margin
    (4.0, 1.0, 0),         # primal == factor dual
    (1.0, 8.0, 2),         # dual > factor primal, with margin
    (1.0, 4.0, 0),         # dual == factor primal
    (0.5, 0.0625, 0),      # primal == tol (above factor dual, not above tol; not below tol either)
    (0.0625, 0.5, 0),      # dual == tol
    (0.0, 0.0, 3),         # both residuals zero
    (0.25, 0.125, 3),      # both below tol, neither ratio
    (2.0, 0.25, 1),
    (0.75, 0.75, 0),       # above tol, neither ratio
    (0.25, 4.0, 2),
]
NORM_RHO_CASES = {"S%d" % _S: dict(k1=len(PATTERNS), S=_S) for _S in (1, 65, 1024, 1025)}
NORM_RHO_CASES["T3u"] = dict(T3U)
NORM_RHO_CASES["T3u-slice"] = dict(T3U, lo=0, hi=200)      # no local scenario for the last node


def norm_rho_rule(primal, dual, allow):
    """norm_rho_updater.py:133-143 on arrays: 1 increase, 2 decrease, 3 converged decrease"""
    act = np.zeros(primal.shape, dtype=np.int32)
    for e in range(primal.size):
        p, d = primal[e], dual[e]
        if (p > FACTOR * d) and (p > TOL):
            act[e] = 1
        elif (d > FACTOR * p) and (d > TOL):
            if allow:
                act[e] = 2
        elif (p < TOL) and (d < TOL):
            act[e] = 3
    return act


def check_norm_rho(lib, device, case):
    ph = build_ph(lib, device, **dict(NORM_RHO_CASES[case]))
    N, S, NNS = ph.batch.nonant.N, ph._S, ph.NNS
    idx = ph._xbar_idx
    rng = np.random.default_rng(4000 + S)
    present = np.zeros(NNS, dtype=bool)
    present[np.unique(idx)] = True
    assert present.all() == (case != "T3u-slice")
    pat = [PATTERNS[e % len(PATTERNS)] for e in range(NNS)]
    primal = np.array([q[0] for q in pat] + [SENTINEL])
    rho = rng.uniform(0.1, 10.0, size=(N, S))                 # non-uniform over the scenarios
    xbar = np.array([0.25 * (e % 7) - 0.5 for e in range(NNS)])
    prev = xbar.copy()
    rep = np.ones(NNS)
    last = {}
    for j in range(N):
        for e in np.unique(idx[j]):
            s_last = int(np.nonzero(idx[j] == e)[0][-1])      # the node's last local scenario
            last[e] = (j, s_last)
            rep[e] = 2.0 ** (e % 3 - 1)
            rho[j, s_last] = rep[e]
    for e in range(NNS):
        prev[e] = xbar[e] + (1 if e % 2 else -1) * pat[e][1] / rep[e]     # dyadic: |xbar - prev| is exact
    seen = set()
    for allow in (0, 1):
        dual = np.array([rho[last[e]] * abs(xbar[e] - prev[e]) if present[e] else 0.0 for e in range(NNS)])
        assert all(dual[e] == pat[e][1] for e in range(NNS) if present[e])
        act = np.where(present, norm_rho_rule(primal[:NNS], dual, allow), 0).astype(np.int32)
        if allow:
            assert all(act[e] == pat[e][2] for e in range(NNS) if present[e])
        a = act[idx]
        new_rho = np.where(a == 1, rho * INC, np.where(a == 2, rho / DEC, np.where(a == 3, rho / CDEC, rho)))
        new_prev = np.where(present, xbar, prev)
        seen |= set(int(v) for v in act)
        o = _native.NormRhoOpts()
        o.tol, o.rho_increase, o.rho_decrease, o.pd_factor, o.conv_decrease = TOL, INC, DEC, FACTOR, CDEC
        o.allow_decrease = allow
        for with_dual in (True, False):
            primal_t, xbar_t, prev_t, rho_t = _dev(ph, primal), _dev(ph, xbar), _dev(ph, prev), _dev(ph, rho)
            dual_t = torch.full((NNS + 1,), SENTINEL, dtype=torch.float64, device=ph.device)
            act_t = torch.full((NNS + 1,), 9, dtype=torch.int32, device=ph.device)
            lib.check(ph._ctx, lib.norm_rho(ph._ctx, ctypes.byref(ph._tree), ctypes.byref(o), primal_t.data_ptr(),
                                            xbar_t.data_ptr(), prev_t.data_ptr(), ph._xbar_idx_t.data_ptr(),
                                            rho_t.data_ptr(), dual_t.data_ptr() if with_dual else None,
                                            act_t.data_ptr(), ph._stream()), "norm_rho")
            got_act, got_dual = rc._get(act_t), rc._get(dual_t)
            assert np.array_equal(got_act[:NNS], act) and got_act[NNS] == 9, (case, allow, got_act, act)
            assert np.array_equal(got_dual[:NNS], dual if with_dual else np.full(NNS, SENTINEL)), (case, allow)
            assert got_dual[NNS] == SENTINEL
            assert np.array_equal(rc._get(rho_t).reshape(N, S), new_rho), (case, allow)
            assert np.array_equal(rc._get(prev_t), new_prev), (case, allow)
            assert np.array_equal(rc._get(primal_t), primal) and np.array_equal(rc._get(xbar_t), xbar)
    assert seen == {0, 1, 2, 3}


# ---------------------------------------------------------------- phx_rho_sums
RHO_SUMS_CASES = [(N, S) for N in (1, 3) for S in EXPECT_SIZES]


def _one_slot_batch(scenario_names, num_scens=None):
    """build_ph's model with one nonant (a0 + z <= 2e4, min z), every scenario at once"""
    n = len(scenario_names)
    nonant = NonantSpec([0], [1], [0], [None], [np.ones(n)], ["a0"])
    return BatchData(scenario_names, [0, 2], [0, 1], np.ones((n, 2)), [-np.inf], [2e4], np.array([-1e4, 0.0]),
                     np.array([1e4, 1.0]), np.array([0.0, 1.0]), 0.0, lm.minimize, [1.0 / num_scens] * n,
                     nonant, ["a0", "z"])


def _one_slot_creator(name, num_scens=None):
    return rc._creator(name, k1=1, S=num_scens)


_one_slot_creator.batch_creator = _one_slot_batch


def check_rho_sums(lib, device, N, S):
    names = farmer.scenario_names_creator(S)
    creator = farmer.scenario_creator if N == 3 else _one_slot_creator
    ph = PH(ph_options(1), names, creator, scenario_creator_kwargs={"num_scens": S}, _native_lib=lib,
            _device=device)
    assert ph._S == S and ph.batch.nonant.N == N and ph.NNS == N
    rng = np.random.default_rng(9100 + S + N)
    p = rng.uniform(0.05, 1.0, size=S)
    p /= p.sum()
    rho = rng.uniform(0.1, 10.0, size=(N, S))
    xbar, prev = values(rng, N), values(rng, N)
    idx = ph._xbar_idx
    rsum = np.zeros(S)
    for j in range(N):                                   # slots in order, as the kernels
        rsum = rsum + rho[j]
    ref0, b0 = _sum_ref(p * rsum)
    ref1, b1 = _sum_ref(rho * np.abs(xbar[idx] - prev[idx]))
    p_t, rho_t, xbar_t, prev_t = _dev(ph, p), _dev(ph, rho), _dev(ph, xbar), _dev(ph, prev)
    outs = []
    for fill, with_prev in ((SENTINEL, True), (-SENTINEL, True), (SENTINEL, False)):
        out_t = torch.full((3,), fill, dtype=torch.float64, device=ph.device)
        lib.check(ph._ctx, lib.rho_sums(ph._ctx, rho_t.data_ptr(), p_t.data_ptr(), xbar_t.data_ptr(),
                                        prev_t.data_ptr() if with_prev else None, ph._xbar_idx_t.data_ptr(),
                                        out_t.data_ptr(), ph._stream()), "rho_sums")
        outs.append(rc._get(out_t))
    assert outs[0][2] == SENTINEL and np.array_equal(outs[0][:2], outs[1][:2])
    assert outs[2][1] == 0.0 and outs[2][0] == outs[0][0], "a NULL xbar_prev must give an exact 0"
    r = [_ratio(outs[0][0], ref0, b0), _ratio(outs[0][1], ref1, b1)]
    print("[rho_sums N=%d S=%d] worst error/bound (sum p rho, sum rho |dxbar|) = %s" % (N, S, ["%.3g" % v for v in r]))
    assert max(r) <= 1.0, (N, S, r)
    return r
