"""Shared cases of the infeasible / unbounded subproblem tests (test_infeasible.py on
the ABI emulation, test_infeasible_gpu.py on the kernels).

A false OPTIMAL on an infeasible lane turns an xhat trial into an inner bound that is
no bound; a false INFEASIBLE (status 4: a Farkas proof) throws a valid incumbent away.
The inputs here are the synthetic families of synth_cases.py, which have no complete
recourse:

* candidate ladders: xhat = x0[:N] + t d for two fixed sign directions d and a ladder
  of steps t, so that one batch mixes feasible and infeasible lanes, from no
  infeasible scenario to all of them, through ``XhatBase._try_one``;
* broken families: a deep copy of a family in which three scenarios get a row side
  shifted out of reach and two get the costs of their one-sided columns negated
  (a recession direction that improves), through ``Iter0`` and ``ph_main``.

The verdicts are the oracle's alone (HiGHS on the plain LP, and for the ladders an
elastic LP in scipy that measures how far from feasible a pair is), fixed before the
engine is consulted.

Measured (emulation / MI355X).  Status-4 lanes over oracle-infeasible lanes, recorded and
not gated: vary_all 154 / 145 of 180 (also weighted and with the JIT off), fill 176 / 176
of 185, eq_range_free 140 / 140 of 140, n30_m25 316 / 316 of 330 (with and without the
workgroup pass), n65_m6 292 / 292 of 292; the other infeasible lanes end as status 2.
Worst objective error of a feasible pair over its 1e-9 tolerance: 1.5e-6 / 1.4e-6
(n30_m25).  Smallest elastic relaxation of an infeasible pair: 5.1e-4 (n30_m25).
"""
import copy
import math

import numpy as np
import pytest
from scipy.optimize import linprog

import synth_cases as sc  # noqa: F401  (the families)
import test_synth_structures as ts
import xhat_cases as xc
from helpers import ph_options, rel
from mpisppy_amd.extensions.xhatbase import XhatBase
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.utils.xhat_eval import Xhat_Eval
from oracle import ph as oph, qp

S = 70
MARGINAL = 1e-6            # an elastic relaxation below this: the pair is marginal
NO_JIT = {"PHX_NO_JIT": "1"}

# case: (family key, solver options, environment, ladder steps, the oracle's infeasible
# counts over the 70 scenarios per step for the two directions)
_VARY_T = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0)
_VARY_C = ((0, 0), (0, 0), (0, 9), (0, 31), (0, 61), (9, 70))
_N30_T = (0.0625, 0.125, 0.1875, 0.25, 0.375, 0.5)
_N30_C = ((0, 0), (8, 0), (20, 12), (38, 20), (66, 38), (70, 58))
LADDERS = {
    "vary_all": ("vary_all", None, {}, _VARY_T, _VARY_C),
    "fill": ("fill", None, {}, (0.25, 0.375, 0.5, 0.75), ((0, 18), (0, 35), (0, 62), (0, 70))),
    # equality rows and free columns: all or nothing
    "eq_range_free": ("eq_range_free", None, {}, (1.0, 1.25, 1.5, 2.0), ((0, 0), (0, 0), (70, 0), (70, 0))),
    # a sparse-solver context (the workgroup pass in front of it by default)
    "n30_m25": ("n30_m25", None, {}, _N30_T, _N30_C),
    "n30_m25/no_wg": ("n30_m25", {"wg_warm": 0}, {}, _N30_T, _N30_C),
    # (workgroup pass, the sparse solver behind it; the step 36 is one more than the
    # four first asked for: without it no candidate is infeasible in every scenario)
    "n65_m6": ("n65_m6", None, {}, (16.0, 24.0, 28.0, 32.0, 36.0),
               ((0, 0), (0, 0), (10, 10), (66, 66), (70, 70))),
    # PDHG, polish and the dense interior point
    "vary_all/no_jit": ("vary_all", {"lane_solver": 0}, NO_JIT, _VARY_T, _VARY_C),
}
LANE_CASES = ("vary_all", "fill", "eq_range_free")      # the lane solver serves these on the GPU

# Iter0 with broken scenarios: (family key, solver options)
BROKEN = {
    "vary_all": ("vary_all", None),
    "n30_m25": ("n30_m25", None),
    "n30_m25/no_wg": ("n30_m25", {"wg_warm": 0}),
    "n65_m6": ("n65_m6", None),
    # the shifted rows alone: on the lane structure every broken scenario is then proven
    # infeasible (status 4) and none is merely left without a verdict
    "vary_all/shifted": ("vary_all", None),
}
SHIFTED, NEGATED = (3, 40, 64), (9, 69)

_ORACLE, _BROKEN = {}, {}


def base_family(key):
    return ts.family(ts.BEYOND.get(key, key), 1, S=S)


def scenario_weights(n):
    """p_k proportional to 1 + (5k mod 7) (weight_cases.scenario_weights)."""
    w = 1.0 + (5 * np.arange(n) % 7)
    return w / w.sum()


# ---------------------------------------------------------------- the ladders' oracle
def candidates(fam, steps):
    """[(t, direction, xhat)] in the order of the nonant-cache rows they go to."""
    d = np.random.RandomState(3).choice([-1., 1.], size=(2, fam.N))
    return [(t, k, fam.x0[:fam.N] + t * d[k]) for t in steps for k in range(2)]


def elastic_relaxation(fam, k, xhat):
    """min v such that every finite row side and every finite bound of a column that
    is no nonant holds when relaxed by v (1 + |b|), the nonants fixed at xhat: 0 on a
    feasible pair, the (scaled) distance from feasibility otherwise."""
    n, N = fam.n, fam.N
    A = fam.dense_A(k)
    rows, rhs = [], []

    def add(a, b, upper):
        # upper: a'x - v (1 + |b|) <= b;  lower: -a'x - v (1 + |b|) <= -b
        rows.append(np.concatenate([a if upper else -a, [-(1.0 + abs(b))]]))
        rhs.append(b if upper else -b)
    for i in range(fam.m):
        if np.isfinite(fam.bu[k, i]):
            add(A[i], fam.bu[k, i], True)
        if np.isfinite(fam.bl[k, i]):
            add(A[i], fam.bl[k, i], False)
    for j in range(N, n):
        e = np.zeros(n)
        e[j] = 1.0
        if np.isfinite(fam.ub[k, j]):
            add(e, fam.ub[k, j], True)
        if np.isfinite(fam.lb[k, j]):
            add(e, fam.lb[k, j], False)
    bounds = [(float(v), float(v)) for v in xhat] + [(None, None)] * (n - N) + [(0.0, None)]
    cost = np.zeros(n + 1)
    cost[n] = 1.0
    r = linprog(cost, A_ub=np.array(rows), b_ub=np.array(rhs), bounds=bounds, method="highs")
    assert r.status == 0, (fam.family, k, r.status, r.message)
    return float(r.fun)


def ladder_oracle(fam, steps):
    """Per candidate: the oracle's fixed-xhat evaluation (oracle.ph.evaluate_xhat:
    HiGHS, then the certified polish), HiGHS's own word on every pair it did not
    solve, and the elastic relaxation of every pair.  A pair is *infeasible* when HiGHS
    says infeasible and v >= 1e-6, *feasible* when HiGHS solves it, marginal otherwise;
    the ladders must have no marginal pair, and the elastic count must be HiGHS's.
    Computed once per family and ladder; nothing here has seen the engine."""
    key = (id(fam), tuple(steps))
    if key in _ORACLE:
        return _ORACLE[key]
    scens = fam.scens()
    out = []
    for t, k, xhat in candidates(fam, steps):
        E, objs, solved = oph.evaluate_xhat(scens, {"ROOT": xhat})
        said_infeasible = np.zeros(fam.S, dtype=bool)
        for s in np.nonzero(~solved)[0]:
            sn = scens[s]
            lb, ub = sn.lb.copy(), sn.ub.copy()
            lb[:fam.N] = ub[:fam.N] = xhat
            said_infeasible[s] = qp.highs_solve(sn.A, sn.bl, sn.bu, lb, ub, sn.c)[1] == "Infeasible"
        v = np.array([elastic_relaxation(fam, s, xhat) for s in range(fam.S)])
        infeasible = said_infeasible & (v >= MARGINAL)
        marginal = ~solved & ~infeasible
        out.append(dict(t=t, direction=k, xhat=xhat, E=E, objs=objs, feasible=solved, infeasible=infeasible,
                        marginal=marginal, v=v))
    _ORACLE[key] = out
    return out


def check_ladder_oracle(fam, steps, counts, all_or_nothing=False):
    """What the ladder must be, from the oracle alone (a family whose draw changed
    fails here, not on the engine): no marginal pair, the elastic LP and HiGHS count
    the same pairs, the counts of the table, a candidate feasible in every scenario
    and one infeasible in every scenario, and two candidates or more with between 5 %
    and 95 % of the scenarios infeasible."""
    orc = ladder_oracle(fam, steps)
    got = [int(c["infeasible"].sum()) for c in orc]
    vmin = min([float(c["v"][c["infeasible"]].min()) for c in orc if c["infeasible"].any()])
    print(fam.family, "infeasible per candidate", got, "smallest relaxation of an infeasible pair %.2e" % vmin)
    assert sum(int(c["marginal"].sum()) for c in orc) == 0
    for c in orc:
        assert np.array_equal(c["v"] >= MARGINAL, c["infeasible"])
        assert np.array_equal(c["feasible"], ~c["infeasible"])
        assert np.isfinite(c["objs"][c["feasible"]]).all()
    assert got == [v for pair in counts for v in pair], got
    assert 0 in got and fam.S in got
    mixed = [g for g in got if 0.05 * fam.S <= g <= 0.95 * fam.S]
    assert all_or_nothing or len(mixed) >= 2, got
    return orc, vmin


# ---------------------------------------------------------------- the ladders' trials
def make_eval(lib, device, fam, so):
    return Xhat_Eval(xc.xhat_options(so), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs,
                     _native_lib=lib, _device=device)


def check_ladder(lib, device, case, monkeypatch, weights=False, lane=False):
    """One row of the table: every candidate through ``_try_one`` (restore_nonants True)
    against the oracle's verdicts.  Returns (status-4 lanes on infeasible pairs,
    infeasible pairs, the largest objective error of a feasible pair over its 1e-9
    tolerance); the detection rate is recorded, not asserted."""
    key, so, env, steps, counts = LADDERS[case]
    fam = base_family(key)
    orc, _ = check_ladder_oracle(fam, steps, counts, all_or_nothing=key == "eq_range_free")
    if weights:
        fam = fam.weighted(prob=scenario_weights(fam.S))
    p = np.array([fam.scen_prob(k) for k in range(fam.S)])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ev = make_eval(lib, device, fam, so)
    ev.solve_loop(solver_options=so)
    before = ev.nonant_values().copy()
    o = ts.oracle_iter0(base_family(key))
    assert rel(ev._host("obj"), o.obj) < 1e-8
    xc.prepare(ev, o)
    cache = o.xn().copy()
    for c, cand in enumerate(orc):
        cache[c] = cand["xhat"]
    ev._put_nonant_cache(cache.ravel())
    ev._restore_nonants()
    cached = ev.nonant_cache.copy()
    assert all(np.array_equal(cached[c], cand["xhat"]) for c, cand in enumerate(orc))
    xb = XhatBase(ev)
    xb.post_iter0()
    views = list(ev.local_scenarios[fam.names[0]]._mpisppy_data.nonant_indices.values())
    info = ev._native.jit_info(ev._ctx).decode()
    # the per-lane arrays as they stand when the trial's restore begins
    at_restore = []
    restore = ev._restore_nonants_device

    def spy():
        at_restore.append((ev._status.cpu().numpy().copy(), ev._host("obj").copy()))
        return restore()
    ev._restore_nonants_device = spy
    found = total = 0
    worst = 0.0
    for c, cand in enumerate(orc):
        infeasible, feasible = cand["infeasible"], cand["feasible"]
        del at_restore[:]
        E = xb._try_one({"ROOT": fam.names[c]}, solver_options=so, restore_nonants=True)
        status = ev._status.cpu().numpy().copy()
        obj = ev._host("obj").copy()
        st = ev.solve_stats[-1]
        infeas_p = ev.infeas_prob()
        n4 = int((status == 4).sum())
        print("%s t=%g d=%d: oracle infeasible %d; status 1/2/3/4 = %s; lane_certified %d stragglers %d "
              "wg_certified %d sp_certified %d; not_optimal %d infeasible %d"
              % (case, cand["t"], cand["direction"], infeasible.sum(),
                 [int((status == q).sum()) for q in (1, 2, 3, 4)], st["lane_certified"], st["stragglers"],
                 st["wg_certified"], st["sp_certified"], st["not_optimal"], st["infeasible"]))
        # the restore of the trial left the trial's per-lane results alone
        assert len(at_restore) == 1
        assert np.array_equal(at_restore[0][0], status) and np.array_equal(at_restore[0][1], obj, equal_nan=True)
        assert not (status[infeasible] == 1).any(), np.nonzero(infeasible & (status == 1))[0]            # 1
        assert not (status[feasible] == 4).any(), np.nonzero(feasible & (status == 4))[0]                # 2
        assert (status[feasible] == 1).all(), (np.nonzero(feasible & (status != 1))[0], status[feasible])  # 3
        if feasible.any():
            err = rel(obj[feasible], cand["objs"][feasible])
            worst = max(worst, err / 1e-9)
            assert err < 1e-9, err
        if infeasible.any():                                                                             # 4
            assert E is None
        else:
            Eo = math.fsum(p * cand["objs"])
            assert E is not None and rel(E, Eo) < 1e-9, (E, Eo)
        assert np.array_equal(ev.nonant_values(), cached)                                                # 5
        assert not ev._fixed.any() and not any(v.fixed for v in views)
        assert st["infeasible"] == n4                                                                    # 6
        # 7: not_optimal counts the lanes that ended without a verdict (status 2 or 3);
        # the status-4 lanes are counted by "infeasible" alone
        assert st["not_optimal"] == int(((status != 1) & (status != 4)).sum())
        assert st["not_optimal"] + st["infeasible"] == int((status != 1).sum())
        assert abs(infeas_p - math.fsum(p[status != 1])) <= 1e-12                                        # 8
        if weights:
            # every infeasible lane is not optimal and every feasible one is, so this is
            # the oracle's infeasible set's probability
            assert abs(infeas_p - math.fsum(p[infeasible])) <= 1e-12
        if lane:
            assert st["lane_certified"] <= int(feasible.sum())
        found += int((status[infeasible] == 4).sum())
        total += int(infeasible.sum())
    ev._restore_nonants_device = restore
    assert np.array_equal(ev.nonant_cache, cached)
    if lane:
        assert "fixed-nonant lane module on" in ev._native.jit_info(ev._ctx).decode(), info
    xc.check_restored_solve(ev, before, solver_options=so)                                               # 9
    for k in env:
        monkeypatch.delenv(k)
    print("%s%s: detected (status 4) %d of %d infeasible pairs = %.3f; worst objective error / 1e-9 = %.2e"
          % (case, " weighted" if weights else "", found, total, found / total, worst))
    assert found > 0, "no lane was proven infeasible: the Farkas test never accepted"
    return found, total, worst


# ---------------------------------------------------------------- Iter0 with broken scenarios
def broken_family(case):
    """A deep copy of the family (ts.family caches: its arrays stay as they are) with
    the lower side of the first ge / range row raised by 64 in scenarios 3, 40 and 64
    (a range row's upper side with it), and the cost of every lower-only and upper-only
    column negated in scenarios 9 and 69.  Returns (family, HiGHS's status per scenario:
    0 solved, 2 infeasible, 3 unbounded, the expected objectives of the solved ones)."""
    if case in _BROKEN:
        return _BROKEN[case]
    key = BROKEN[case][0]
    negated = () if case.endswith("/shifted") else NEGATED
    base = base_family(key)
    fam = copy.deepcopy(base)
    i = [kd in ("ge", "range") for kd in fam.rkind].index(True)
    for k in SHIFTED:
        fam.bl[k, i] += 64.0
        if fam.rkind[i] == "range":
            fam.bu[k, i] += 64.0
    one_sided = [j for j, kd in enumerate(fam.ckind) if kd in ("lo", "up")]
    for k in negated:
        fam.c[k, one_sided] = -fam.c[k, one_sided]
    fam.creator = fam._make_creator()
    verdict = np.zeros(fam.S, dtype=int)
    want = ts.oracle_iter0(base).obj.copy()
    for k in SHIFTED + negated:
        sn = fam.scen(k)
        eq = sn.bl == sn.bu
        lo, hi = np.isfinite(sn.bl) & ~eq, np.isfinite(sn.bu) & ~eq
        r = linprog(sn.c, A_ub=np.vstack([sn.A[hi], -sn.A[lo]]), b_ub=np.concatenate([sn.bu[hi], -sn.bl[lo]]),
                    A_eq=sn.A[eq] if eq.any() else None, b_eq=sn.bl[eq] if eq.any() else None,
                    bounds=[(None if np.isinf(l) else l, None if np.isinf(u) else u)
                            for l, u in zip(sn.lb, sn.ub)], method="highs")
        assert r.status in (0, 2, 3), (key, k, r.status, r.message)
        verdict[k] = r.status
        want[k] = np.nan
        if r.status == 0:
            x, ok = qp.solve(sn.A, sn.bl, sn.bu, sn.lb, sn.ub, sn.c, None)
            assert ok
            want[k] = float(np.dot(sn.c, x)) + sn.c0
    print(case, "HiGHS on the broken scenarios:", {k: int(verdict[k]) for k in SHIFTED + negated})
    # (the engine would have nothing to refuse otherwise)
    assert (verdict[list(negated)] == 3).all() and (verdict != 0).sum() >= 2
    _BROKEN[case] = (fam, verdict, want)
    return _BROKEN[case]


def check_broken_iter0(lib, device, case):
    """Iter0 quits; no infeasible scenario is OPTIMAL, no unbounded one OPTIMAL or
    INFEASIBLE (status 4 claims a proof that the feasible set is empty); every other
    scenario is OPTIMAL, finite, and at the oracle's objective to 1e-8."""
    so = BROKEN[case][1]
    fam, verdict, want = broken_family(case)
    ph = PH(ph_options(0, solver=so), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs,
            _native_lib=lib, _device=device)
    ph.PH_Prep()
    ph.subproblem_creation(False)
    with pytest.raises(SystemExit):
        ph.Iter0()
    status = ph._status.cpu().numpy().copy()
    st = ph.solve_stats[-1]
    print("%s: status of the broken scenarios %s; not_optimal %d infeasible %d"
          % (case, {int(k): int(status[k]) for k in np.nonzero(verdict)[0]}, st["not_optimal"], st["infeasible"]))
    assert (status[verdict == 2] != 1).all(), status[verdict == 2]
    assert np.isin(status[verdict == 3], (2, 3)).all(), status[verdict == 3]
    good = verdict == 0
    assert (status[good] == 1).all(), np.nonzero(good & (status != 1))[0]
    assert np.isfinite(ph._host("x")[:, good]).all()
    assert rel(ph._host("obj")[good], want[good]) < 1e-8
    assert st["infeasible"] == int((status == 4).sum())
    assert st["not_optimal"] == int(((status != 1) & (status != 4)).sum())
    return status, verdict


def check_broken_ph_main(lib, device, case, adopts):
    """ph_main with Iter0's checks deferred (test_engine_emu.check_infeasible_deferred_iter0
    on the lane, workgroup and sparse modes of the device loop): no PH iteration runs, as
    the reference quits right after Iter0 (phbase.py:812-823).  adopts (lane mode): the
    device loop adopts Iter0's pending solve and stops behind it.  In the workgroup and
    sparse modes Iter0's solve is the generic path's, final when it returns, and there
    is nothing to adopt: the checks quit before the loop, or a loop that is entered
    runs nothing."""
    so = BROKEN[case][1]
    fam = broken_family(case)[0]
    ph = PH(ph_options(20, solver=so), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs,
            _native_lib=lib, _device=device)
    seen = []
    orig = ph._native.iterk

    def spy(ctx, so_, a, res, stream):
        rc = orig(ctx, so_, a, res, stream)
        seen.append((res._obj.iters, res._obj.solves, res._obj.adopted))
        return rc
    ph._native.iterk = spy
    try:
        with pytest.raises(SystemExit):
            ph.ph_main()
    finally:
        ph._native.iterk = orig
    st = ph.solve_stats[0]
    print("%s: phx_iterk calls (iterations, solves, adopted) %s; Iter0 not_optimal %d infeasible %d; solves %d"
          % (case, seen, st["not_optimal"], st["infeasible"], len(ph.solve_stats)))
    if adopts:
        assert seen == [(0, 0, 1)], seen
    assert all(s[0] == 0 and s[1] == 0 for s in seen), seen
    assert ph._PHIter == 0 and len(ph.solve_stats) == 1
    return ph
