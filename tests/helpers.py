"""Shared helpers for the parity tests (run the engine and the oracle side by side)."""
import numpy as np

import mpisppy_amd  # noqa: F401
from mpisppy_amd.opt.ph import PH
from oracle import models as om, ph as oph


def ph_options(iters, rho=1.0, convthresh=1e-10, solver=None):
    return {"solver_name": "phx", "PHIterLimit": iters, "defaultPHrho": rho, "convthresh": convthresh,
            "verbose": False, "display_progress": False,
            "iter0_solver_options": dict(solver or {}), "iterk_solver_options": dict(solver or {})}


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def run_engine(creator, names, kwargs, iters, rho=1.0, lib=None, device=None, all_nodenames=None,
               options=None, mpicomm=None):
    opts = ph_options(iters, rho)
    if options:
        opts.update(options)
    ph = PH(opts, names, creator, scenario_creator_kwargs=kwargs, all_nodenames=all_nodenames,
            mpicomm=mpicomm, _native_lib=lib, _device=device)
    conv, Eobj, tb = ph.ph_main()
    return ph, conv, Eobj, tb


REF_XBAR = np.array([96.88717449844287, 274.2239371483933, 128.88888831920772])
REF_W = np.array([[-16.10425295139681, 70.84705093609978, -54.742797934166234],
                  [-41.104251445950844, 89.57647412029155, -48.47222265026873],
                  [57.20850439734766, -160.42352505639107, 103.21502058443501]])


def oracle_continue_from(ph_iter0, scens, iters, rho=1.0, convthresh=1e-10):
    """The oracle's PH iterations 1..iters started from the engine's Iter0 point
    (degenerate Iter0 LPs may have several optimal vertices; from iteration 1 on the
    prox term makes each subproblem's nonant optimum unique, so the trajectories must
    agree).  ph_iter0: an engine run with PHIterLimit = 0."""
    o = oph.OraclePH(scens, rho=rho)
    x = ph_iter0._host("x")
    for k in range(len(scens)):
        o.x[k] = x[:, k].copy()
    o.W_on = o.prox_on = 1
    o.iterk(iters, convthresh)
    return o


def _by_index(terms, idx, size):
    """(S, size) sums of the (S, K) terms over equal idx[k] (numpy only: a loop over the
    deepest group, not over scenarios or entries)."""
    out = np.zeros((terms.shape[0], size), dtype=terms.dtype)
    if terms.shape[1] == 0:
        return out
    order = np.argsort(idx, kind="stable")
    sidx = np.asarray(idx)[order]
    start = np.searchsorted(sidx, sidx, side="left")
    rank = np.arange(len(sidx)) - start               # position of an entry inside its group
    for r in range(int(rank.max()) + 1):
        sel = rank == r
        out[:, sidx[sel]] += terms[:, order[sel]]
    return out


def kkt_recheck(ph, kkt_tol=1e-9, tag=""):
    """The row duals y of the engine's last solve against its own x, independent of the
    kernels' certificates, from the engine's host data (ph.batch, the cost as the library
    was given it, W / rho / x-bar when PH terms were on: ph._PHIter > 0), vectorised over
    the scenarios.  The rule is the oracle's (oracle/qp.py _certified), which every
    tier's certificate states in unscaled quantities, for the minimisation form:

        q = c (+ W - rho x-bar on the nonant columns),  p = rho there, else 0
        z = p o x + q - A'y,         dtol = kkt_tol (1 + max_j |q_j|)
        z_j >= -dtol unless column j is at ub,   z_j <= dtol unless it is at lb
        y_i >= -dtol unless row i is at bu,      y_i <= dtol unless it is at bl

    "at" a bound or side: within 1e-9 (1 + |bound|), host_recheck's primal tolerance; a
    fixed column and an equality row are at both, so free.  Every y is finite.  z is
    evaluated in extended precision where numpy has it; dtol is widened only by the
    rounding of a float64 evaluation of z_j, (k_j + 3) 2^-53 sum|terms of z_j| with k_j
    the column's non-zeros, so that a ratio of exactly 1 does not flip.  kkt_tol is the
    solver option the run used, not a tuned figure.  Returns and prints the four worst
    violation-to-dtol ratios (z below, z above, y below, y above); each must be <= 1.

    Worst ratios (z, y) on the host emulation, measured before any GPU run: the lane,
    interior-point, unfused, starved and host-loop paths of the small synthetic
    families 3.4e-7, 0; their PDHG path 3.6e-7, 0.35 (fixed_empty_upper); the families
    beyond the lane limits on the workgroup / sparse / PDHG tiers 2.5e-6, 2.4e-8; sslp
    6.6e-7, 0; netdes 2.1e-7, 0; farmer 1.7e-9, 0; farmer cm=10 (S = 6) 9.4e-9, 0;
    aircond 2.9e-7, 0.
    First run on the MI355X, worst per tier: lane kernels (fused and unfused device
    loop, host loop, interior point; S = 70 .. 197,120) 3.0e-7, 0; PDHG + polish on the
    small families 3.0e-7, 0.28 (fixed_empty_upper), starved lanes finished by another
    tier 2.0e-7, 0.070; workgroup, sparse and PDHG tiers beyond the lane limits 4.7e-7,
    0; farmer cm=10 at S = 1,000: workgroup pass 1.1e-8, 0.0025, without it 1.0e-8,
    0.0021; sslp 7.7e-7, 0; netdes 2.1e-7, 0; farmer on the fused loop 3.0e-9, 0, its
    lanes finished after a straggler stop 2.2e-9, 0; aircond (every phx_lane_all build)
    2.8e-7, 0.  No tier's duals needed a fix."""
    ph._settle()
    b = ph.batch
    S, n, m, N = ph._S, b.n, b.m, b.nonant.N
    ld = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64
    host = lambda t: t.detach().cpu().numpy()
    per = lambda a, k: np.broadcast_to(np.asarray(a, dtype=np.float64), (S, k))
    x = host(ph._x).reshape(n, S).T
    y = host(ph._y).reshape(-1, S)[:m].T
    assert np.isfinite(y).all(), "%s: a row dual is not finite" % tag
    c = host(ph._dev["c"])
    c = c.reshape(n, S).T if b.c_vary else per(c, n)
    if b.kvar is None:
        A = b.A_full
    elif b.nvar == 0:
        A = b.Aconst
    else:
        A = np.where(b.kvar[None, :] < 0, b.Aconst[None, :], b.Avar[np.maximum(b.kvar, 0)].T)
    A = per(A, b.nnz)
    rowof = np.repeat(np.arange(m), np.diff(b.rowptr))
    lb, ub, bl, bu = per(b.lb, n), per(b.ub, n), per(b.bl, m), per(b.bu, m)
    cols = b.nonant.slot_col
    fixed = getattr(ph, "_fixed", None)
    if fixed is not None and fixed.any():
        lb, ub = lb.copy(), ub.copy()                  # a fixed nonant: lb = ub = its value
        lb[:, cols] = np.where(fixed, x[:, cols], lb[:, cols])
        ub[:, cols] = np.where(fixed, x[:, cols], ub[:, cols])
    # q, p and the terms of z
    q = c.astype(ld)
    zabs = np.abs(c)
    px = np.zeros((S, n), dtype=ld)
    if ph._PHIter > 0 and N:
        W, rho = host(ph._W).reshape(N, S).T, host(ph._rho).reshape(N, S).T
        xb = host(ph._xbar_node)[ph._xbar_idx].T
        rxb = rho.astype(ld) * xb
        q[:, cols] += W - rxb
        zabs[:, cols] += np.abs(W) + np.abs(rho * xb)
        px[:, cols] = rho.astype(ld) * x[:, cols]
    ay = A.astype(ld) * y[:, rowof]
    z = px + q - _by_index(ay, b.colidx, n)
    zabs = zabs + np.abs(px).astype(np.float64) + _by_index(np.abs(ay).astype(np.float64), b.colidx, n)
    kj = np.bincount(b.colidx, minlength=n)
    dtol = kkt_tol * (1.0 + (np.max(np.abs(q), axis=1) if n else np.zeros(S))).astype(np.float64)
    ztol = dtol[:, None] + (kj[None, :] + 3) * 2.0 ** -53 * zabs
    act = _by_index(A.astype(ld) * x[:, b.colidx], rowof, m).astype(np.float64)
    fin = lambda a: np.where(np.isfinite(a), a, 0.0)
    with np.errstate(invalid="ignore"):
        at_lb = np.isfinite(lb) & (x - lb <= 1e-9 * (1.0 + np.abs(fin(lb))))
        at_ub = np.isfinite(ub) & (ub - x <= 1e-9 * (1.0 + np.abs(fin(ub))))
        at_bl = np.isfinite(bl) & (act - bl <= 1e-9 * (1.0 + np.abs(fin(bl))))
        at_bu = np.isfinite(bu) & (bu - act <= 1e-9 * (1.0 + np.abs(fin(bu))))
    z = z.astype(np.float64)

    def worst(v, tol, free):
        r = np.where(free, 0.0, v / tol)
        return max(float(r.max()), 0.0) + 0.0 if r.size else 0.0

    ratios = (worst(-z, ztol, at_ub), worst(z, ztol, at_lb),
              worst(-y, dtol[:, None], at_bu), worst(y, dtol[:, None], at_bl))
    print("[kkt %s] S=%d n=%d m=%d iter=%d worst violation/dtol: z below %.3g, z above %.3g, "
          "y below %.3g, y above %.3g" % ((tag, S, n, m, ph._PHIter) + ratios))
    assert max(ratios) <= 1.0, (tag, ratios)
    return ratios


def all_certified(ph):
    """Every solve certified: the host loop's per-solve statistics and, when the
    device loop (phx_iterk) ran the iterations, its count of uncertified lanes."""
    return (all(s["not_optimal"] == 0 for s in ph.solve_stats)
            and getattr(ph, "iterk_stats", {}).get("not_optimal", 0) == 0)
