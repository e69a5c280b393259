"""Synthetic shared-pattern LP families for the solver tiers (test_synth_structures.py
on the ABI emulation, test_synth_structures_gpu.py on the kernels).

The example models reach few of the structures the lane solver is generated for
(csrc/phx_jit.h lane_kernel_source).  A family here is one sparsity pattern with
switchable features -- equality / range / one-sided rows, boxed / lower-only /
upper-only / free / fixed columns, a column without row entries, varying A entries,
varying costs / bounds / row sides, a pattern whose Cholesky has fill, a three-stage
tree -- and per-scenario numbers that are a closed-form function of the scenario
index, so a scenario is the same whatever the batch size (the lane module, cached by
source text, compiles once per family and seed).

Every instance is feasible and bounded by construction:

* a known point x0 lies strictly inside every inequality row and non-fixed bound and
  on every equality row; A, x0, the slacks and the per-scenario shifts are small
  dyadic fractions, so A x0 is exact in float64 (asserted here, for a sample of
  scenarios in rational arithmetic as well);
* a column without an upper bound has a positive cost, one without a lower bound a
  negative cost, so no recession direction over the one-sided columns improves;
* a free column has a defining equality or range row whose other columns are all
  boxed or fixed, so it cannot move along a recession direction and may carry any cost.

The same arrays feed the engine's ``scenario_creator`` (LinearModel), a vectorised
``batch_creator`` (BatchData) and the oracle's dense ``Scen`` objects.
"""
from fractions import Fraction

import numpy as np

from mpisppy_amd import model as lm
from mpisppy_amd.batch import BatchData, NonantSpec
from mpisppy_amd.scenario_tree import ScenarioNode
from mpisppy_amd.utils import sputils
from oracle import models as om

INF = np.inf

# column kinds: "lo" lower bound only, "up" upper bound only, "box", "free", "fixed";
# row kinds: "eq", "range", "le", "ge".
# Keys: n, m, N (nonants = the first N columns; a pair for a three-stage tree), cols /
# rows (kinds, cycled to n / m), empty (columns without row entries), nvar (varying A
# entries), c_vary / bnd_vary / rhs_vary, nnz (exact entry count), arrow (a pattern
# with Cholesky fill), finvary (a column whose upper bound is finite in odd scenarios
# only), bf (branching factors of the three-stage tree).
FAMILIES = {
    # the six structures of the GPU tests (n <= 10, m <= 6: seconds of hipRTC each)
    "eq_range_free": dict(n=9, m=5, N=3, cols=["lo", "box", "box", "free", "box", "free", "box", "lo", "box"],
                          rows=["eq", "range", "le", "eq", "ge"], nvar=3),
    "fixed_empty_upper": dict(n=9, m=4, N=3, cols=["lo", "box", "up", "fixed", "box", "up", "box", "lo", "box"],
                              rows=["le", "ge", "range", "le"], empty=[4], nvar=2),
    "vary_all": dict(n=8, m=5, N=3, cols=["box", "lo", "box", "lo", "up", "box", "lo", "box"],
                     rows=["le", "ge", "eq", "range", "le"], nvar=4, c_vary=True, bnd_vary=True, rhs_vary=True),
    "nvar0": dict(n=8, m=4, N=3, cols=["lo", "box", "lo", "box", "up", "box", "fixed", "lo"],
                  rows=["eq", "le", "ge", "range"], nvar=0, rhs_vary=True),
    "fill": dict(n=10, m=6, N=3, cols=["lo", "box", "box", "lo", "box", "up", "box", "lo", "box", "lo"],
                 rows=["le", "ge", "le", "range", "ge", "le"], arrow=True, nvar=3),
    "multistage": dict(n=10, m=5, N=(2, 2), bf=(7, 10),
                       cols=["lo", "box", "box", "lo", "free", "box", "up", "box", "lo", "box"],
                       rows=["eq", "le", "ge", "range", "le"], nvar=3, rhs_vary=True),
    # further small families of the CPU tests
    "plain": dict(n=8, m=4, N=3, cols=["lo", "box"], rows=["le", "ge"], nvar=3),
    "c_only": dict(n=8, m=4, N=3, cols=["lo", "box", "box", "up"], rows=["le", "ge", "range"], nvar=0, c_vary=True),
    "bnd_only": dict(n=8, m=4, N=3, cols=["lo", "box", "box", "up"], rows=["le", "eq", "ge"], nvar=0,
                     bnd_vary=True),
    "finvary": dict(n=8, m=4, N=3, cols=["lo", "box", "lo", "box"], rows=["le", "ge", "range"], nvar=2,
                    finvary=2),
}
_ALL_COLS = ["lo", "box", "box", "free", "up", "box", "fixed", "box"]
_ALL_ROWS = ["eq", "le", "range", "ge", "le", "ge"]
GPU_FAMILIES = ["eq_range_free", "fixed_empty_upper", "vary_all", "nvar0", "fill", "multistage"]


def sized_family(n, m, nnz=None, N=4):
    """Every feature at a given size (the lane solver's dispatch edges)."""
    return dict(n=n, m=m, N=N, cols=_ALL_COLS, rows=_ALL_ROWS, empty=[n - 1], nvar=6, c_vary=True, bnd_vary=True,
                rhs_vary=True, nnz=nnz)


def _spec(family):
    return dict(FAMILIES[family]) if isinstance(family, str) else dict(family)


def _dy(rng, lo, hi, den, size):
    """Random dyadic fractions k / den in [lo, hi]."""
    return rng.randint(int(lo * den), int(hi * den) + 1, size=size) / float(den)


def _pattern(rng, n, m, ckind, rkind, empty, arrow, nnz):
    """Row column-sets of one pattern: every row has two entries or more, every
    non-empty column one or more, a free column's defining row is otherwise boxed."""
    if arrow:
        # rows 1.. on disjoint column pairs, row 0 on one column of each: the normal
        # matrix is an arrow, and eliminating row 0 fills the rest
        assert n >= 2 * (m - 1) and not empty
        rows = [set(range(0, 2 * (m - 1), 2))] + [{2 * i - 2, 2 * i - 1} for i in range(1, m)]
        for j in range(2 * (m - 1), n):
            rows[1 + (j % (m - 1))].add(j)
        return [sorted(r) for r in rows], {}
    closed_ok = [j for j in range(n) if ckind[j] in ("box", "fixed") and j not in empty]
    live = [j for j in range(n) if j not in empty]
    frees = [j for j in live if ckind[j] == "free"]
    defrows = [i for i in range(m) if rkind[i] in ("eq", "range")]
    assert len(frees) <= len(defrows) and len(frees) < m, "a free column needs a defining row of its own"
    defining = {}
    for f, i in zip(frees, rng.permutation(defrows)[:len(frees)]):
        defining[int(i)] = f
    per_row = max(2, min(len(live), (nnz // m) if nnz else 3))
    rows = []
    for i in range(m):
        if i in defining:
            k = min(len(closed_ok), max(2, per_row - 1))
            rows.append({defining[i]} | set(rng.choice(closed_ok, k, replace=False).tolist()))
        else:
            rows.append(set(rng.choice(live, per_row, replace=False).tolist()))

    def fits(i, j):
        return j not in rows[i] and (i not in defining or j in closed_ok)
    for j in live:
        if not any(j in r for r in rows):
            rows[int(rng.choice([i for i in range(m) if fits(i, j)]))].add(j)
    if nnz:
        while sum(len(r) for r in rows) > nnz:
            i = int(rng.randint(m))
            drop = [j for j in rows[i] if j != defining.get(i) and sum(j in r for r in rows) > 1]
            if len(rows[i]) > 2 and drop:
                rows[i].remove(int(rng.choice(drop)))
        while sum(len(r) for r in rows) < nnz:
            i, j = int(rng.randint(m)), int(rng.choice(live))
            if fits(i, j):
                rows[i].add(j)
    return [sorted(r) for r in rows], defining


class SynthFamily:
    """One family at one seed: ``creator`` / ``names`` / ``kwargs`` / ``nodenames`` for
    the engine, ``scens()`` for the oracle, ``flags`` the features realised.  ``prob`` /
    ``node_prob``: optional scenario probabilities and conditional probabilities of the
    stage-2 nodes (weight_cases.py); they reach the creator, the batch creator and
    ``scen()`` and nothing else (the numbers drawn do not depend on them)."""

    DRAWS = 32

    def __init__(self, family, seed, n=None, m=None, N=None, S=70, prob=None, node_prob=None):
        # PH has work to do only where the scenarios disagree on a nonant.  Nothing in
        # the construction forces that (every nonant may sit at a shared bound), so
        # the numbers are drawn again, from the next stream of the same seed, until
        # the plain LPs of the first scenarios disagree -- decided by scipy's HiGHS
        # alone, never by the engine or by the oracle's verdict on the engine; an LP
        # HiGHS cannot solve is an error here, not a reason to draw again
        for draw in range(self.DRAWS):
            self._build(family, seed, draw, n, m, N, S)
            if self._nonants_disagree():
                break
        else:
            raise RuntimeError("synth family %s seed %d: no draw on which the scenarios disagree" % (family, seed))
        self.flags["draw"] = draw
        if prob is not None or node_prob is not None:
            self._set_weights(prob, node_prob)

    def _set_weights(self, prob, node_prob):
        """Scenario probabilities (S,) and, on a three-stage tree, the conditional
        probabilities (bf[0],) of the stage-2 nodes; None: 1 / S and 1 / bf[0], by the
        expressions a family without weights has always used."""
        self.prob = None if prob is None else np.asarray(prob, dtype=np.float64).copy()
        self.node_prob = None if node_prob is None else np.asarray(node_prob, dtype=np.float64).copy()
        assert self.prob is None or self.prob.shape == (self.S,)
        assert self.node_prob is None or (self.bf and self.node_prob.shape == (self.bf[0],))
        self.creator = self._make_creator()

    def weighted(self, prob=None, node_prob=None):
        """The same scenarios (shared arrays, no new draw) under other probabilities."""
        import copy
        fam = copy.copy(self)
        fam._set_weights(prob, node_prob)
        return fam

    def scen_prob(self, k):
        return 1.0 / self.S if self.prob is None else float(self.prob[k])

    def node_cond_prob(self, v):
        return 1.0 / self.bf[0] if self.node_prob is None else float(self.node_prob[v])

    def _nonants_disagree(self, count=8, tol=1e-2):
        from scipy.optimize import linprog
        xs = []
        for k in range(min(count, self.S)):
            A = self.dense_A(k)
            eq = self.bl[k] == self.bu[k]
            lo, hi = np.isfinite(self.bl[k]) & ~eq, np.isfinite(self.bu[k]) & ~eq
            r = linprog(self.c[k], A_ub=np.vstack([A[hi], -A[lo]]), b_ub=np.concatenate([self.bu[k][hi], -self.bl[k][lo]]),
                        A_eq=A[eq] if eq.any() else None, b_eq=self.bl[k][eq] if eq.any() else None,
                        bounds=[(None if np.isinf(l) else l, None if np.isinf(u) else u)
                                for l, u in zip(self.lb[k], self.ub[k])], method="highs")
            if r.status != 0:
                raise RuntimeError("synth family %s: HiGHS status %d (%s) on a scenario with a known feasible "
                                   "point" % (self.family, r.status, r.message))
            xs.append(r.x[:self.N])
        xs = np.array(xs)
        return bool((xs.max(axis=0) - xs.min(axis=0)).max() > tol)

    def _build(self, family, seed, draw, n, m, N, S):
        sp = _spec(family)
        self.family = family if isinstance(family, str) else "sized"
        n = self.n = n or sp["n"]
        m = self.m = m or sp["m"]
        N = N or sp["N"]
        self.S = S
        self.prob = self.node_prob = None
        self.stage_N = tuple(N) if isinstance(N, (tuple, list)) else (N,)
        self.N = sum(self.stage_N)
        self.bf = sp.get("bf")
        assert (self.bf is None) == (len(self.stage_N) == 1)
        if self.bf:
            assert S == self.bf[0] * self.bf[1]
        rng = np.random.RandomState(4096 * (sorted(FAMILIES).index(family) + 1 if isinstance(family, str)
                                            else 97 * n + m) + self.DRAWS * seed + draw)
        ckind = self.ckind = [sp["cols"][j % len(sp["cols"])] for j in range(n)]
        rkind = self.rkind = [sp["rows"][i % len(sp["rows"])] for i in range(m)]
        empty = self.empty = list(sp.get("empty", []))
        for j in empty:
            if ckind[j] == "free":
                ckind[j] = "box"
        # a free column needs a defining row of its own: the surplus is boxed
        ndef = min(sum(k in ("eq", "range") for k in rkind), m - 1)
        for j in [j for j in range(n) if ckind[j] == "free"][ndef:]:
            ckind[j] = "box"
        nonant_kinds = set(ckind[:self.N])
        assert {"lo", "box"} <= nonant_kinds, "the nonants include a lower-only and a boxed column"
        self.c_vary, self.bnd_vary, self.rhs_vary = (bool(sp.get(k)) for k in ("c_vary", "bnd_vary", "rhs_vary"))
        finvary = sp.get("finvary")
        rows, defining = _pattern(rng, n, m, ckind, rkind, empty, sp.get("arrow"), sp.get("nnz"))
        self.rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        self.colidx = np.concatenate(rows).astype(np.int32)
        self.rowof = np.repeat(np.arange(m), [len(r) for r in rows])
        nnz = self.nnz = len(self.colidx)
        s = np.arange(S, dtype=np.int64)

        def shift(count, den):
            """(S, count) per-scenario dyadic shifts ((s a + b) mod 16) / den, a odd."""
            a, b = 2 * rng.randint(0, 8, count) + 1, rng.randint(0, 16, count)
            return ((s[:, None] * a[None, :] + b[None, :]) % 16) / float(den)

        x0 = self.x0 = _dy(rng, -4, 4, 2, n)
        base = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], nnz)
        # varying entries: off the equality rows unless the row sides vary too
        cand = [k for k in range(nnz) if self.rhs_vary or rkind[self.rowof[k]] != "eq"]
        # (entries of nonant columns first: the scenarios must disagree on the nonants)
        cand = [k for k in cand if self.colidx[k] < self.N] + [k for k in cand if self.colidx[k] >= self.N]
        nv = min(sp.get("nvar", 0), len(cand))
        near = min(len(cand), 2 * nv)
        vark = np.sort(rng.choice(cand[:near], nv, replace=False)) if nv else []
        A = np.tile(base, (S, 1))
        spread = np.zeros(nnz)
        if len(vark):
            A[:, vark] += shift(len(vark), 16) - 0.5             # in [-1/2, 1/2): never zero
            spread[vark] = 0.5
        self.vark = np.asarray(vark, dtype=np.int64)
        act = np.zeros((S, m))
        np.add.at(act.T, self.rowof, (A * x0[self.colidx][None, :]).T)
        # the row activity of x0 over every possible shift (not only this batch's)
        mid = np.zeros(m)
        np.add.at(mid, self.rowof, base * x0[self.colidx])
        rad = np.zeros(m)
        np.add.at(rad, self.rowof, spread * np.abs(x0[self.colidx]))
        # rows tighter than the bounds' boxes, so that rows (and their varying entries)
        # decide the vertex and PH has something to agree on
        gl, gu = _dy(rng, 0.25, 1, 4, m), _dy(rng, 0.25, 1, 4, m)
        if self.rhs_vary:
            bl = act - gl[None, :] - shift(m, 8)
            bu = act + gu[None, :] + shift(m, 8)
        else:
            bl = np.tile(mid - rad - gl, (S, 1))
            bu = np.tile(mid + rad + gu, (S, 1))
        for i, kd in enumerate(rkind):
            if kd == "eq":
                assert self.rhs_vary or rad[i] == 0.0
                bl[:, i] = bu[:, i] = act[:, i]
            elif kd == "le":
                bl[:, i] = -INF
            elif kd == "ge":
                bu[:, i] = INF
        dl, du = _dy(rng, 2, 6, 2, n), _dy(rng, 2, 6, 2, n)
        lb = np.tile(x0 - dl, (S, 1))
        ub = np.tile(x0 + du, (S, 1))
        if self.bnd_vary:
            lb -= shift(n, 8)
            ub += shift(n, 8)
        for j, kd in enumerate(ckind):
            if kd in ("lo", "free"):
                ub[:, j] = INF
            if kd in ("up", "free"):
                lb[:, j] = -INF
            if kd == "fixed":
                lb[:, j] = ub[:, j] = x0[j]
        if finvary is not None:
            assert ckind[finvary] == "lo"
            ub[1::2, finvary] = x0[finvary] + du[finvary]
        mag = _dy(rng, 0.5, 6, 4, n)
        sign = rng.choice([-1.0, 1.0], n)
        for j, kd in enumerate(ckind):
            sign[j] = 1.0 if kd == "lo" else -1.0 if kd == "up" else sign[j]
        c = np.tile(sign * mag, (S, 1))
        if self.c_vary:
            c *= 1.0 + shift(n, 16)                              # in [1, 2): the signs stay
        self.A, self.bl, self.bu, self.lb, self.ub, self.c = A, bl, bu, lb, ub, c
        self.c0 = 3.5
        self.names = ["scen%d" % k for k in range(S)]
        self.kwargs = {}
        self.nodenames = sputils.create_nodenames_from_branching_factors(list(self.bf)) if self.bf else None
        self.var_names = ["x%d" % j for j in range(n)]
        self._check_known_point()
        fin_l, fin_u = np.isfinite(lb), np.isfinite(ub)
        self.flags = dict(
            n=n, m=m, nnz=nnz, N=self.N, nvar=len(self.vark), c_vary=self.c_vary,
            bnd_vary=bool(self.bnd_vary or finvary is not None), rhs_vary=self.rhs_vary,
            rows={k: rkind.count(k) for k in ("eq", "range", "le", "ge")},
            cols={k: ckind.count(k) for k in ("lo", "up", "box", "free", "fixed")},
            empty_cols=len(empty), arrow=bool(sp.get("arrow")), stages=len(self.stage_N) + 1,
            finiteness_varies=bool((fin_l != fin_l[0]).any() or (fin_u != fin_u[0]).any()))
        self.creator = self._make_creator()

    # ------------------------------------------------------------ construction checks
    def _check_known_point(self):
        x0, S = self.x0, self.S
        act = np.zeros((S, self.m))
        np.add.at(act.T, self.rowof, (self.A * x0[self.colidx][None, :]).T)
        for i, kd in enumerate(self.rkind):
            if kd == "eq":
                assert (act[:, i] == self.bl[:, i]).all() and (act[:, i] == self.bu[:, i]).all()
            else:
                assert (act[:, i] > self.bl[:, i]).all() and (act[:, i] < self.bu[:, i]).all()
            if kd == "range":
                assert np.isfinite(self.bl[:, i]).all() and np.isfinite(self.bu[:, i]).all()
        for j, kd in enumerate(self.ckind):
            if kd == "fixed":
                assert (self.lb[:, j] == x0[j]).all() and (self.ub[:, j] == x0[j]).all()
            else:
                assert (self.lb[:, j] < x0[j]).all() and (x0[j] < self.ub[:, j]).all()
            assert (self.c[np.isinf(self.ub[:, j]), j] > 0).all() or kd == "free"
            assert (self.c[np.isinf(self.lb[:, j]), j] < 0).all() or kd == "free"
        assert (self.A != 0.0).all()
        # the same in rational arithmetic (float64 holds these dyadic values exactly)
        for k in sorted({0, 1, S // 2, S - 1}):
            for i in range(self.m):
                ks = range(self.rowptr[i], self.rowptr[i + 1])
                r = sum(Fraction(float(self.A[k, e])) * Fraction(float(x0[self.colidx[e]])) for e in ks)
                assert r == Fraction(float(act[k, i]))
                if np.isfinite(self.bl[k, i]):
                    assert Fraction(float(self.bl[k, i])) <= r
                if np.isfinite(self.bu[k, i]):
                    assert r <= Fraction(float(self.bu[k, i]))

    # ------------------------------------------------------------ engine side
    def _node_cols(self):
        out, j = [], 0
        for cnt in self.stage_N:
            out.append(list(range(j, j + cnt)))
            j += cnt
        return out

    def _make_creator(self):
        fam = self

        def scenario_creator(name):
            k = sputils.extract_num(name)
            m = lm.LinearModel(name)
            v = [m.add_var(fam.var_names[j], None if np.isinf(fam.lb[k, j]) else fam.lb[k, j],
                           None if np.isinf(fam.ub[k, j]) else fam.ub[k, j]) for j in range(fam.n)]
            for i in range(fam.m):
                e = slice(fam.rowptr[i], fam.rowptr[i + 1])
                m.add_row(fam.colidx[e], fam.A[k, e], None if np.isinf(fam.bl[k, i]) else fam.bl[k, i],
                          None if np.isinf(fam.bu[k, i]) else fam.bu[k, i])
            m.set_objective(lm.LinExpr({j: fam.c[k, j] for j in range(fam.n)}, fam.c0, m), lm.minimize)
            cols = fam._node_cols()
            first = lm.LinExpr({j: fam.c[k, j] for j in cols[0]}, 0.0, m)
            if fam.bf is None:
                sputils.attach_root_node(m, first, [v[j] for j in cols[0]])
            else:
                second = lm.LinExpr({j: fam.c[k, j] for j in cols[1]}, 0.0, m)
                node = k // fam.bf[1]
                m._mpisppy_node_list = [
                    ScenarioNode("ROOT", 1.0, 1, first, [v[j] for j in cols[0]], m),
                    ScenarioNode("ROOT_%d" % node, fam.node_cond_prob(node), 2, second, [v[j] for j in cols[1]], m,
                                 parent_name="ROOT")]
            m._mpisppy_probability = fam.scen_prob(k)
            return m
        return scenario_creator

    def batch_creator_fn(self):
        """The same creator with a vectorised ``batch_creator`` attached (two-stage
        families; the arrays from_models would extract from the per-scenario models)."""
        assert self.bf is None
        fam = self
        creator = self._make_creator()

        def batch_creator(names):
            ks = np.array([sputils.extract_num(nm) for nm in names])
            spec = NonantSpec(list(range(fam.N)), [1] * fam.N, list(range(fam.N)), [None], [np.ones(len(ks))],
                              fam.var_names[:fam.N])
            return BatchData(names, fam.rowptr, fam.colidx, fam.A[ks], fam.bl[ks], fam.bu[ks], fam.lb[ks],
                             fam.ub[ks], fam.c[ks], fam.c0, lm.minimize, [fam.scen_prob(k) for k in ks], spec,
                             list(fam.var_names))
        creator.batch_creator = batch_creator
        return creator

    # ------------------------------------------------------------ oracle side
    def dense_A(self, k):
        A = np.zeros((self.m, self.n))
        A[self.rowof, self.colidx] = self.A[k]
        return A

    def scen(self, k):
        cols = self._node_cols()
        nodes = [("ROOT", 1.0, 1, cols[0])]
        if self.bf:
            nodes.append(("ROOT_%d" % (k // self.bf[1]), self.node_cond_prob(k // self.bf[1]), 2, cols[1]))
        return om.Scen(self.names[k], self.var_names, self.c[k], self.c0, self.dense_A(k), self.bl[k], self.bu[k],
                       self.lb[k], self.ub[k], nodes, self.scen_prob(k))

    def scens(self, ks=None):
        return [self.scen(k) for k in (range(self.S) if ks is None else ks)]


def synth_family(family, seed, n=None, m=None, N=None, S=70):
    """A deterministic function of its arguments: (scenario_creator, the same scenarios
    as oracle.models.Scen, the feature flags realised).  The tests keep the SynthFamily
    itself, which also carries the names, the tree and the arrays."""
    fam = SynthFamily(family, seed, n, m, N, S)
    return fam.creator, fam.scens(), fam.flags


# ---------------------------------------------------------------- structure recomputation
def symbolic_fill(rowptr, colidx, m):
    """(pair positions, L pattern) of the packed lower triangle of A D A': rows i, j
    pair when they share a column; the symbolic Cholesky adds the fill."""
    rows = [set(colidx[rowptr[i]:rowptr[i + 1]].tolist()) for i in range(m)]
    pos = lambda i, j: i * (i + 1) // 2 + j
    pair = np.zeros(m * (m + 1) // 2, dtype=bool)
    for i in range(m):
        for j in range(i + 1):
            pair[pos(i, j)] = i == j or bool(rows[i] & rows[j])
    lnz = pair.copy()
    for jj in range(m):
        for i in range(jj + 1, m):
            for k in range(jj):
                if lnz[pos(i, k)] and lnz[pos(jj, k)]:
                    lnz[pos(i, jj)] = True
    return pair, lnz
