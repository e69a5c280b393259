"""PH loops under non-uniform scenario probabilities, unequal conditional node
probabilities, a per-(scenario, nonant) rho from a ``rho_setter`` and
``variable_probability``: the cases, the weights and the checks.
``test_weights.py`` runs them on the ABI emulation, ``test_weights_gpu.py`` on the HIP
kernels (the fused warm kernels, k_small_xw, k_xbar + k_update_w_seg and the
k_iter0_keep* kernels carry their own copies of the weighted arithmetic, which the
stand-alone entry points of test_reductions.py do not reach).

A case is one synthetic family (synth_cases.py) under one of three modes: "p"
(probabilities only: no rho setter, so Iter0 is deferred and adopted by the device
loop), "p_rho" (probabilities and the rho setter) and "rho" (the rho setter under
uniform probabilities).  The weights are closed forms of the scenario index k, the
stage-2 node v and the nonant slot j, the same whatever the batch size:

* two-stage trees: p_k ~ 1 + (5 k mod 7);
* three-stage trees: node v has conditional probability ~ 1 + (3 v mod 5), a leaf k
  inside its node ~ 1 + (5 k mod 7) normalised per node, p_k their product;
* rho[k, j] = 2 ** (((3 k + 5 j) mod 7) - 3): 1/8 .. 8, powers of two, differing
  across scenarios and slots;
* variable_probability: P[k, j] ~ 1 + (k (2 j + 3) mod 11) normalised per slot.

Checks (tolerances are the project's existing ones, none chosen here):

A  ``check_not_vacuous``: the oracle's weighted trajectory differs from its own
   uniform one (p = 1 / S, rho = 1) by more than 1e-3 in W and in x-bar (``rel``).
B  ``check_oracle``: the engine against the oracle continued from the engine's Iter0
   point under the same p, conditional probabilities and rho (check_vs_oracle's
   tolerances: trivial bound 1e-9, E[obj] 1e-8, x-bar 1e-8, W 1e-7, nonants 1e-6),
   every lane certified, every iteration run, and the engine's rho equal to the
   setter's bit for bit.  ``check_sampled_oracle``: the large batches' form (a sample
   of scenarios re-solved by the oracle from the engine's W / x-bar / rho).
C  ``check_prefix``: runs with PHIterLimit = k - 1 and k are deterministic prefixes of
   one another; from run k - 1's nonants and W and the device's own pc and rho, the
   per-(node, slot) sums of pc x and pc x^2, W + rho (x - x-bar) and conv recomputed
   with math.fsum must agree with run k's to 1e-12 relative
   (check_reductions_by_iteration's tolerance), and the device's pc and rho must be
   the case's.  No oracle is involved.
D  ``check_loops``: native_loop 0, iterk_fused 0 and starved lanes against the default
   run (check_paths' tolerances: W 1e-8, x-bar 1e-9, E[obj] 1e-9, trivial bound 1e-9).

The tolerances were fixed before any GPU run.  Worst error-to-tolerance ratio per path
(seed 1), as first measured:

* emulation, S = 70, nine cases (its device loop is never fused): B: W 4.3e-7, x-bar
  7.1e-8, nonants 4.2e-9, E[obj] 6.4e-8, trivial bound 3.2e-7; C: x-bar 6.9e-4, x-sq-bar
  8.2e-4, W 4.3e-2, conv 1.6e-3; D: W 5.1e-6 (starved; 0 on native_loop 0 and iterk_fused
  0, which repeat the default run bit for bit), x-bar 1.1e-6, E[obj] 4.3e-7, trivial
  bound 2.1e-7; variable_probability: W 4.4e-8, nonants 5.2e-10.
* MI355X, S = 70: B: W 8.5e-7, x-bar 1.5e-7, nonants 9.5e-9, E[obj] 1.4e-7, trivial
  bound 2.1e-7; C on phx_lane_warm_fz1 (two-stage, default): x-bar 2.1e-4, x-sq-bar
  2.1e-4, W 7.1e-3, conv 3.3e-4; C on k_small_xw (three-stage): x-bar 2.1e-4, x-sq-bar
  2.2e-4, W 1.4e-2, conv 1.1e-4; D: W 7.1e-7 (native_loop 0 and iterk_fused 0: k_small_xw
  against the fused kernel), 3.9e-6 (starved), x-bar 5.1e-7, E[obj] 2.2e-7, trivial bound
  2.1e-7; Iter0 deferred in the probabilities-only runs only, fused on the two-stage
  families only, 3 straggler stops in every starved run.
* MI355X, S = 1,100: C fused (18 blocks) x-bar 1.7e-4, x-sq-bar 2.5e-4, W 7.1e-3, conv
  5.6e-5; unfused (k_xbar + k_update_w_seg) 1.6e-4, 2.5e-4, 7.1e-3, 5.6e-5; sampled
  oracle: nonants 2.5e-10, objectives 3.9e-8; unfused against fused: W 2.1e-6, x-bar 3e-7.
* MI355X, S = 8,200 (k_iter0_keep): C x-bar 1.6e-4, x-sq-bar 2.0e-4, W 8.9e-4, conv
  1.1e-4; the trivial bound against the host sum 1.6e-4, deferred or not; sampled
  oracle: nonants 2.8e-10, objectives 1.9e-8.
* MI355X, S = 65,600 (phx_lane_warm_fzr2): C x-bar 1.7e-4, x-sq-bar 2.0e-4, W 7.1e-3,
  conv 1.7e-4; sampled oracle: nonants 2.5e-10, objectives 3.3e-8.
* MI355X, variable_probability: W 1.4e-7, x-bar 6.0e-8, nonants 2.5e-9; two ranks against
  one process (tolerance 1e-9): W 7.1e-6, the rest below 6.1e-7.
"""
import math

import numpy as np
import torch

import test_synth_structures as ts
from helpers import all_certified, ph_options, rel
from mpisppy_amd.extensions.extension import Extension
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.utils import sputils
from oracle import ph as oph

ITERS = 4
SEED = 1
MODES = {"p": (True, False), "p_rho": (True, True), "rho": (False, True)}
FAMILIES = ["vary_all", "eq_range_free", "multistage"]
# the loops of check D (test_synth_structures.PATHS entries)
LOOPS = {k: ts.PATHS[k] for k in ("host_loop", "unfused", "starved")}


# ---------------------------------------------------------------- weights
def scenario_weights(S):
    w = 1.0 + (5 * np.arange(S) % 7)
    return w / w.sum()


def tree_weights(bf):
    """(scenario probabilities, conditional node probabilities) of a three-stage tree."""
    nv, nl = bf
    node = 1.0 + (3 * np.arange(nv) % 5)
    node = node / node.sum()
    leaf = (1.0 + (5 * np.arange(nv * nl) % 7)).reshape(nv, nl)
    leaf = leaf / leaf.sum(axis=1, keepdims=True)
    return (node[:, None] * leaf).ravel(), node


def rho_values(S, N):
    k, j = np.arange(S)[:, None], np.arange(N)[None, :]
    return 2.0 ** (((3 * k + 5 * j) % 7) - 3.0)


def slot_probabilities(S, N, zero=None):
    """variable_probability's (S, N) table; zero = (k, j): that entry 0, its slot
    renormalised."""
    k, j = np.arange(S)[:, None], np.arange(N)[None, :]
    P = 1.0 + (k * (2 * j + 3) % 11)
    if zero is not None:
        P[zero] = 0.0
    return P / P.sum(axis=0, keepdims=True)


# ---------------------------------------------------------------- cases
class Case:
    """A family under a mode: ``fam`` (weighted SynthFamily), ``base`` (the same
    scenarios, uniform), ``p`` (S,), ``pc`` (S, N) the prob_coeff expected of the
    engine, ``rho`` (S, N) or None, ``groups[j]`` = [(node name, scenario indices)]."""

    def __init__(self, key, mode, S=70, seed=SEED):
        probs, rho = MODES[mode]
        self.key, self.mode, self.S = key, mode, S
        base = self.base = ts.family(key, seed, S)
        N = self.N = base.N
        node = None
        if not probs:
            self.fam, self.p = base, np.full(S, 1.0 / S)
        elif base.bf:
            self.p, node = tree_weights(base.bf)
            self.fam = base.weighted(self.p, node)
        else:
            self.p = scenario_weights(S)
            self.fam = base.weighted(self.p)
        self.rho = rho_values(S, N) if rho else None
        self.pc = np.tile(self.p[:, None], (1, N))
        allk = np.arange(S)
        self.groups = [[("ROOT", allk)] for _ in range(N)]
        if base.bf:
            nv, nl = base.bf
            cond = np.full(nv, 1.0 / nv) if node is None else node
            for j in range(base.stage_N[0], N):
                self.pc[:, j] = self.p / np.repeat(cond, nl)
                self.groups[j] = [("ROOT_%d" % v, allk[v * nl:(v + 1) * nl]) for v in range(nv)]

    def rho_setter(self, model):
        """The reference's contract: [(id(var), rho)] of a scenario model (nonant slot j
        is column j in every family here; run() asserts it)."""
        k = sputils.extract_num(model.name)
        return [(id(model._vars[j]), float(self.rho[k, j])) for j in range(self.N)]

    def oracle(self, ks=None):
        """An OraclePH of the case's scenarios (all, or the sample ks) with its rho."""
        o = oph.OraclePH(self.fam.scens(ks), rho=1.0)
        if self.rho is not None:
            o.rho[:] = self.rho if ks is None else self.rho[ks]
        return o


_CASES = {}


def case(key, mode, S=70):
    k = (key, mode, S)
    if k not in _CASES:
        _CASES[k] = Case(key, mode, S)
    return _CASES[k]


class PublishRho(Extension):
    """rho written in one device copy after Iter0 (a batch without per-scenario
    models has no rho_setter).  Only post_iter0 is overridden: no in-loop hook, so the
    device loop still runs.  ``rho_SN`` is set on the subclass that rho_extension makes."""
    rho_SN = None

    def post_iter0(self):
        ph = self.opt
        ph._rho.copy_(torch.as_tensor(np.ascontiguousarray(self.rho_SN.T).ravel()).to(ph.device))
        ph._bump()


def rho_extension(rho_SN):
    return type("PublishRhoCase", (PublishRho,), {"rho_SN": rho_SN})


# ---------------------------------------------------------------- engine runs
def run(lib, device, cs, iters, so=None, creator=None, extension=False, mpicomm=None, options=None):
    """PH on a case: rho through the rho_setter (per-scenario models), or, extension:
    through PublishRho (any creator)."""
    opts = ph_options(iters)
    opts.update(ts.solver(so))
    opts.update(options or {})
    fam = cs.fam
    setter = cs.rho_setter if cs.rho is not None and not extension else None
    ph = PH(opts, fam.names, creator or fam.creator, scenario_creator_kwargs=fam.kwargs,
            all_nodenames=fam.nodenames, rho_setter=setter,
            extensions=rho_extension(cs.rho) if extension else None, mpicomm=mpicomm, _native_lib=lib,
            _device=device)
    assert list(ph.batch.nonant.slot_col) == list(range(cs.N))
    conv, Eobj, tb = ph.ph_main()
    return ph, conv, Eobj, tb


def iter0_expectations(ph):
    """(what the loop left in the pinned Iter0 expectations, phx_expect on the kept Iter0
    objectives and statuses into a fresh buffer), both [3] float64."""
    lib = ph._native
    again = torch.full((3,), np.nan, dtype=torch.float64, device=ph.device)
    lib.check(ph._ctx, lib.expect(ph._ctx, ph._prob.data_ptr(), ph._iter0_obj_dev.data_ptr(),
                                  ph._iter0_status_dev.data_ptr(), again.data_ptr(), ph._stream()), "expect")
    return ph._iter0_exp_host.numpy().copy(), again.cpu().numpy()


def snapshot(cs, ph, conv, Eobj, tb, keep_x=False):
    """What the checks read of a run, as host arrays (the PH object is not kept)."""
    N, S = cs.N, cs.S
    st = getattr(ph, "iterk_stats", None)
    deferred = bool(getattr(ph, "_iter0_was_deferred", False))
    return dict(
        xn=ph.nonant_values(), W=ph.W_array(), xb=ph.xbar_by_node(), conv=conv, Eobj=Eobj, tb=tb,
        obj=ph._host("obj").copy(), x=ph._host("x").copy() if keep_x else None,
        pc=ph._pc.view(N, S).cpu().numpy().T.copy(), pc_host=ph._prob_coeff.T.copy(), rho=ph._host("rho").T.copy(),
        loc=np.asarray(ph.batch.nonant.slot_local), iters=ph._PHIter, certified=all_certified(ph),
        stats=None if st is None else dict(st), solve_stats=[dict(s) for s in ph.solve_stats],
        deferred=deferred, E1=getattr(ph, "E1", None), iter0_exp=iter0_expectations(ph) if deferred else None,
        iter0_obj=ph._iter0_obj.copy(), jit=ph._native.jit_info(ph._ctx).decode())


def prefix_runs(lib, device, cs, so=None, K=ITERS, creator=None, extension=False, keep_x=False):
    """Snapshots of the runs with PHIterLimit = 0..K."""
    out = []
    for k in range(K + 1):
        r = run(lib, device, cs, k, so, creator, extension)
        out.append(snapshot(cs, *r, keep_x=keep_x and k == 0))
        del r
    return out


def xbar_SN(cs, r, sq=False):
    """(S, N) x-bar (or x-sq-bar) of every scenario's nodes from a snapshot."""
    out = np.empty((cs.S, cs.N))
    for j in range(cs.N):
        for nd, ks in cs.groups[j]:
            out[ks, j] = r["xb"][nd][1 if sq else 0][r["loc"][j]]
    return out


def stragglers(r):
    return (r["stats"] or {}).get("stragglers", 0) + sum(s.get("stragglers", 0) for s in r["solve_stats"])


# ---------------------------------------------------------------- check A
_UNIFORM = {}


def _oracle_from_own_iter0(o, base, iters):
    """The oracle's iterations from its own Iter0 point (the LPs do not depend on the
    weights: the shared, unmodified Iter0 of test_synth_structures)."""
    o0 = ts.oracle_iter0(base)
    for k in range(o.S):
        o.x[k] = o0.x[k].copy()
    o.W_on = o.prox_on = 1
    o.iterk(iters, 1e-10)
    return o


def check_not_vacuous(cs, iters=ITERS):
    """Check A.  Returns (W difference, x-bar difference)."""
    if id(cs.base) not in _UNIFORM:
        _UNIFORM[id(cs.base)] = _oracle_from_own_iter0(oph.OraclePH(cs.base.scens(), rho=1.0), cs.base, iters)
    u = _UNIFORM[id(cs.base)]
    w = _oracle_from_own_iter0(cs.oracle(), cs.base, iters)
    dW, dx = rel(w.W, u.W), rel(w.xbar, u.xbar)
    print("A %s/%s: weighted vs uniform oracle: W %.2e x-bar %.2e" % (cs.key, cs.mode, dW, dx))
    assert dW > 1e-3 and dx > 1e-3, (dW, dx)
    return dW, dx


# ---------------------------------------------------------------- check B
def check_weights_uploaded(cs, r):
    """The device's prob_coeff is the case's (one division's rounding on a three-stage
    tree) and its host mirror; rho is the setter's bit for bit (all 1 without one)."""
    assert np.array_equal(r["pc"], r["pc_host"])
    assert rel(r["pc"] / cs.pc, 1.0) <= 4 * np.finfo(float).eps, rel(r["pc"] / cs.pc, 1.0)
    assert np.array_equal(r["rho"], np.ones((cs.S, cs.N)) if cs.rho is None else cs.rho)


def check_oracle(cs, runs, iters=ITERS):
    """Check B on prefix_runs(..., keep_x=True).  Returns the errors."""
    r0, r = runs[0], runs[iters]
    assert r0["certified"] and r["certified"], (r["solve_stats"], r["stats"])
    assert r["iters"] == iters, (r["iters"], r["conv"])
    check_weights_uploaded(cs, r)
    o0 = ts.oracle_iter0(cs.base)
    tb = math.fsum(cs.p[k] * o0.obj[k] for k in range(cs.S))
    o = cs.oracle()
    for k in range(cs.S):
        o.x[k] = r0["x"][:, k].copy()
    o.W_on = o.prox_on = 1
    o.iterk(iters, 1e-10)
    errs = {"tb": rel(r["tb"], tb), "Eobj": rel(r["Eobj"], o.Eobjective()), "xbar": rel(xbar_SN(cs, r), o.xbar),
            "W": rel(r["W"], o.W), "nonants": rel(r["xn"], o.xn()), "conv": rel(r["conv"], o.conv)}
    print("B %s/%s" % (cs.key, cs.mode), {k: "%.1e" % v for k, v in errs.items()})
    assert errs["tb"] < 1e-9
    assert errs["Eobj"] < 1e-8
    assert errs["xbar"] < 1e-8
    assert errs["W"] < 1e-7
    assert errs["nonants"] < 1e-6
    return errs


def check_sampled_oracle(cs, r, count=32):
    """Check B for the large batches (as test_large_batch_gpu): ``count`` random
    scenarios plus the first and the last re-solved by the oracle from the run's W,
    x-bar and rho; nonants to 1e-6, objectives to 1e-8."""
    sample = sorted(set(np.random.RandomState(7).randint(0, cs.S, count).tolist()) | {0, cs.S - 1})
    o = cs.oracle(sample)
    o.W_on = o.prox_on = 1
    o.W[:] = r["W"][sample]
    o.xbar[:] = xbar_SN(cs, r)[sample]
    o.solve_loop()
    errs = {"nonants": rel(o.xn(), r["xn"][sample]), "obj": rel(o.obj, r["obj"][sample])}
    print("B(sample) %s/%s S=%d" % (cs.key, cs.mode, cs.S), {k: "%.1e" % v for k, v in errs.items()})
    assert errs["nonants"] < 1e-6
    assert errs["obj"] < 1e-8
    return errs


# ---------------------------------------------------------------- check C
def check_prefix(cs, runs):
    """Check C on prefix_runs(...).  Returns the worst errors over the iterations."""
    worst = {"xbar": 0.0, "xsq": 0.0, "W": 0.0, "conv": 0.0}
    S, N = cs.S, cs.N
    for k in range(1, len(runs)):
        prev, cur = runs[k - 1], runs[k]
        assert prev["certified"] and cur["certified"], k
        assert cur["iters"] == k, (k, cur["iters"], cur["conv"])
        check_weights_uploaded(cs, cur)
        x, pc, rho = prev["xn"], cur["pc"], cur["rho"]
        xb, xsq = np.empty((S, N)), np.empty((S, N))
        for j in range(N):
            for nd, ks in cs.groups[j]:
                t = pc[ks, j] * x[ks, j]
                xb[ks, j] = math.fsum(t)
                xsq[ks, j] = math.fsum(t * x[ks, j])
        W = prev["W"] + rho * (x - xb)
        conv = math.fsum(np.abs(x - xb).ravel()) / (S * N)
        errs = {"xbar": rel(xbar_SN(cs, cur), xb), "xsq": rel(xbar_SN(cs, cur, sq=True), xsq), "W": rel(cur["W"], W),
                "conv": abs(cur["conv"] - conv) / max(1.0, conv)}
        for name, e in errs.items():
            assert e < 1e-12, (name, k, e)
            worst[name] = max(worst[name], e)
    print("C %s/%s S=%d" % (cs.key, cs.mode, S), {k: "%.1e" % v for k, v in worst.items()})
    return worst


# ---------------------------------------------------------------- check D
def check_loops(lib, device, cs, base, loops=LOOPS, iters=ITERS):
    """Check D: ``base`` is the default run's snapshot.  Returns {loop: snapshot}."""
    assert base["stats"] is not None
    out = {}
    for name, so in loops.items():
        r = out[name] = snapshot(cs, *run(lib, device, cs, iters, so))
        assert r["certified"] and r["iters"] == iters, name
        check_weights_uploaded(cs, r)
        errs = (rel(r["W"], base["W"]), rel(xbar_SN(cs, r), xbar_SN(cs, base)), rel(r["Eobj"], base["Eobj"]),
                rel(r["tb"], base["tb"]))
        print("D %s/%s %s" % (cs.key, cs.mode, name), ["%.1e" % e for e in errs],
              "stats", r["stats"] and {k: r["stats"][k] for k in ("fused", "stragglers", "straggler_stops")})
        assert errs[0] < 1e-8, name
        assert errs[1] < 1e-9, name
        assert errs[2] < 1e-9 and errs[3] < 1e-9, name
        assert (r["stats"] is None) == (name == "host_loop"), name
        if name == "host_loop":
            assert not r["deferred"]
        if name == "starved":
            assert stragglers(r) > 0
    return out


def check_which_loop(cs, r, fused=None):
    """The default run of a case: the device loop ran; Iter0 was deferred (and adopted)
    exactly without a rho setter; fused (the library only): as given."""
    assert r["stats"] is not None
    assert r["deferred"] == (cs.mode == "p"), (cs.mode, r["deferred"])
    if fused is not None:
        assert r["stats"]["fused"] == fused, r["stats"]


def check_case(lib, device, cs, fused=None, loops=LOOPS):
    """Checks B, C, D of one S = 70 case; fused: (default, unfused) as the library
    reports them, None on the emulation."""
    runs = prefix_runs(lib, device, cs, keep_x=True)
    check_which_loop(cs, runs[ITERS], None if fused is None else fused)
    errs = {"B": check_oracle(cs, runs), "C": check_prefix(cs, runs)}
    out = check_loops(lib, device, cs, runs[ITERS], loops)
    if fused is not None and "unfused" in out:
        assert out["unfused"]["stats"]["fused"] is False
    print("loops %s/%s: default %s deferred %s" % (cs.key, cs.mode, runs[ITERS]["stats"], runs[ITERS]["deferred"]))
    return runs, out, errs


# ---------------------------------------------------------------- variable_probability
def check_variable_probability(lib, device, key="vary_all", S=70, zero=None, iters=ITERS):
    """Per-slot probabilities on a synthetic family against the oracle with the same
    table (o.pc, prob0_mask), at check B's tolerances; W == 0 exactly where P == 0;
    the W mask runs in the host loop."""
    fam = ts.family(key, SEED, S)
    P = slot_probabilities(S, fam.N, zero)
    assert (zero is None) == bool((P != 0).all())

    def vp(model):
        k = sputils.extract_num(model.name)
        return [(id(model._vars[j]), float(P[k, j])) for j in range(fam.N)]

    def go(it):
        ph = PH(ph_options(it), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs, variable_probability=vp,
                _native_lib=lib, _device=device)
        return (ph,) + tuple(ph.ph_main())
    ph0 = go(0)[0]
    ph, conv, Eobj, tb = go(iters)
    assert all_certified(ph0) and all_certified(ph) and ph._PHIter == iters
    assert not hasattr(ph, "iterk_stats")
    assert np.array_equal(ph._pc.view(fam.N, S).cpu().numpy().T, P)
    o = oph.OraclePH(fam.scens(), rho=1.0)
    o.pc[:] = P
    o.prob0_mask = (P != 0).astype(float)
    x = ph0._host("x")
    for k in range(S):
        o.x[k] = x[:, k].copy()
    o.W_on = o.prox_on = 1
    o.iterk(iters, 1e-10)
    o0 = ts.oracle_iter0(fam)
    errs = {"tb": rel(tb, o0.trivial_bound), "Eobj": rel(Eobj, o.Eobjective()),
            "xbar": rel(ph.xbar_by_node()["ROOT"][0], o.xbar[0]), "W": rel(ph.W_array(), o.W),
            "nonants": rel(ph.nonant_values(), o.xn()), "conv": rel(conv, o.conv)}
    print("variable_probability %s zero=%s" % (key, zero), {k: "%.1e" % v for k, v in errs.items()})
    assert errs["tb"] < 1e-9
    assert errs["Eobj"] < 1e-8
    assert errs["xbar"] < 1e-8
    assert errs["W"] < 1e-7
    assert errs["nonants"] < 1e-6
    if zero is not None:
        assert np.all(ph.W_array()[P == 0] == 0.0) and np.any(ph.W_array()[P != 0] != 0.0)
        m = ph._models[fam.names[zero[0]]]
        assert ph.is_zero_prob(m, m._vars[zero[1]])
    return errs
