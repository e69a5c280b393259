"""NormRhoUpdater, NormRhoConverger and PrimalDualConverger end to end: the
engine's host loop with the device-side update against the CPU oracle with a
numpy restatement of the reference's ``miditer``
(``mpisppy/extensions/norm_rho_updater.py:112-158``) and of the two
convergers, inserted between ``convergence_diff`` and the stop test
(phbase.py:914-926).

Parity cases (primal_dual_difference_factor 10, defaultPHrho 1): farmer with 3
scenarios over 30 iterations and hydro with 9 (three stages, node-indexed
x-bar) over 20.  The oracle continues from the engine's Iter0 point, as
helpers.oracle_continue_from does (hydro's Iter0 LPs are degenerate).  From
there farmer takes 10 increases and 8 decreases and the closest comparison of
the rule has a relative margin of 8.8e-3; hydro takes 10 increases, 50
decreases and 133 converged decreases with a margin of 1.8e-2 (from the
oracle's own Iter0 vertex: 8 / 43 / 125, margin 7.1e-2).  The test asserts a
margin of at least 1e-4, that every kind of action occurred, the same actions
at every iteration, a final rho equal to the oracle's bit for bit (products of
the same factors in the same order), and x-bar, W and conv within the
tolerances of the fixed-rho parity tests of the same models
(test_gpu_parity.test_farmer3_golden: 1e-9 / 1e-8 / 1e-7; test_hydro: 1e-8 /
1e-6 / 1e-6), fixed on the emulation before any GPU run.  Worst figures
(x-bar / W / conv): emulation farmer 1.2e-15 / 9.1e-15 / 7.1e-14, hydro
1.2e-14 / 7.5e-14 / 2.3e-15; first run on the MI355X farmer 8.4e-16 / 1.4e-14
/ 4.0e-14, hydro 3.7e-14 / 2.8e-13 / 3.8e-14.  The converger's gaps, engine
against oracle: emulation 3.8e-13 (farmer) and 1.4e-13 (hydro), MI355X 4.0e-13
and 5.0e-13.
"""
import math

import numpy as np
import pytest
import torch

from helpers import all_certified, ph_options, rel
from mpisppy_amd.convergers.norm_rho_converger import NormRhoConverger
from mpisppy_amd.convergers.primal_dual_converger import PrimalDualConverger
from mpisppy_amd.examples import farmer, hydro
from mpisppy_amd.extensions.extension import Extension, MultiExtension
from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater, _norm_rho_defaults
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.utils import sputils
from oracle import models as om, ph as oph

BFS = [3, 3]
HOST_LOOP = {"native_loop": 0}


# ---------------------------------------------------------------- the oracle
class NormRhoOracle(oph.OraclePH):
    """OraclePH with the reference's NormRhoUpdater.miditer restated in numpy
    and, optionally, one of the two convergers ("norm_rho", "primal_dual")."""

    def __init__(self, scens, rho=1.0, options=None, converger=None, tol=1.0, updater=True):
        super().__init__(scens, rho=rho)
        o = dict(_norm_rho_defaults)
        o.update(options or {})
        self.o = o
        self.updater = updater
        self.prev_avg = None
        self.actions = []          # per miditer with an update: {key: action}
        self.margin = np.inf       # the closest comparison of the rule, relative
        self.converger = converger
        self.tol = tol
        self.pd_prev = np.zeros((self.S, self.N))     # x-bar when the converger is built (after Iter0: zeros)
        self.trace = []            # per iteration: the converger's figures

    def _keys(self):
        """{(node, slot): the scenarios of the node, ascending}"""
        keys = {}
        for k in range(self.S):
            for j in range(self.N):
                keys.setdefault((self.node_of[k][j], j), []).append(k)
        return keys

    def _cmp(self, a, b):
        """a > b, noting how close the call is"""
        m = max(abs(a), abs(b))
        if m > 0.0:
            self.margin = min(self.margin, abs(a - b) / m)
        return a > b

    def miditer(self):
        o = self.o
        if not self.updater:
            return
        if o["rho_update_stop_iterations"] is not None and self.iter > o["rho_update_stop_iterations"]:
            return
        keys = self._keys()
        if self.prev_avg is None:
            self.prev_avg = {key: self.xbar[ks[0], key[1]] for key, ks in keys.items()}
            return
        xn = self.xn()
        acts = {}
        tol, f = o["convergence_tolerance"], o["primal_dual_difference_factor"]
        for key, ks in keys.items():
            j = key[1]
            primal = 0.0
            for k in ks:
                primal += self.scens[k].prob * abs(xn[k, j] - self.xbar[k, j])
            dual = self.rho[ks[-1], j] * math.fabs(self.xbar[ks[-1], j] - self.prev_avg[key])
            act = 0
            if self._cmp(primal, f * dual) and self._cmp(primal, tol):
                act = 1
            elif self._cmp(dual, f * primal) and self._cmp(dual, tol):
                if self.iter >= o["iterations_converged_before_decrease"]:
                    act = 2
            elif self._cmp(tol, primal) and self._cmp(tol, dual):
                act = 3
            acts[key] = act
            self.prev_avg[key] = self.xbar[ks[0], j]
            for k in ks:
                if act == 1:
                    self.rho[k, j] *= o["rho_increase_multiplier"]
                elif act == 2:
                    self.rho[k, j] /= o["rho_decrease_multiplier"]
                elif act == 3:
                    self.rho[k, j] /= o["rho_converged_decrease_multiplier"]
        self.actions.append(acts)

    def is_converged(self, convthresh):
        if self.converger == "norm_rho":
            v = math.log(sum(self.scens[k].prob * sum(self.rho[k]) for k in range(self.S)))
            self.trace.append(v)
            return v < convthresh
        if self.converger == "primal_dual":
            primal = float(np.sum(self.pc * np.abs(self.xbar - self.xn())))
            dual = float(np.sum(self.rho * np.abs(self.xbar - self.pd_prev)))
            self.pd_prev = self.xbar.copy()
            self.trace.append((primal, dual))
            return max(primal, dual) <= self.tol
        return self.conv < convthresh

    def iterk(self, max_iterations, convthresh):
        self.conv = None
        for it in range(1, max_iterations + 1):
            self.iter = it
            self.compute_xbar()
            self.update_w()
            self.conv = self.convergence_diff()
            self.history.append(self.conv)
            self.miditer()
            if self.is_converged(convthresh):
                return it
            self.solve_loop()
        return max_iterations

    def start_from(self, ph_iter0):
        """helpers.oracle_continue_from's start: the engine's Iter0 point (its
        degenerate LPs have several optimal vertices)"""
        x = ph_iter0._host("x")
        for k in range(self.S):
            self.x[k] = x[:, k].copy()
        self.W_on = self.prox_on = 1


# ---------------------------------------------------------------- the engine side
class RecordingUpdater(NormRhoUpdater):
    """NormRhoUpdater that keeps each update's actions (read after miditer)."""

    def __init__(self, ph):
        super().__init__(ph)
        self.seen = []

    def miditer(self):
        had = self._have_prev
        super().miditer()
        stop = self._stop_iter_rho_update
        if had and not (stop is not None and self.ph._PHIter > stop):
            self.seen.append(self._action.cpu().numpy().copy())


class RecordingNormRhoConverger(NormRhoConverger):
    def is_converged(self):
        r = super().is_converged()
        self.__dict__.setdefault("seen", []).append(self.conv)
        return r


class RecordingPrimalDualConverger(PrimalDualConverger):
    def is_converged(self):
        r = super().is_converged()
        self.__dict__.setdefault("seen", []).append((self.primal_gap, self.dual_gap))
        return r


CASES = {
    # model: (creator, names, creator kwargs, node names, oracle scenarios, iterations, tolerances x-bar / W / conv)
    "farmer": dict(creator=farmer.scenario_creator, names=farmer.scenario_names_creator(3), kw={"num_scens": 3},
                   nodenames=None, scens=lambda: [om.farmer("scen%d" % i, num_scens=3) for i in range(3)],
                   iters=30, tol=(1e-9, 1e-8, 1e-7), kinds={1, 2}),
    "hydro": dict(creator=hydro.scenario_creator, names=hydro.scenario_names_creator(9),
                  kw={"branching_factors": BFS}, nodenames=sputils.create_nodenames_from_branching_factors(BFS),
                  scens=lambda: [om.hydro(nm, BFS) for nm in hydro.scenario_names_creator(9)],
                  iters=20, tol=(1e-8, 1e-6, 1e-6), kinds={1, 2, 3}),
}
NRO = {"primal_dual_difference_factor": 10}


def engine(case, lib, device, iters, nro=NRO, extensions=RecordingUpdater, extension_kwargs=None, converger=None,
           options=None):
    c = CASES[case]
    opts = ph_options(iters, 1.0)
    opts.update({"iter0_solver_options": dict(HOST_LOOP), "iterk_solver_options": dict(HOST_LOOP)})
    if nro is not None:
        opts["norm_rho_options"] = dict(nro)
    opts.update(options or {})
    return PH(opts, c["names"], c["creator"], scenario_creator_kwargs=c["kw"], all_nodenames=c["nodenames"],
              extensions=extensions, extension_kwargs=extension_kwargs, ph_converger=converger,
              _native_lib=lib, _device=device)


_ITER0 = {}


def oracle(case, lib, device, iters, nro=NRO, convthresh=1e-10, **kw):
    """the oracle's run from the engine's Iter0 point (one engine Iter0 per case and library)"""
    key = (case, lib.prefix)
    if key not in _ITER0:
        ph0 = engine(case, lib, device, 0, nro=None, extensions=None)
        ph0.ph_main()
        _ITER0[key] = ph0
    o = NormRhoOracle(CASES[case]["scens"](), rho=1.0, options=nro, **kw)
    o.start_from(_ITER0[key])
    o.iterk(iters, convthresh)
    return o


def entry_actions(ph, acts):
    """the oracle's {(node, slot): action} as the engine's [NNS] vector"""
    out = np.zeros(ph.NNS, dtype=np.int32)
    names = {nd: v for v, nd in enumerate(ph._node_names)}
    stage_first = {}
    for j, (ndn, i) in enumerate(ph.slot_keys(0)):
        stage_first.setdefault(ndn.count("_"), j)
    for (ndn, j), a in acts.items():
        out[int(ph._node_off[names[ndn]]) + j - stage_first[ndn.count("_")]] = a
    return out


def check_parity(case, lib, device):
    c = CASES[case]
    ph = engine(case, lib, device, c["iters"])
    conv, Eobj, tb = ph.ph_main()
    assert all_certified(ph) and not hasattr(ph, "iterk_stats")        # the host loop ran
    o = oracle(case, lib, device, c["iters"])
    assert ph._PHIter == o.iter == c["iters"]
    # 1. a well-conditioned case: no comparison of the rule is a close call
    assert o.margin >= 1e-4, o.margin
    # 2. every action of the table occurred, in the oracle and in the engine alike
    counts = {a: sum(list(d.values()).count(a) for d in o.actions) for a in (1, 2, 3)}
    assert {a for a, n in counts.items() if n} == c["kinds"], counts
    seen = ph.extobject.seen
    assert len(seen) == len(o.actions) == c["iters"] - 1
    for got, acts in zip(seen, o.actions):
        assert np.array_equal(got, entry_actions(ph, acts))
    # 3. rho bit for bit
    assert np.array_equal(ph._host("rho").T, o.rho)
    # 4. x-bar, W, conv at the fixed-rho parity tests' tolerances
    xb = ph.xbar_by_node()
    ex = rel(xb["ROOT"][0], o.xbar[0, :len(xb["ROOT"][0])])
    if case == "hydro":
        for b in range(3):
            ex = max(ex, rel(xb["ROOT_%d" % b][0], o.xbar[3 * b, 4:]))
    ew, ec = rel(ph.W_array(), o.W), rel(conv, o.conv)
    print("[norm rho parity %s on %s] margin %.3g actions %s; engine vs oracle: x-bar %.3g W %.3g conv %.3g"
          % (case, lib.prefix, o.margin, counts, ex, ew, ec))
    assert ex < c["tol"][0] and ew < c["tol"][1] and ec < c["tol"][2], (ex, ew, ec)
    return ph, o


@pytest.mark.parametrize("case", list(CASES))
def test_parity_emu(emu, case):
    check_parity(case, emu, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_parity_gpu(gpu_lib, case):
    check_parity(case, gpu_lib, None)


# ---------------------------------------------------------------- drop-in: the reference algorithm on the views
class ViewNormRhoUpdater(Extension):
    """The reference's NormRhoUpdater (norm_rho_updater.py:50-158) ported the
    way SURVEY.md tells users to: against the per-scenario views."""

    def __init__(self, ph):
        super().__init__(ph)
        self.ph = ph
        o = dict(_norm_rho_defaults)
        o.update(ph.options.get("norm_rho_options", {}))
        self.o = o
        self._prev_avg = {}

    def _snapshot_avg(self, ph):
        for s in ph.local_scenarios.values():
            for ndn_i in s._mpisppy_model.xbars.keys():
                self._prev_avg[ndn_i] = s._mpisppy_model.xbars[ndn_i].value

    def miditer(self):
        ph, o = self.ph, self.o
        ph_iter = ph._PHIter
        if o["rho_update_stop_iterations"] is not None and ph_iter > o["rho_update_stop_iterations"]:
            return
        if not self._prev_avg:
            self._snapshot_avg(ph)
            return
        primal, dual = {}, {}
        for s in ph.local_scenarios.values():
            for ndn_i, v in s._mpisppy_data.nonant_indices.items():
                primal[ndn_i] = primal.get(ndn_i, 0.0) + s._mpisppy_probability * abs(
                    v.value - s._mpisppy_model.xbars[ndn_i].value)
        for s in ph.local_scenarios.values():
            for ndn_i in s._mpisppy_data.nonant_indices:
                dual[ndn_i] = s._mpisppy_model.rho[ndn_i].value * math.fabs(
                    s._mpisppy_model.xbars[ndn_i].value - self._prev_avg[ndn_i])
        self._snapshot_avg(ph)
        f, tol = o["primal_dual_difference_factor"], o["convergence_tolerance"]
        for s in ph.local_scenarios.values():
            for ndn_i in s._mpisppy_model.rho.keys():
                rho = s._mpisppy_model.rho[ndn_i]
                p, d = primal[ndn_i], dual[ndn_i]
                if (p > f * d) and (p > tol):
                    rho.value = rho.value * o["rho_increase_multiplier"]
                elif (d > f * p) and (d > tol):
                    if ph_iter >= o["iterations_converged_before_decrease"]:
                        rho.value = rho.value / o["rho_decrease_multiplier"]
                elif (p < tol) and (d < tol):
                    rho.value = rho.value / o["rho_converged_decrease_multiplier"]


def test_view_port_gives_the_same_rho_emu(emu):
    a = engine("farmer", emu, "cpu", 12)
    a.ph_main()
    b = engine("farmer", emu, "cpu", 12, extensions=ViewNormRhoUpdater)
    b.ph_main()
    assert any(v.any() for v in a.extobject.seen)
    assert np.array_equal(a._host("rho"), b._host("rho"))
    assert np.array_equal(a._host("W"), b._host("W"))


# ---------------------------------------------------------------- options
def test_defaults_are_the_reference_s(emu):
    ph = engine("farmer", emu, "cpu", 1, nro=None, extensions=NormRhoUpdater)
    e = ph.extobject
    assert ph._mpisppy_norm_rho_update_inuse is True
    assert (e._tol, e._rho_decrease, e._rho_increase, e._primal_dual_difference_factor,
            e._required_converged_before_decrease, e._rho_converged_residual_decrease, e._stop_iter_rho_update,
            e._verbose) == (1e-4, 2.0, 2.0, 100., 0, 1.1, None, False)
    ph = engine("farmer", emu, "cpu", 1, nro={"rho_increase_multiplier": 3.0, "verbose": True},
                extensions=NormRhoUpdater)
    assert ph.extobject._rho_increase == 3.0 and ph.extobject._verbose and ph.extobject._rho_decrease == 2.0


def test_stop_iterations_freezes_rho_emu(emu):
    nro = dict(NRO, rho_update_stop_iterations=6)
    a = engine("farmer", emu, "cpu", 14, nro=nro)
    a.ph_main()
    assert len(a.extobject.seen) == 5                       # iterations 2..6
    b = engine("farmer", emu, "cpu", 6)
    b.ph_main()
    assert any(v.any() for v in b.extobject.seen)
    assert np.array_equal(a._host("rho"), b._host("rho"))
    o = oracle("farmer", emu, "cpu", 14, nro=nro)
    assert np.array_equal(a._host("rho").T, o.rho)


def test_decreases_wait_for_the_iteration_count_emu(emu):
    base = engine("farmer", emu, "cpu", 30)
    base.ph_main()
    assert any((v == 2).any() for v in base.extobject.seen)
    nro = dict(NRO, iterations_converged_before_decrease=1000)
    a = engine("farmer", emu, "cpu", 30, nro=nro)
    a.ph_main()
    assert not any((v == 2).any() for v in a.extobject.seen) and any((v == 1).any() for v in a.extobject.seen)
    o = oracle("farmer", emu, "cpu", 30, nro=nro)
    assert np.array_equal(a._host("rho").T, o.rho)
    assert a._host("rho").min() >= 1.0


def test_multi_extension_emu(emu):
    a = engine("farmer", emu, "cpu", 12)
    a.ph_main()
    b = engine("farmer", emu, "cpu", 12, extensions=MultiExtension,
               extension_kwargs={"ext_classes": [NormRhoUpdater]})
    b.ph_main()
    assert np.array_equal(a._host("rho"), b._host("rho")) and np.array_equal(a._host("W"), b._host("W"))


def test_verbose_prints_the_table_emu(emu, capsys):
    ph = engine("farmer", emu, "cpu", 4, nro=dict(NRO, verbose=True), extensions=NormRhoUpdater)
    ph.ph_main()
    out = capsys.readouterr().out
    assert "Updating rho values:" in out and "Primal Residual" in out
    assert any(a in out for a in ("Increasing", "Decreasing"))
    assert "DevotedAcreage" in out


def test_miditer_reads_nothing_back_emu(emu, monkeypatch):
    """One rank, not verbose: miditer enqueues its kernels and returns -- no
    device-to-host read, no host synchronisation."""
    ph = engine("farmer", emu, "cpu", 3, extensions=NormRhoUpdater)
    ph.ph_main()
    ph._PHIter += 1
    ph.Compute_Xbar(False)
    ph.Update_W(False)
    ph.convergence_diff()
    rho0 = ph._host("rho").copy()
    ph.extobject._prev_avg.zero_()      # (a dual residual that forces an action whatever the state)

    def boom(*a, **k):
        raise AssertionError("miditer read device state back")
    with monkeypatch.context() as m:
        m.setattr(ph, "_host", boom)
        m.setattr(ph, "_read_small", boom)
        m.setattr(torch.Tensor, "cpu", boom)
        m.setattr(torch.Tensor, "item", boom)
        ph.extobject.miditer()
    assert ph.extobject._action.cpu().numpy().any()
    assert not np.array_equal(ph._host("rho"), rho0)


# ---------------------------------------------------------------- convergers
def test_norm_rho_converger_needs_the_updater_emu(emu):
    ph = engine("farmer", emu, "cpu", 3, nro=None, extensions=None, converger=NormRhoConverger)
    with pytest.raises(RuntimeError, match="NormRhoConverger can only be used if NormRhoUpdater is"):
        ph.ph_main()


def check_norm_rho_converger(case, lib, device):
    iters = 12
    ph = engine(case, lib, device, iters, converger=RecordingNormRhoConverger, options={"convthresh": -100.0})
    ph.ph_main()
    o = oracle(case, lib, device, iters, converger="norm_rho", convthresh=-100.0)
    got = ph.convobject.seen
    assert len(got) == len(o.trace) == iters
    assert len(set(o.trace)) > 1                         # rho moved
    for a, b in zip(got, o.trace):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)
    # and it stops, at the first iteration whose log(sum p rho) is below the
    # threshold: one past the start that undercuts every earlier value by a
    # clear gap (hydro's rho shrinks; farmer's does not within these iterations)
    k = next((i for i in range(3, iters) if o.trace[i] < min(o.trace[:i]) - 1e-3), None)
    assert k is not None or case == "farmer"
    if k is not None:
        thr = 0.5 * (o.trace[k] + min(o.trace[:k]))
        ph = engine(case, lib, device, iters, converger=NormRhoConverger, options={"convthresh": thr})
        ph.ph_main()
        assert ph._PHIter == k + 1


@pytest.mark.parametrize("case", list(CASES))
def test_norm_rho_converger_emu(emu, case):
    check_norm_rho_converger(case, emu, "cpu")


@pytest.mark.gpu
def test_norm_rho_converger_gpu(gpu_lib):
    check_norm_rho_converger("hydro", gpu_lib, None)


def check_primal_dual_converger(case, lib, device):
    c = CASES[case]
    iters = 15
    pdo = {"primal_dual_converger_options": {"tol": 0.0}}
    ph = engine(case, lib, device, iters, converger=RecordingPrimalDualConverger, options=pdo)
    ph.ph_main()
    o = oracle(case, lib, device, iters, converger="primal_dual", tol=0.0)
    got = ph.convobject.seen
    assert len(got) == len(o.trace) == iters
    worst = max(max(rel(a[0], b[0]), rel(a[1], b[1])) for a, b in zip(got, o.trace))
    print("[primal-dual converger %s on %s] gaps, engine vs oracle: %.3g" % (case, lib.prefix, worst))
    assert worst < c["tol"][0], worst
    # a threshold the oracle's run crosses with 10 % to spare on both sides
    m = [max(t) for t in o.trace]
    k = next(i for i in range(2, iters) if m[i] * 1.21 <= min(m[:i]))
    tol = math.sqrt(m[k] * min(m[:k]))
    assert m[k] <= tol / 1.1 and min(m[:k]) >= 1.1 * tol
    ph = engine(case, lib, device, iters, converger=PrimalDualConverger,
                options={"primal_dual_converger_options": {"tol": tol}})
    ph.ph_main()
    assert ph._PHIter == k + 1


@pytest.mark.parametrize("case", list(CASES))
def test_primal_dual_converger_emu(emu, case):
    check_primal_dual_converger(case, emu, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_primal_dual_converger_gpu(gpu_lib, case):
    check_primal_dual_converger(case, gpu_lib, None)


def test_primal_dual_converger_options_emu(emu):
    ph = engine("farmer", emu, "cpu", 1, nro=None, extensions=None)
    c = PrimalDualConverger(ph)
    assert c.convergence_threshold == 1 and c._verbose is False
    ph.options["primal_dual_converger_options"] = {"tracking": True}
    with pytest.raises(NotImplementedError):
        PrimalDualConverger(ph)
