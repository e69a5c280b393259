"""NormRhoUpdater's update inside the device loop (phx_iterk_norm_rho): the
checks shared by test_iterk_rho.py (host emulation), test_iterk_rho_gpu.py and
test_iterk_rho_distributed.py.

The device loop (``native_loop`` 1, a plain ``NormRhoUpdater`` with
``log_actions``) is compared with the host loop (``native_loop`` 0,
``test_norm_rho.RecordingUpdater``) under the same options.  The unfused device
loop equals the host loop bit for bit at a fixed rho
(test_engine_emu.check_native_vs_host, fused=0), the residuals come from the
same pass as phx_node_absdev's and the rule's arithmetic is phx_norm_rho's, so
everything compared here must be EQUAL: _PHIter, rho, W, the nonant values,
x-bar, conv, Eobjective, the trivial bound, every iteration's actions and the
updater's own state (snapshot, last residuals, last actions, have_prev).
"""
import math

import numpy as np

from helpers import all_certified, ph_options, rel
from mpisppy_amd.examples import farmer
from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater
from mpisppy_amd.opt.ph import PH
from test_norm_rho import CASES, NRO, RecordingUpdater, entry_actions, oracle

DEVICE_LOOP = {"native_loop": 1}
HOST_LOOP = {"native_loop": 0}


class ConvRecordingUpdater(RecordingUpdater):
    """RecordingUpdater that also keeps convergence_diff of every iteration (miditer runs right after it)."""

    def __init__(self, ph):
        super().__init__(ph)
        self.convs = []

    def miditer(self):
        self.convs.append(float(self.ph.conv))
        super().miditer()


def make(lib, device, creator, names, kw, iters, native, nro=NRO, nodenames=None, solver=None, iterk_extra=None,
         options=None, extensions=None, mpicomm=None):
    """One engine with the updater; native: the device loop (a plain NormRhoUpdater
    that logs its actions) or the host loop (RecordingUpdater)."""
    opts = ph_options(iters, 1.0)
    so = dict(solver or {}, native_loop=1 if native else 0, **(iterk_extra or {}))
    opts.update({"iter0_solver_options": dict(solver or {}), "iterk_solver_options": so,
                 "norm_rho_options": dict(nro)})
    opts.update(options or {})
    if extensions is None:
        extensions = NormRhoUpdater if native else RecordingUpdater
    ph = PH(opts, names, creator, scenario_creator_kwargs=kw, all_nodenames=nodenames, extensions=extensions,
            mpicomm=mpicomm, _native_lib=lib, _device=device)
    if native:
        ph.extobject.log_actions = True
    return ph


def farmer_pair(lib, device, S, iters, kw=None, **more):
    """(device loop, host loop) runs of farmer with S scenarios: [(ph, conv, Eobj, trivial bound)] * 2"""
    runs = []
    for native in (True, False):
        ph = make(lib, device, farmer.scenario_creator, farmer.scenario_names_creator(S),
                  dict({"num_scens": S}, **(kw or {})), iters, native, **more)
        runs.append((ph,) + tuple(ph.ph_main()))
    return runs


def update_rows(ph, n_updates):
    """The action log's rows of the iterations that updated (2, 3, ...: iteration
    1 only takes the snapshot); every other row must have stayed zero."""
    log = ph.extobject.action_log.cpu().numpy()
    assert log.shape == (max(int(ph.options["PHIterLimit"]), 1), max(ph.NNS, 1))
    rows = log[1:1 + n_updates]
    rest = np.concatenate([log[:1], log[1 + n_updates:]])
    assert not rest.any()
    return rows


def assert_equal_runs(runs):
    """The comparison rule: the device loop's run equals the host loop's, bit for bit."""
    (a, ca, Ea, ta), (b, cb, Eb, tb) = runs
    assert hasattr(a, "iterk_stats") and not hasattr(b, "iterk_stats")
    assert a.iterk_stats["fused"] is False
    assert all_certified(a) and all_certified(b)
    assert a._PHIter == b._PHIter
    assert np.array_equal(a._host("rho"), b._host("rho"))
    assert np.array_equal(a.W_array(), b.W_array())
    assert np.array_equal(a.nonant_values(), b.nonant_values())
    for k, v in b.xbar_by_node().items():
        assert np.array_equal(a.xbar_by_node()[k][0], v[0]), k
    assert ca == cb and Ea == Eb and ta == tb, ((ca, cb), (Ea, Eb), (ta, tb))
    seen = b.extobject.seen
    assert a.iterk_stats["rho_updates"] == len(seen)
    if seen:
        assert np.array_equal(update_rows(a, len(seen)), np.array(seen))
    else:
        update_rows(a, 0)
    # the updater is left as the host loop's miditer leaves it
    ea, eb = a.extobject, b.extobject
    assert ea._have_prev == eb._have_prev
    for name in ("_prev_avg", "_action", "_dual", "_primal"):
        assert np.array_equal(getattr(ea, name).cpu().numpy(), getattr(eb, name).cpu().numpy()), name
    return a, b


# ---------------------------------------------------------------- 1. oracle parity through the device loop
def check_oracle_parity(case, lib, device):
    """test_norm_rho.check_parity's four assertions with the device loop in the engine's place."""
    c = CASES[case]
    ph = make(lib, device, c["creator"], c["names"], c["kw"], c["iters"], True, nodenames=c["nodenames"])
    conv, Eobj, tb = ph.ph_main()
    assert all_certified(ph) and hasattr(ph, "iterk_stats") and ph.iterk_stats["fused"] is False
    o = oracle(case, lib, device, c["iters"])
    assert ph._PHIter == o.iter == c["iters"]
    assert o.margin >= 1e-4, o.margin
    counts = {a: sum(list(d.values()).count(a) for d in o.actions) for a in (1, 2, 3)}
    assert {a for a, n in counts.items() if n} == c["kinds"], counts
    assert ph.iterk_stats["rho_updates"] == len(o.actions) == c["iters"] - 1
    for got, acts in zip(update_rows(ph, len(o.actions)), o.actions):
        assert np.array_equal(got, entry_actions(ph, acts))
    assert np.array_equal(ph._host("rho").T, o.rho)
    xb = ph.xbar_by_node()
    ex = rel(xb["ROOT"][0], o.xbar[0, :len(xb["ROOT"][0])])
    if case == "hydro":
        for b in range(3):
            ex = max(ex, rel(xb["ROOT_%d" % b][0], o.xbar[3 * b, 4:]))
    ew, ec = rel(ph.W_array(), o.W), rel(conv, o.conv)
    print("[iterk norm rho parity %s on %s] margin %.3g actions %s; device loop vs oracle: x-bar %.3g W %.3g "
          "conv %.3g" % (case, lib.prefix, o.margin, counts, ex, ew, ec))
    assert ex < c["tol"][0] and ew < c["tol"][1] and ec < c["tol"][2], (ex, ew, ec)
    # and the host loop, bit for bit (hydro: NNS > N, node-indexed x-bar)
    hb = make(lib, device, c["creator"], c["names"], c["kw"], c["iters"], False, nodenames=c["nodenames"])
    assert_equal_runs([(ph, conv, Eobj, tb), (hb,) + tuple(hb.ph_main())])
    return ph


# ---------------------------------------------------------------- 2. kernel size edges
SIZE_EDGES = [1100, 8500]      # the tiled k_absdev with the rule in its last block; above 32 tiles: the block-reduction fold


def check_size_edge(lib, device, S):
    a, b = assert_equal_runs(farmer_pair(lib, device, S, 8))
    assert not np.all(a._host("rho") == 1.0)
    return a, b


# ---------------------------------------------------------------- 3. stop by convthresh
def conv_stop_threshold(convs, seen, k_min=5):
    """(k*, threshold): the first iteration k* >= k_min whose conv is a new running
    minimum and whose own update changes rho (seen[k* - 2]: the updates start at
    iteration 2), so that a loop which skipped the update of the iteration that
    converges would leave another rho; the threshold is the geometric mean of that
    conv and the previous running minimum, with a relative gap of at least 1e-3
    on both sides."""
    for k in range(max(k_min, 2), len(convs) + 1):
        prev = min(convs[:k - 1])
        if convs[k - 1] < prev and seen[k - 2].any():
            thr = math.sqrt(convs[k - 1] * prev)
            assert (thr - convs[k - 1]) / thr >= 1e-3 and (prev - thr) / prev >= 1e-3, (convs[k - 1], thr, prev)
            return k, thr
    raise AssertionError("no new running minimum from iteration %d on" % k_min)


def check_convthresh_stop(lib, device, S=30, iters=30):
    """Both loops leave at k* with `converged`, and rho carries the update of
    iteration k* itself (miditer runs before the stop test)."""
    h = make(lib, device, farmer.scenario_creator, farmer.scenario_names_creator(S), {"num_scens": S}, iters, False,
             extensions=ConvRecordingUpdater)
    h.ph_main()
    kstar, thr = conv_stop_threshold(h.extobject.convs, h.extobject.seen)
    a, b = assert_equal_runs(farmer_pair(lib, device, S, iters, options={"convthresh": thr}))
    assert a._PHIter == b._PHIter == kstar < iters
    assert a.iterk_stats["converged"] and a.iterk_stats["iters"] == kstar
    assert a.iterk_stats["rho_updates"] == kstar - 1          # iterations 2 .. k*, the last one included
    # the update of iteration k* moved rho: the run stopped one iteration earlier has another rho
    assert update_rows(a, kstar - 1)[-1].any()
    return a, b, kstar


# ---------------------------------------------------------------- 4. straggler stops
STRAGGLERS = [{"as_rounds": 1, "ipm_max_it": 3, "rescue_rounds": 1}, {"as_rounds": 0, "ipm_max_it": 2}]


def check_straggler_stops(lib, device, so, S=2000, iters=5):
    a, b = assert_equal_runs(farmer_pair(lib, device, S, iters, solver=so, iterk_extra={"iterk_fused": 0}))
    assert not np.all(a._host("rho") == 1.0)
    return a, b


def check_straggler_stops_wg(lib, device, S, iterk_extra=None):
    """check_native_vs_host_wg's model: above the lane limits, the workgroup tier
    derives its PH terms from rho (k_ph_terms) after every update."""
    a, b = assert_equal_runs(farmer_pair(lib, device, S, 5, kw={"crops_multiplier": 10}, solver={"wg_warm": 1},
                                         iterk_extra=iterk_extra))
    assert not a._native.jit_info(a._ctx).decode().startswith("on")
    assert not np.all(a._host("rho") == 1.0)
    return a, b


# ---------------------------------------------------------------- 5. options
def check_option(lib, device, nro_extra):
    a, b = assert_equal_runs(farmer_pair(lib, device, 3, 12, nro=dict(NRO, **nro_extra)))
    return a, b


def check_keeps_host_loop(lib, device):
    """verbose, and a subclass that overrides miditer, keep the host loop"""
    for kw in (dict(nro=dict(NRO, verbose=True)), dict(extensions=RecordingUpdater)):
        ph = make(lib, device, farmer.scenario_creator, farmer.scenario_names_creator(3), {"num_scens": 3}, 4,
                  True, **kw)
        ph.ph_main()
        assert not hasattr(ph, "iterk_stats")
        assert ph.extobject.action_log is None


def check_iteration_limits(lib, device):
    """PHIterLimit 0 and 1 run; have_prev is 0 / 1 afterwards and no update was applied"""
    for iters in (0, 1):
        a, b = assert_equal_runs(farmer_pair(lib, device, 3, iters))
        assert a.extobject._have_prev == bool(iters)
        assert a.iterk_stats["rho_updates"] == 0 and np.all(a._host("rho") == 1.0)
