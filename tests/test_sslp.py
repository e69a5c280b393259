"""sslp LP relaxation (workload C5a): the restated scenario creator
(batch == per-scenario models, bit-exact), and PH through the engine (generic
PDHG + polish path: n = 705 is above the lane-solver limits) against the oracle on
the shipped sslp_15_45_5 instance.  The reference ships no sslp golden values
(no sslp test in mpisppy/tests): parity here is engine vs the oracle restatement,
whose PH loop is pinned by the farmer/aircond goldens (test_oracle_golden.py)."""
import numpy as np
import pytest

from helpers import all_certified, kkt_recheck, rel, run_engine
from mpisppy_amd.batch import from_models
from mpisppy_amd.examples import sslp
from oracle import models as om, ph as oph


def test_sslp_batch_equals_models():
    names = sslp.scenario_names_creator(8)          # Scenario1..5 shipped, 6..8 synthetic
    a = from_models(names, [sslp.scenario_creator(nm, instance=5) for nm in names]).compress()
    b = sslp.batch_creator(names, instance=5).compress()
    for k in ["rowptr", "colidx", "kvar", "Aconst", "Avar", "c", "lb", "ub", "bl", "bu"]:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.n, a.m, a.nnz) == (705, 60, b.nnz)
    assert list(a.nonant.slot_col) == list(range(15)) and a.rhs_vary and not a.c_vary
    # the shipped instance data, and the synthetic Bernoulli(0.5) rate
    d = sslp.data()
    assert np.array_equal(a.bl[:, 15:][0], d["ClientPresent"]["5"][0])
    P = np.stack([sslp.client_present(k) for k in range(100, 400)])
    assert 0.45 < P.mean() < 0.55


def test_sslp_oracle_model_matches_creator():
    for nm in ["Scenario2", "Scenario9"]:
        m = sslp.scenario_creator(nm, data_dir="x/sslp_15_45_5/scenariodata")
        sf = m.standard_form()
        o = om.sslp(nm, instance=5)
        A = np.zeros((len(sf["bl"]), len(sf["c"])))
        for i in range(len(sf["bl"])):
            for k in range(sf["rowptr"][i], sf["rowptr"][i + 1]):
                A[i, sf["colidx"][k]] = sf["vals"][k]
        assert np.array_equal(A, o.A) and np.array_equal(sf["c"], o.c)
        assert np.array_equal(sf["bl"], o.bl) and np.array_equal(sf["bu"], o.bu)
        assert np.array_equal(sf["lb"], o.lb) and np.array_equal(sf["ub"], o.ub)


def check_sslp_ph(lib, device, iters=3):
    """Iter0 LPs are degenerate (several optimal vertices), so engine
    and oracle may take different PH trajectories.  Checked instead: the trivial
    bound (the LP optimum value is unique), and every subproblem of the last
    iteration re-solved by the oracle from the engine's own W / x-bar / rho: the
    nonant optimum is unique there (strictly convex prox) and must agree to 1e-6,
    the objective to 1e-8 (north_star bar)."""
    names = sslp.scenario_names_creator(5)
    ph, conv, Eobj, tb = run_engine(sslp.scenario_creator, names, {"instance": 5}, iters, lib=lib, device=device,
                                    options={"per_scenario_models": True})
    o = oph.OraclePH([om.sslp(nm, instance=5) for nm in names], rho=1.0)
    otb = o.iter0()
    assert rel(tb, otb) < 1e-8
    assert all_certified(ph)
    o.W = ph.W_array().copy()
    xb = ph.xbar_by_node()["ROOT"][0]
    o.xbar = np.tile(xb, (len(names), 1))
    o.W_on, o.prox_on = 1, 1
    o.solve_loop()
    assert rel(ph.nonant_values(), o.xn()) < 1e-6
    eng_obj = ph._host("obj")
    assert rel(eng_obj, o.obj) < 1e-8
    kkt_recheck(ph, tag="sslp")
    return ph, o


def test_sslp_ph_emu(emu):
    check_sslp_ph(emu, "cpu", iters=2)


def check_sslp_10k(lib, device, S, iters, pick):
    """BASELINE configs[4] C5a: S stochastic-RHS scenarios (synthetic
    Bernoulli(0.5) client presence, p = 1/S), `iters` PH iterations: every
    subproblem of every solve certified; the sampled scenarios' Iter0 optima
    (unique LP values) and their last-iteration subproblems re-solved by the oracle
    from the engine's own W / x-bar agree to 1e-8 / 1e-6 (nonants) / 1e-8 (obj)."""
    names = sslp.scenario_names_creator(S)
    ph, conv, Eobj, tb = run_engine(sslp.scenario_creator, names, {"num_scens": S}, iters, lib=lib, device=device)
    assert all_certified(ph), [s["not_optimal"] for s in ph.solve_stats]
    o = oph.OraclePH([om.sslp(names[k], num_scens=S) for k in pick], rho=1.0)
    o.iter0()
    assert rel(ph._iter0_obj[pick], o.obj) < 1e-8
    o.W = ph.W_array()[pick].copy()
    o.xbar = np.tile(ph.xbar_by_node()["ROOT"][0], (len(pick), 1))
    o.W_on, o.prox_on = 1, 1
    o.solve_loop()
    assert rel(ph.nonant_values()[pick], o.xn()) < 1e-6
    assert rel(ph._host("obj")[pick], o.obj) < 1e-8
    return ph


def test_sslp_synthetic_emu(emu):
    check_sslp_10k(emu, "cpu", 64, 3, [0, 5, 31, 63])


@pytest.mark.gpu
def test_sslp_10k_gpu(gpu_lib):
    ph = check_sslp_10k(gpu_lib, None, 10000, 3, [0, 1, 2, 4999, 5000, 9998, 9999])
    print({k: [s.get(k) for s in ph.solve_stats] for k in ["sp_certified", "wg_certified", "sp_ms", "wg_ms"]})
