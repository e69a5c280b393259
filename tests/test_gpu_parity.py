"""GPU parity: the real libphx kernels against the CPU oracle and the reference goldens.

Tolerance (north_star): xbar, W and the PH objective within 1e-6 relative;
every subproblem optimum polished to a KKT certificate of 1e-9.
"""
import json
import os

import numpy as np
import pytest

from helpers import (all_certified, kkt_recheck, oracle_continue_from, ph_options, REF_W, REF_XBAR, rel,
                     run_engine)
from mpisppy_amd.examples import farmer, aircond
from mpisppy_amd.opt.ph import PH
from oracle import models as om, ph as oph

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_goldens.json")))

pytestmark = pytest.mark.gpu


def test_farmer3_golden(gpu_lib):
    ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(3),
                                    {"num_scens": 3}, 5, lib=gpu_lib)
    xbar = ph.xbar_by_node()["ROOT"][0]
    assert rel(xbar, REF_XBAR) < 1e-7
    assert np.max(np.abs(ph.W_array() - REF_W)) < 5e-6        # reference asserts places=5
    o = oph.OraclePH([om.farmer("scen%d" % i, num_scens=3) for i in range(3)], rho=1.0)
    oc, oE, otb = o.ph_main(5)
    assert rel(xbar, o.xbar[0]) < 1e-9
    assert rel(ph.W_array(), o.W) < 1e-8
    assert rel(Eobj, oE) < 1e-9 and rel(tb, otb) < 1e-9 and rel(conv, oc) < 1e-7


@pytest.mark.parametrize("S", [30, 300])
def test_farmer_many_vs_oracle(gpu_lib, S):
    ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S),
                                    {"num_scens": S}, 3, lib=gpu_lib)
    o = oph.OraclePH([om.farmer("scen%d" % i, num_scens=S) for i in range(S)], rho=1.0)
    oc, oE, otb = o.ph_main(3)
    assert rel(tb, otb) < 1e-9
    assert rel(ph.xbar_by_node()["ROOT"][0], o.xbar[0]) < 1e-8
    assert rel(ph.W_array(), o.W) < 1e-7
    assert rel(Eobj, oE) < 1e-8
    assert all_certified(ph)
    kkt_recheck(ph, tag="farmer S=%d, fused loop" % S)


def test_aircond_multistage_vs_oracle(gpu_lib):
    bfs = [3, 3, 2]
    from mpisppy_amd.utils import sputils
    names = ["scen%d" % i for i in range(18)]
    ph, conv, Eobj, tb = run_engine(aircond.scenario_creator, names, {"branching_factors": bfs, "start_seed": 0},
                                    4, lib=gpu_lib,
                                    all_nodenames=sputils.create_nodenames_from_branching_factors(bfs))
    scens = [om.aircond(n, bfs, start_seed=0) for n in names]
    o = oph.OraclePH(scens, rho=1.0)
    oc, oE, otb = o.ph_main(4)
    assert rel(tb, otb) < 1e-9
    assert rel(Eobj, oE) < 1e-8
    assert rel(ph.W_array(), o.W) < 1e-7
    kkt_recheck(ph, tag="aircond 3x3x2")


def test_lane_and_generic_paths_agree(gpu_lib):
    """The structure-specialised lane solver (warm active set + IPM) and the
    generic PDHG + polish path give the same PH trajectory."""
    S = 200
    res = []
    for so in ({"lane_solver": 1}, {"lane_solver": 0}, {"lane_solver": 1, "as_rounds": 0}):
        ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S),
                                        {"num_scens": S}, 4, lib=gpu_lib,
                                        options={"iter0_solver_options": so, "iterk_solver_options": so})
        assert all_certified(ph)
        res.append((ph.W_array(), ph.xbar_by_node()["ROOT"][0], Eobj, tb))
    for W, xb, E, t in res[1:]:
        assert rel(W, res[0][0]) < 1e-8
        assert rel(xb, res[0][1]) < 1e-9
        assert rel(E, res[0][2]) < 1e-9 and rel(t, res[0][3]) < 1e-9


def test_farmer_100k_sampled_oracle(gpu_lib):
    """Full-size run (BASELINE configs[2]: farmer, 100,000 scenarios): every
    subproblem certified; a sample of scenarios re-solved by the CPU oracle
    from the engine's own W / xbar agrees to 1e-6 relative (north_star bar)."""
    S = 100000
    ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S),
                                    {"num_scens": S}, 3, lib=gpu_lib)
    assert all_certified(ph)
    W = ph.W_array()
    xb = ph.xbar_by_node()["ROOT"][0]
    xn = ph.nonant_values()
    obj = ph._host("obj")
    rng = np.random.RandomState(7)
    sample = sorted(set(rng.randint(0, S, 48).tolist()) | {0, 1, 2, S - 1})
    # W/xbar are those of the last update; the last solve used W, xbar after
    # iteration 3's update, which are exactly the current values
    scens = [om.farmer("scen%d" % k, num_scens=S) for k in sample]
    o = oph.OraclePH(scens, rho=1.0)
    o.W_on = o.prox_on = 1
    o.W[:] = W[sample]
    o.xbar[:] = xb[None, :]
    o.solve_loop()
    assert rel(o.xn(), xn[sample]) < 1e-6
    assert rel(o.obj, obj[sample]) < 1e-8
    assert 0.0 < conv < 1e4 and np.isfinite(Eobj) and np.isfinite(tb)


@pytest.mark.parametrize("fused", [0, 1])
def test_farmer_100k_reductions_recheck(gpu_lib, fused):
    """Full size (100,000 scenarios: 391 x-bar tiles, 8 arrival shards): after each of
    3 PH iterations, x-bar / x-sq-bar / W / conv equal a host recomputation from the
    engine's own x (math.fsum) to 1e-12 -- unfused (k_xbar + k_update_w_seg) and fused
    (the warm kernel's x-bar partials and last-block fold from iteration 2 on)."""
    from test_engine_emu import check_reductions_by_iteration
    runs = check_reductions_by_iteration(gpu_lib, None, 100000, fused)
    assert all(bool(r["fused"]) == bool(fused) for r in runs[1:])


def test_uncertified_counts_infeasible_gpu(gpu_lib):
    from test_xhat_emu import check_uncertified_counts_infeasible
    check_uncertified_counts_infeasible(gpu_lib, None)


def test_deferred_solve_with_stragglers_matches_sync(gpu_lib):
    """Deferred solve + optimistic Compute_Xbar/Update_W; stragglers forced by
    starving the interior point: the redo path must reproduce the synchronous run."""
    S = 300
    so = {"as_rounds": 0, "ipm_max_it": 2}
    runs = []
    for defer in (1, 0):
        o = dict(so, defer=defer, native_loop=0)
        ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S),
                                        {"num_scens": S}, 4, lib=gpu_lib,
                                        options={"iter0_solver_options": o, "iterk_solver_options": o})
        assert all_certified(ph)
        runs.append((ph, conv, Eobj, tb))
    (a, ca, Ea, ta), (b, cb, Eb, tb_) = runs
    assert any(s.get("stragglers", 0) > 0 for s in a.solve_stats)
    assert rel(a.W_array(), b.W_array()) < 1e-12
    assert rel(ca, cb) < 1e-12 and rel(Ea, Eb) < 1e-12 and rel(ta, tb_) < 1e-12


def test_xhat_eval_farmer_gpu(gpu_lib):
    """Xhat_Eval over farmer 100 names / num_scens 10 (test_conf_int_farmer.py:168-202)."""
    from test_xhat_emu import check_farmer_xhat
    check_farmer_xhat(gpu_lib, None)


def test_xhat_eval_aircond_gpu(gpu_lib):
    from test_xhat_emu import check_aircond_xhat
    check_aircond_xhat(gpu_lib, None)


def test_infeasible_xhat_gpu(gpu_lib):
    """An xhat over the 500-acre limit on 2,000 scenarios: every subproblem ends
    INFEASIBLE with a Farkas certificate and infeas_prob() == 1; a feasible xhat
    afterwards evaluates normally."""
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    from test_xhat_emu import xhat_options
    S = 2000
    ev = Xhat_Eval(xhat_options(), farmer.scenario_names_creator(S), farmer.scenario_creator,
                   scenario_creator_kwargs={"num_scens": S}, _native_lib=gpu_lib)
    ev.solve_loop()
    ev.evaluate({"ROOT": [300.0, 300.0, 300.0]})
    assert ev.infeas_prob() == pytest.approx(1.0)
    assert ev.solve_stats[-1]["infeasible"] == S, ev.solve_stats[-1]
    ev.evaluate({"ROOT": [80.0, 250.0, 170.0]})
    assert ev.infeas_prob() == 0.0


def test_fixed_nonants_large_batch_gpu(gpu_lib):
    """Fixing over 20k scenarios (generic path with per-scenario bounds), sampled
    against the oracle; then unfixing returns to the lane path's solution."""
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    from test_xhat_emu import xhat_options
    S = 20000
    ev = Xhat_Eval(xhat_options(), farmer.scenario_names_creator(S), farmer.scenario_creator,
                   scenario_creator_kwargs={"num_scens": S}, _native_lib=gpu_lib)
    ev.solve_loop()
    base = ev.nonant_values().copy()
    xhat = {"ROOT": [80.0, 250.0, 170.0]}
    E = ev.evaluate(xhat)
    assert ev.infeas_prob() == 0.0
    idx = np.r_[0:5, S - 5:S, np.random.RandomState(0).choice(S, 20, replace=False)]
    _, objs, _ = oph.evaluate_xhat([om.farmer("scen%d" % i, num_scens=S) for i in idx], xhat)
    got = np.array([ev.objs_dict["scen%d" % i] for i in idx])
    assert rel(got, objs) < 1e-9
    ev._unfix_nonants()
    ev.solve_loop()
    assert rel(ev.nonant_values(), base) < 1e-9


@pytest.mark.parametrize("case", ["farmer", "aircond", "conv_ranks", "converge"])
def test_native_loop_matches_host_loop_gpu(gpu_lib, case):
    """phx_iterk (device-side stop flag, pipelined) == the Python loop, bit for bit."""
    from test_engine_emu import check_native_vs_host
    check_native_vs_host(gpu_lib, None, case, S=1000)


@pytest.mark.parametrize("case", ["farmer", "aircond", "conv_ranks", "converge"])
def test_native_loop_fused_matches_host_loop_gpu(gpu_lib, case):
    """phx_iterk fused mode (one phx_lane_warm launch per PH iteration: Update_W,
    conv partials, solve, next x-bar partials) == the Python loop to 1e-9, same
    iteration count; multistage / emulated-rank cases fall back (bit for bit)."""
    from test_engine_emu import check_native_vs_host
    check_native_vs_host(gpu_lib, None, case, S=1000, fused=1)


@pytest.mark.parametrize("so,fused", [({"as_rounds": 0, "ipm_max_it": 2}, 0), ({"as_rounds": 1, "ipm_max_it": 3, "rescue_rounds": 1}, 0),
                                      ({"as_rounds": 1, "ipm_max_it": 3, "rescue_rounds": 1}, 1)])
def test_native_loop_straggler_stops_gpu(gpu_lib, so, fused):
    """Starved lane solves leave lanes to the generic path: phx_iterk stops the
    pipeline, finishes them and resumes; the trajectory equals the host loop's."""
    from test_engine_emu import check_native_vs_host
    a, b = check_native_vs_host(gpu_lib, None, "farmer", S=2000, solver=so, fused=fused)
    assert a.iterk_stats["straggler_stops"] > 0
    # y of the lanes another tier finished after a stop, and the host loop's
    kkt_recheck(a, tag="farmer stragglers %s fused=%d, device loop" % (so, fused))
    kkt_recheck(b, tag="farmer stragglers %s, host loop" % (so,))


def test_affine_map_path_matches_oracle_gpu(gpu_lib, monkeypatch):
    """Opt-in affine solution maps (PHX_LANE_MAP=1, phx_lane.h map_apply): the
    map pass + rounds pass give the oracle's PH trajectory."""
    monkeypatch.setenv("PHX_LANE_MAP", "1")
    S = 300
    ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), {"num_scens": S},
                                    6, lib=gpu_lib)
    o = oph.OraclePH([om.farmer("scen%d" % i, num_scens=S) for i in range(S)], rho=1.0)
    oc, oE, otb = o.ph_main(6)
    assert rel(ph.W_array(), o.W) < 1e-7
    assert rel(conv, oc) < 1e-7 and rel(Eobj, oE) < 1e-9 and rel(tb, otb) < 1e-9


def test_hub_contract_gpu(gpu_lib):
    from test_hub_spoke_emu import check_hub
    check_hub(gpu_lib, None, S=300)


def test_lagrangian_spoke_gpu(gpu_lib):
    from test_hub_spoke_emu import check_lagrangian_spoke
    check_lagrangian_spoke(gpu_lib, None, S=300)


def test_sslp_ph_gpu(gpu_lib):
    """sslp_15_45_5 LP relaxation (n = 705, m = 60: generic PDHG + polish path) vs the oracle."""
    from test_sslp import check_sslp_ph
    check_sslp_ph(gpu_lib, None, iters=3)


def test_sslp_synthetic_batch_gpu(gpu_lib):
    """400 synthetic sslp scenarios (batch creator): every subproblem certified, the
    trivial bound equal to the oracle's."""
    from mpisppy_amd.examples import sslp
    names = sslp.scenario_names_creator(400)
    ph, conv, Eobj, tb = run_engine(sslp.scenario_creator, names, {}, 1, lib=gpu_lib)
    assert all_certified(ph)
    o = oph.OraclePH([om.sslp(nm) for nm in names], rho=1.0)
    assert rel(tb, o.iter0()) < 1e-8


def test_aircond_bf10x10x10_gpu(gpu_lib):
    """configs[3]: aircond branching 10x10x10 (1,000 scenarios, 111 non-leaf nodes,
    per-node x-bar reductions) through the device-driven loop, vs the oracle."""
    from mpisppy_amd.utils import sputils
    bfs = [10, 10, 10]
    names = ["scen%d" % i for i in range(1000)]
    ph, conv, Eobj, tb = run_engine(aircond.scenario_creator, names, {"branching_factors": bfs}, 3, lib=gpu_lib,
                                    all_nodenames=sputils.create_nodenames_from_branching_factors(bfs))
    assert hasattr(ph, "iterk_stats")
    o = oph.OraclePH([om.aircond(n, bfs) for n in names], rho=1.0)
    oc, oE, otb = o.ph_main(3)
    assert rel(tb, otb) < 1e-9
    assert rel(Eobj, oE) < 1e-8
    assert rel(ph.W_array(), o.W) < 1e-6
    assert len(ph.xbar_by_node()) == 111


def test_farmer_cm10_1000_workgroup_gpu(gpu_lib):
    """BASELINE configs[1] (farmer crops_multiplier=10, 1,000 scenarios, n=120:
    generic path).  The workgroup warm active-set pass (k_wg_warm, phx_wg.h)
    certifies the later PH iterations without PDHG; its trajectory equals the
    PDHG + polish path's, and a sample re-solved by the oracle from the engine's
    own W / x-bar agrees in optimum value to 1e-8 (the oracle's point is never
    better; see test_engine_emu.test_farmer_cm10_workgroup_warm_pass)."""
    S, it = 1000, 5
    kw = {"num_scens": S, "crops_multiplier": 10}
    res = {}
    for wg in (1, 0):
        so = {"wg_warm": 16 * wg, "native_loop": 0}   # per-solve statistics: the host loop
        res[wg] = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), kw, it, lib=gpu_lib,
                             options={"iter0_solver_options": so, "iterk_solver_options": so})
    ph1, ph0 = res[1][0], res[0][0]
    assert all(r["not_optimal"] == 0 for r in ph1.solve_stats + ph0.solve_stats)
    wgc = [r["wg_certified"] for r in ph1.solve_stats]
    assert wgc[0] == 0 and wgc[-1] == S, wgc
    assert rel(ph1.xbar_by_node()["ROOT"][0], ph0.xbar_by_node()["ROOT"][0]) < 1e-8
    assert rel(ph1.W_array(), ph0.W_array()) < 1e-6
    assert rel(res[1][2], res[0][2]) < 1e-9
    kkt_recheck(ph1, tag="farmer cm=10, workgroup pass")
    kkt_recheck(ph0, tag="farmer cm=10, wg_warm 0")
    W, xb, xn, obj = ph1.W_array(), ph1.xbar_by_node()["ROOT"][0], ph1.nonant_values(), ph1._host("obj")
    sample = [0, 1, 2, 3, 500, 998, 999]
    o = oph.OraclePH([om.farmer("scen%d" % k, crops_multiplier=10, num_scens=S) for k in sample], rho=1.0)
    o.W_on = o.prox_on = 1
    o.W[:] = W[sample]
    o.xbar[:] = xb[None, :]
    o.solve_loop()
    assert rel(o.obj, obj[sample]) < 1e-8
    assert rel(o.xn(), xn[sample]) < 1e-6
    # full W / x-bar trajectory of all 1,000 scenarios: the oracle's iterations 1..it
    # from the engine's Iter0 point (degenerate Iter0 vertices)
    ph00 = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), kw, 0, lib=gpu_lib)[0]
    oc = oracle_continue_from(ph00, [om.farmer("scen%d" % k, crops_multiplier=10, num_scens=S) for k in range(S)], it)
    assert rel(W, oc.W) < 1e-6
    assert rel(xb, oc.xbar[0]) < 1e-8


def test_wxbar_writer_reader_gpu(gpu_lib, tmp_path):
    """W / x-bar CSV checkpoint I/O through the device state: the reference's
    fixture and asserts (test_w_writer.py), see tests/test_wxbar.py."""
    import test_wxbar as tw
    tw.check_writer(gpu_lib, None, tmp_path)
    tw.check_reader(gpu_lib, None)


def check_time_to_conv(lib, device, S):
    """Time to conv < 1e-4 (BASELINE.json metric, second half): PH.ph_main with
    convthresh = 1e-4 through the device-driven loop stops at the oracle's iteration
    (farmer-3: 94, farmer-30: 376) with the oracle's x-bar; farmer-3's
    x-bar matches the reference's converged nonants
    (rho_test_data/farmer_cyl_nonants.npy, abs 2e-3 as test_oracle_golden.py)."""
    names = farmer.scenario_names_creator(S)
    ph = PH(ph_options(2000, convthresh=1e-4), names, farmer.scenario_creator,
            scenario_creator_kwargs={"num_scens": S}, _native_lib=lib, _device=device)
    conv, Eobj, tb = ph.ph_main()
    o = oph.OraclePH([om.farmer(n, num_scens=S) for n in names], rho=1.0)
    oc, oE, otb = o.ph_main(2000, 1e-4)
    assert o.iter == {3: 94, 30: 376}[S]
    assert ph._PHIter == o.iter and conv < 1e-4
    assert rel(conv, oc) < 1e-6
    assert rel(ph.xbar_by_node()["ROOT"][0], o.xbar[0]) < 1e-6
    assert rel(Eobj, oE) < 1e-8
    if S == 3:
        ref = np.array(G["farmer3_converged_nonants"]["CORN0,SUGAR_BEETS0,WHEAT0"])
        assert np.max(np.abs(ph.xbar_by_node()["ROOT"][0] - ref)) < 2e-3
    return ph


@pytest.mark.parametrize("S", [3, 30])
def test_time_to_conv_gpu(gpu_lib, S):
    ph = check_time_to_conv(gpu_lib, None, S)
    assert ph.iterk_stats["converged"]          # the device-driven loop ran the whole solve


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["PHX_FENCED_HANDOFF", "PHX_RELAXED_HANDOFF"])
@pytest.mark.parametrize("S", [1000, 20000])
def test_handoff_variants_fused_loop_gpu(gpu_lib, monkeypatch, S, variant):
    """The fused loop's inter-workgroup hand-off in its two opt-in variants --
    release fences on the producers too (PHX_FENCED_HANDOFF), or no acquire on
    the consumers (PHX_RELAXED_HANDOFF: `sc1` loads alone) -- gives the host
    loop's trajectory, as the default (write-through producers, acquiring
    consumers; phx_lane.h) does; at 20k scenarios (79 workgroups) every arrival
    shard and the top counter are used."""
    monkeypatch.setenv("PHX_LANE_DEFS", variant)
    from test_engine_emu import check_native_vs_host
    a, b = check_native_vs_host(gpu_lib, None, "farmer", S=S, fused=1)
    assert a.iterk_stats["fused"]


@pytest.mark.gpu
def test_infeasible_iter0_status_gpu(gpu_lib):
    from test_engine_emu import check_infeasible_iter0_status
    check_infeasible_iter0_status(gpu_lib, None)


@pytest.mark.gpu
def test_infeasible_deferred_iter0_gpu(gpu_lib):
    from test_engine_emu import check_infeasible_deferred_iter0
    check_infeasible_deferred_iter0(gpu_lib, None)


@pytest.mark.gpu
def test_unseeded_and_seeded_iter0_agree_gpu(gpu_lib, monkeypatch):
    """Iter0 seeds from templates only when the batch has more wavefronts than
    SIMDs (phx_solve); both routes certify every lane at the same optimum
    (PHX_FORCE_SEED takes the seeded route at 20k scenarios)."""
    import torch
    S = 20000
    runs = []
    for force in (False, True):
        if force:
            monkeypatch.setenv("PHX_FORCE_SEED", "1")
        ph = PH(ph_options(0), farmer.scenario_names_creator(S), farmer.scenario_creator,
                scenario_creator_kwargs={"num_scens": S}, _native_lib=gpu_lib)
        conv, Eobj, tb = ph.ph_main()
        runs.append((ph._obj.cpu().numpy().copy(), tb, ph._status.cpu().numpy().copy()))
        del ph
        torch.cuda.empty_cache()
    (o0, tb0, s0), (o1, tb1, s1) = runs
    assert (s0 == 1).all() and (s1 == 1).all()
    assert rel(o0, o1) < 1e-9
    assert abs(tb0 - tb1) <= 1e-9 * abs(tb0)


@pytest.mark.gpu
def test_stream_mismatch_raises_gpu(gpu_lib):
    """An object built on one stream and run inside torch.cuda.stream(other) raises
    (its torch-side reads would not be ordered after the native kernels)."""
    import torch
    S = 30
    ph = PH(ph_options(3), farmer.scenario_names_creator(S), farmer.scenario_creator,
            scenario_creator_kwargs={"num_scens": S}, _native_lib=gpu_lib)
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(RuntimeError, match="not the stream"):
            ph.ph_main()


def test_native_loop_workgroup_matches_host_loop_gpu(gpu_lib):
    """farmer crops_multiplier=10 x 1000 (configs[1]): phx_iterk runs the
    workgroup warm pass per iteration, bit-equal to the host loop."""
    from test_engine_emu import check_native_vs_host_wg
    a, b = check_native_vs_host_wg(gpu_lib, None, S=1000, iters=6)
    assert a.iterk_stats["not_optimal"] == 0


@pytest.mark.parametrize("ipm_cut", [0, 1])
def test_native_loop_workgroup_stragglers_gpu(gpu_lib, ipm_cut):
    """One workgroup round per solve: the lanes it leaves go on to the sparse
    solver's interior point in the stream (no pipeline stop); with that interior
    point cut to 2 iterations (ipm_cut) its leftovers stop the device loop,
    which finishes them with PDHG + polish and resumes.  Either way the host
    loop's trajectory, bit for bit."""
    from test_engine_emu import check_native_vs_host_wg
    a, b = check_native_vs_host_wg(gpu_lib, None, S=300, iters=5, solver={"wg_warm": 1},
                                   iterk_extra={"ipm_max_it": 2} if ipm_cut else None)
    if ipm_cut:
        assert a.iterk_stats["straggler_stops"] > 0
    else:
        assert a.iterk_stats["straggler_stops"] == 0


def test_wg_first_budget_after_gated_pass_gpu(gpu_lib):
    """the first warm workgroup pass's round budget (wg_first) belongs
    to the first pass that RUNS after a cold solve.  A device loop that stops at
    iteration 1 (converged: its pass enqueued, gated, never run) gives the budget
    back, so a second loop call's first pass gets wg_first as the host loop's
    does; then a straggler-stopping loop (the sparse interior point cut short).
    Both continuations equal the host loop's bit for bit."""
    runs = []
    for nl in (1, 0):
        so = {"wg_warm": 8, "wg_first": 1, "ipm_max_it": 2, "native_loop": nl}
        opts = ph_options(4, convthresh=1e9)
        opts["iter0_solver_options"] = {"wg_warm": 8, "wg_first": 1}
        opts["iterk_solver_options"] = so
        ph = PH(opts, farmer.scenario_names_creator(120), farmer.scenario_creator,
                scenario_creator_kwargs={"num_scens": 120, "crops_multiplier": 10}, _native_lib=gpu_lib)
        ph.ph_main(finalize=False)
        assert ph._PHIter == 1                  # converged at iteration 1: no solve ran
        ph.options["convthresh"] = 1e-10
        ph.iterk_loop()
        ph._settle()
        runs.append(ph)
    a, b = runs
    assert a.iterk_stats["iters"] == 4 and not hasattr(b, "iterk_stats")
    assert np.array_equal(a.W_array(), b.W_array())
    assert np.array_equal(a.nonant_values(), b.nonant_values())


def test_sp_off_on_sparse_context_raises_gpu(gpu_lib):
    """sp = 0 (the dense generic path) on a context that holds the sparse
    solver's workspaces only: refused with an error, not run on absent buffers."""
    from mpisppy_amd._native import NativeError
    so = {"wg_warm": 1, "sp": 0}
    with pytest.raises(NativeError, match="sp = 0"):
        run_engine(farmer.scenario_creator, farmer.scenario_names_creator(30), {"num_scens": 30, "crops_multiplier": 10},
                   2, lib=gpu_lib, options={"iter0_solver_options": dict(so), "iterk_solver_options": dict(so)})


@pytest.mark.parametrize("fused", [0, 1])
def test_native_rccl_path_one_rank_gpu(gpu_lib, fused):
    """phx_iterk's own RCCL all-reduce (phx_set_comm + ncclAllReduce on the loop's
    stream: the N > 1 path with the device-side conv test after the collective),
    exercised on one rank through a one-rank communicator: the same trajectory
    as the single-rank loop."""
    S = 2000
    res = []
    for nc in (0, 2):
        so = {"native_comm": nc, "iterk_fused": fused}
        ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), {"num_scens": S},
                                        6, lib=gpu_lib, options={"iter0_solver_options": so,
                                                                 "iterk_solver_options": so})
        assert ph._native_comm == bool(nc) and hasattr(ph, "iterk_stats")
        assert bool(ph.iterk_stats["fused"]) == bool(fused)
        res.append((ph.W_array(), ph.xbar_by_node()["ROOT"][0], conv, Eobj))
    (W0, x0, c0, E0), (W1, x1, c1, E1) = res
    assert rel(W1, W0) < 1e-12 and rel(x1, x0) < 1e-12
    assert rel(c1, c0) < 1e-12 and rel(E1, E0) < 1e-12


def test_wg_factor_cache_gpu(gpu_lib, monkeypatch):
    """k_wg_warm's factor cache reproduces the recomputed-factor trajectory bit for bit
    (farmer crops_multiplier=10)."""
    from test_engine_emu import check_wg_factor_cache
    check_wg_factor_cache(gpu_lib, None, monkeypatch, S=1000, iters=6)


@pytest.mark.parametrize("so0", [None, {"as_rounds": 0, "ipm_max_it": 2}])
def test_deferred_iter0_gpu(gpu_lib, so0):
    """ph_main's deferred Iter0 (phx_iterk adopts the pending solve; with starved
    Iter0 solves its leftovers stop the pipeline at iteration 1 and are finished)
    == the step-by-step run, bit for bit."""
    from test_engine_emu import check_deferred_iter0
    a, b = check_deferred_iter0(gpu_lib, None, S=3000, iter0_solver=so0)
    assert a.iterk_stats["fused"]
    if so0:
        assert a.solve_stats[0]["stragglers"] > 0


@pytest.mark.parametrize("env,creator_kw,levels", [
    # farmer cm=10: A varies (the split area holds A's values, the pattern is shared)
    ("PHX_WG_SPLIT", ("farmer", {"num_scens": 300, "crops_multiplier": 10}), ("0", "1")),
    # sslp: A constant (pattern and A shared by every workgroup; the default layout)
    ("PHX_WG_SPLIT", ("sslp", {"num_scens": 64}), ("0", "1")),
    # level 2: the row vector in the scratch slot too
    ("PHX_SP_SPLIT", ("sslp", {"num_scens": 64}), ("0", "1", "2")),
    # the sparse scratch's row vectors in LDS (the default where they fit) or in the slot
    ("PHX_SP_ROWS_LDS", ("sslp", {"num_scens": 64}), ("1", "0")),
])
def test_split_layouts_bit_equal_gpu(gpu_lib, monkeypatch, env, creator_kw, levels):
    """The workgroup / sparse solvers' split layouts (per-scenario vectors in a
    global area instead of LDS, scenario-invariant arrays shared: phx_wg.h /
    phx_sp.h) move memory, not arithmetic: the same PH trajectory bit for bit as
    the all-LDS layout."""
    from mpisppy_amd.examples import sslp
    mod = farmer if creator_kw[0] == "farmer" else sslp
    kw = creator_kw[1]
    names = mod.scenario_names_creator(kw["num_scens"])
    out = {}
    for v in levels:
        monkeypatch.setenv(env, v)
        ph, conv, E, tb = run_engine(mod.scenario_creator, names, kw, 3, lib=gpu_lib)
        assert all_certified(ph)
        out[v] = (ph.W_array(), ph.xbar_by_node()["ROOT"][0], E, tb)
    for v in levels[1:]:
        assert np.array_equal(out[levels[0]][0], out[v][0]), v
        assert np.array_equal(out[levels[0]][1], out[v][1]), v
        assert out[levels[0]][2] == out[v][2] and out[levels[0]][3] == out[v][3], v


def test_window_timing_fused_loop_gpu(gpu_lib):
    """iterk_timing < 0 (bench.py's default): one event pair around every fused
    launch of the run (iteration 1 after Iter0 is the unfused rescue iteration,
    so iterations 2..K), and the same trajectory as the untimed loop."""
    S, K = 1000, 10
    names = farmer.scenario_names_creator(S)
    a, _, _, _ = run_engine(farmer.scenario_creator, names, {"num_scens": S}, K, lib=gpu_lib,
                            options={"iterk_solver_options": {"iterk_timing": -5}})
    b, _, _, _ = run_engine(farmer.scenario_creator, names, {"num_scens": S}, K, lib=gpu_lib)
    st = a.iterk_stats
    assert st["fused"] and st["iters"] == K
    assert st["warm_launches"] == K - 1 and st["lane_warm_ms"] > 0.0
    assert np.array_equal(a.W_array(), b.W_array())


def test_per_rank_slice_12500_gpu(gpu_lib):
    """The 8-GPU per-rank slice (C3s8: farmer 12,500 on one GPU): the unseeded
    Iter0 at one wavefront per SIMD, the one-launch small-batch solve
    (phx_lane_all) of the first iteration and the one-wave fused kernel
    (phx_lane_warm_fz1) after it == the Python loop (x-bar, W, nonants,
    conv, E[obj] to 1e-9; the fused sums run in another fixed order)."""
    from test_engine_emu import check_native_vs_host
    check_native_vs_host(gpu_lib, None, "farmer", S=12500, fused=1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["farmer100k", "aircond1k"])
def test_register_resident_rescue_rounds_gpu(gpu_lib, monkeypatch, case):
    """The rescue-list kernel and phx_lane_all run their rounds on the data
    loaded at entry (phx_lane.h warm_lane<.., REG>); the re-loading builds
    (PHX_LIST_RELOAD, PHX_ALL_RELOAD) run the same arithmetic on the same
    values: both give the same PH trajectory (farmer 100k: the first
    iteration's rescue list; aircond 10x10x10: phx_lane_all's rescue rounds)."""
    from mpisppy_amd.examples import aircond, farmer
    from mpisppy_amd.utils import sputils
    runs = []
    for defs in ("", "PHX_LIST_RELOAD PHX_ALL_RELOAD"):
        monkeypatch.setenv("PHX_LANE_DEFS", defs)
        if case == "farmer100k":
            S = 100000
            r = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), {"num_scens": S}, 3,
                           lib=gpu_lib, device="cuda")
        else:
            bfs = [10, 10, 10]
            r = run_engine(aircond.scenario_creator, ["scen%d" % i for i in range(1000)],
                           {"branching_factors": bfs, "start_seed": 0}, 6, lib=gpu_lib, device="cuda",
                           all_nodenames=sputils.create_nodenames_from_branching_factors(bfs))
        assert all(s["not_optimal"] == 0 for s in r[0].solve_stats)
        runs.append(r)
    (a, ca, Ea, ta), (b, cb, Eb, tb) = runs
    assert rel(a.W_array(), b.W_array()) < 1e-12
    assert abs(Ea - Eb) <= 1e-12 * abs(Ea) and abs(ca - cb) <= 1e-12 * max(1.0, abs(ca))
