"""Scenario-donor xhat inner bounds on CPU (the ABI emulation): the two entry
points phx_donor_gather / phx_fix_nonants against a numpy restatement,
XhatBase._try_one against the oracle's fixed-xhat evaluation, two gloo ranks,
ScenarioCycler, the xhatshuffle wheel and the XhatSpecific / XhatLooper
extensions.  The GPU versions (fixed-nonant lane module) are in
test_xhat_donor_gpu.py."""
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import xhat_cases as xc
from helpers import ph_options, rel
from mpisppy_amd.cylinders.xhatshufflelooper_bounder import ScenarioCycler
from mpisppy_amd.examples import farmer
from mpisppy_amd.extensions.xhatbase import XhatBase
from mpisppy_amd.extensions.xhatlooper import XhatLooper
from mpisppy_amd.extensions.xhatspecific import XhatSpecific
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.utils import sputils
from oracle import models as om, ph as oph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- entry points
@pytest.mark.parametrize("S", xc.S_LIST)
def test_gather_and_fix_farmer_emu(emu, S):
    ev, _ = xc.make_eval(emu, "cpu", "farmer", S)
    xc.check_gather(ev)
    xc.check_fix(ev)


@pytest.mark.parametrize("bf", [(2, 2), (3, 2)])
def test_gather_and_fix_aircond_emu(emu, bf):
    ev, nodes = xc.make_eval(emu, "cpu", "aircond", bf)
    assert len(xc.local_nodes(ev)) == 1 + bf[0]
    xc.check_gather(ev)
    xc.check_fix(ev)


def test_symbols_exported(emu):
    assert hasattr(emu, "donor_gather") and hasattr(emu, "fix_nonants")


# ---------------------------------------------------------------- _try_one
def test_try_one_farmer3_emu(emu):
    ev, _ = xc.make_eval(emu, "cpu", "farmer", 3)
    xc.check_try_one(ev, "farmer", 3, [{"ROOT": "scen0"}, {"ROOT": "scen2"}, {"ROOT": "scen1"}, {"ROOT": "scen1"}])


def test_try_one_farmer30_emu(emu):
    ev, _ = xc.make_eval(emu, "cpu", "farmer", 30)
    xc.check_try_one(ev, "farmer", 30, [{"ROOT": "scen29"}, {"ROOT": "scen0"}, {"ROOT": "scen17"}])


AIRCOND_DONORS = [{"ROOT": "scen3", "ROOT_0": "scen1", "ROOT_1": "scen2", "ROOT_2": "scen5"},
                  {"ROOT": "scen0", "ROOT_0": "scen0", "ROOT_1": "scen3", "ROOT_2": "scen4"},
                  {"ROOT": "scen5", "ROOT_0": "scen1", "ROOT_1": "scen3", "ROOT_2": "scen5"}]


def test_try_one_aircond_emu(emu):
    ev, _ = xc.make_eval(emu, "cpu", "aircond", (3, 2))
    xc.check_try_one(ev, "aircond", (3, 2), AIRCOND_DONORS)


def test_try_one_infeasible_emu(emu):
    ev, _ = xc.make_eval(emu, "cpu", "farmer", 3, solver_options={"pdhg_max_iters": 4096})
    ev.current_solver_options = {"pdhg_max_iters": 4096}
    S = 3
    ev._save_original_nonants()
    ev._lazy_create_solvers()
    ev._save_nonants()
    bad = np.tile([300.0, 300.0, 300.0], S)
    ev._put_nonant_cache(bad)
    ev._restore_nonants()
    xb = XhatBase(ev)
    assert xb._try_one({"ROOT": "scen0"}, solver_options={"pdhg_max_iters": 4096}, restore_nonants=False) is None
    assert ev.solve_stats[-1]["infeasible"] == S
    assert np.array_equal(ev.nonant_values(), bad.reshape(S, 3))
    assert not ev._fixed.any()
    # the next solve is the unfixed problem again
    ev.solve_loop()
    assert ev.infeas_prob() == 0.0


def test_try_one_errors_emu(emu):
    ev, _ = xc.make_eval(emu, "cpu", "aircond", (3, 2))
    xb = XhatBase(ev)
    good = dict(AIRCOND_DONORS[0])
    with pytest.raises(RuntimeError, match="ROOT_1 not in snamedict="):
        xb._try_one({k: v for k, v in good.items() if k != "ROOT_1"})
    with pytest.raises(RuntimeError, match="Bad scenario selection for xhat"):
        xb._try_one(dict(good, ROOT_0="scen4"))           # scen4 is not a scenario of ROOT_0
    with pytest.raises(NotImplementedError, match="stage2EFsolvern"):
        xb._try_one(good, stage2EFsolvern="an_ef_solver", branching_factors=[3, 2])
    ev2, _ = xc.make_eval(emu, "cpu", "farmer", 3)
    with pytest.raises(KeyError):
        XhatBase(ev2)._try_one({"ROOT_0": "scen0"})
    with pytest.raises(RuntimeError, match="Bad scenario selection for xhat"):
        XhatBase(ev2)._try_one({"ROOT": "scen7"})


def test_tree_nodes_and_ranks_emu(emu):
    ev, _ = xc.make_eval(emu, "cpu", "aircond", (3, 2))
    nl = ev.nonleaf_nodes
    assert list(nl) == ["ROOT", "ROOT_0", "ROOT_1", "ROOT_2"]
    assert [(nd.scenfirst, nd.scenlast) for nd in nl.values()] == [(0, 5), (0, 1), (2, 3), (4, 5)]
    assert [k.name for k in nl["ROOT"].kids] == ["ROOT_0", "ROOT_1", "ROOT_2"] and not nl["ROOT"].kids[0].is_leaf
    assert nl["ROOT_1"].kids[0].is_leaf
    assert ev.scenario_names_to_rank["ROOT_1"] == {"scen2": 0, "scen3": 0}
    ev2, _ = xc.make_eval(emu, "cpu", "farmer", 5)
    assert (ev2.nonleaf_nodes["ROOT"].scenfirst, ev2.nonleaf_nodes["ROOT"].scenlast) == (0, 4)
    assert ev2.nonleaf_nodes["ROOT"].kids == []
    assert ev2.scenario_names_to_rank == {"ROOT": {"scen%d" % i: 0 for i in range(5)}}


# ---------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_rank_case(lib, case, comm=None):
    """(E, fixed nonant values, donors' cache values) of one trial of ``case``."""
    if case == "farmer":
        model, size, donors = "farmer", 9, {"ROOT": "scen7"}
    else:
        # ROOT_1 = {scen2, scen3} is cut by the rank boundary; its donor and ROOT's are rank 1's
        model, size, donors = "aircond", (3, 2), {"ROOT": "scen4", "ROOT_0": "scen1", "ROOT_1": "scen3",
                                                  "ROOT_2": "scen5"}
    ev, _ = xc.make_eval(lib, "cpu", model, size, mpicomm=comm)
    scens = xc.oracle_scens(model, size)
    o = oph.OraclePH(scens, rho=1.0)
    o.iter0()
    lo, hi = ev._local_lo, ev._local_hi
    ev._save_original_nonants()
    ev._lazy_create_solvers()
    ev._save_nonants()
    ev._put_nonant_cache(o.xn()[lo:hi].ravel())
    ev._restore_nonants()
    E = XhatBase(ev)._try_one(donors, restore_nonants=False)
    cache = xc.donor_cache(o, donors)
    want = np.array([[cache[o.node_of[s][j]][ev.batch.nonant.slot_local[j]] for j in range(o.N)]
                     for s in range(lo, hi)])
    Eo, _, _ = oph.evaluate_xhat(scens, cache)
    return E, ev.nonant_values(), want, Eo, ev.scenario_names_to_rank


def _worker2(rank, world, port, out, case):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.comm import Comm
    emu = _native.Lib(os.path.join(ROOT, "tests", "emu", "libphx_emu.so"), prefix="emu_phx_")
    out[rank] = _one_rank_case(emu, case, comm=Comm())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["farmer", "aircond"])
def test_try_one_two_ranks(emu, case):
    """Donors on rank 1: both ranks return the one-rank objective, and rank 0's
    nonants are fixed at the donors' bits (one all-reduce instead of the
    reference's per-node bcast)."""
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker2, args=(2, _free_port(), out, case), nprocs=2, join=True)
    E1, fixed1, want1, Eo, _ = _one_rank_case(emu, case)
    assert rel(E1, Eo) < 1e-9 and np.array_equal(fixed1, want1)
    for r in range(2):
        E, fixed, want, _, ranks = out[r]
        assert E == pytest.approx(E1, rel=1e-12)
        assert np.array_equal(fixed, want), r
    assert np.array_equal(np.vstack([out[0][1], out[1][1]]), fixed1)
    ranks = out[0][4]
    if case == "farmer":
        assert ranks["ROOT"]["scen3"] == 0 and ranks["ROOT"]["scen7"] == 1
    else:
        assert ranks["ROOT_1"] == {"scen2": 0, "scen3": 1}


# ---------------------------------------------------------------- ScenarioCycler
def _shuffled(n):
    names = list(enumerate("scen%d" % i for i in range(n)))
    return random.Random(42).sample(names, len(names))


def test_cycler_two_stage():
    n = 7
    sh = _shuffled(n)
    nl = sputils.nonleaf_tree_nodes(["ROOT"], n)
    cyc = ScenarioCycler(sh, nl, True, None)
    for epoch in range(2):
        got = [cyc.get_next() for _ in range(n)]
        assert [d["ROOT"] for d in got] == [nm for _, nm in sh]        # every scenario once, shuffled order
        assert all(list(d) == ["ROOT"] for d in got)
        assert cyc.get_next() is None and cyc.get_next() is None
        cyc.begin_epoch()                                               # (two-stage: never reversed)
    # iter_step
    cyc = ScenarioCycler(sh, nl, True, 3)
    got = [cyc.get_next()["ROOT"] for _ in range(n)]
    assert got[:3] == [sh[0][1], sh[3][1], sh[6][1]] and sorted(got) == sorted(nm for _, nm in sh)
    assert cyc.get_next() is None
    cyc.best = {"ROOT": "scen1"}
    assert cyc.best == {"ROOT": "scen1"}


@pytest.mark.parametrize("bf", [(2, 2), (3, 2)])
def test_cycler_multistage(bf):
    n = int(np.prod(bf))
    sh = _shuffled(n)
    order = [nm for _, nm in sh]
    num = {nm: k for k, nm in sh}
    nl = sputils.nonleaf_tree_nodes(sputils.create_nodenames_from_branching_factors(list(bf)), n)
    assert len(nl) == 1 + bf[0]

    def epoch(cyc):
        dicts = []
        while True:
            d = cyc.get_next()
            if d is None:
                return dicts
            dicts.append(dict(d))
            assert len(dicts) <= n

    def check(dicts, seq, step):
        roots = [d["ROOT"] for d in dicts]
        assert len(set(roots)) == len(roots) == n                      # no ROOT donor twice, all visited
        for d in dicts:
            assert set(d) == set(nl)                                    # every non-leaf node covered
            for ndn, sname in d.items():
                assert nl[ndn].scenfirst <= num[sname] <= nl[ndn].scenlast
        # ROOT advances by `step` along the epoch's order, skipping visited ones
        pos, seen, want = 0, set(), []
        for _ in range(n):
            want.append(seq[pos])
            seen.add(seq[pos])
            pos = (pos + step) % n
            start = pos
            while seq[pos] in seen and (pos + 1) % n != start:
                pos = (pos + 1) % n
        assert roots == want
        # every other node: the first scenario of the node from the ROOT donor on
        for d in dicts:
            p = seq.index(d["ROOT"])
            for ndn in nl:
                q = p
                while not (nl[ndn].scenfirst <= num[seq[q]] <= nl[ndn].scenlast):
                    q = (q + 1) % n
                assert d[ndn] == seq[q], (ndn, d)

    cyc = ScenarioCycler(sh, nl, None, None)                            # reverse None -> True, step BF0
    assert cyc.BF0 == bf[0]
    check(epoch(cyc), order, bf[0])
    cyc.begin_epoch()
    check(epoch(cyc), order[::-1], bf[0])                               # the reverse epoch
    cyc.begin_epoch()
    check(epoch(cyc), order, bf[0])                                     # forward again
    cyc = ScenarioCycler(sh, nl, False, 1)                              # reverse off, iter_step 1
    check(epoch(cyc), order, 1)
    cyc.begin_epoch()
    check(epoch(cyc), order, 1)


# ---------------------------------------------------------------- the wheel
WS = 6


def _worker_wheel(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.comm import Comm
    from mpisppy_amd.cylinders import LagrangianOuterBound, PHHub, XhatShuffleInnerBound
    from mpisppy_amd.phbase import PHBase
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    emu = _native.Lib(os.path.join(ROOT, "tests", "emu", "libphx_emu.so"), prefix="emu_phx_")
    names = farmer.scenario_names_creator(WS)
    tried = []

    class RecordingShuffle(XhatShuffleInnerBound):
        def try_scenario_dict(self, d):
            k = names.index(d["ROOT"])
            self._donor_vals = self.opt.nonant_cache[k].copy()
            return super().try_scenario_dict(d)

        def update_if_improving(self, b):
            sent = super().update_if_improving(b)
            tried.append((self._donor_vals, b, sent))
            return sent

    okw = dict(options=ph_options(200), all_scenario_names=names, scenario_creator=farmer.scenario_creator,
               scenario_creator_kwargs={"num_scens": WS}, _native_lib=emu, _device="cpu")
    xopts = dict(ph_options(200))
    xopts["xhat_looper_options"] = {"xhat_solver_options": {}, "scen_limit": 3}
    hub_dict = {"hub_class": PHHub, "hub_kwargs": {"options": {"rel_gap": 0.01, "display_progress": False}},
                "opt_class": PH, "opt_kwargs": dict(okw)}
    spokes = [{"spoke_class": LagrangianOuterBound, "opt_class": PHBase, "opt_kwargs": dict(okw)},
              {"spoke_class": RecordingShuffle, "opt_class": Xhat_Eval, "opt_kwargs": dict(okw, options=xopts)}]
    wheel = WheelSpinner(hub_dict, spokes)
    wheel.spin(comm_world=Comm())
    rec = {"strata_rank": wheel.strata_rank}
    if wheel.strata_rank == 0:
        rec.update(best_outer=wheel.BestOuterBound, best_inner=wheel.BestInnerBound,
                   iters=wheel.spcomm.opt._PHIter)
    elif wheel.strata_rank == 2:
        rec.update(tried=tried, best=wheel.spcomm.best_inner_bound, char=wheel.spcomm.converger_spoke_char)
    out[rank] = rec
    dist.barrier()
    dist.destroy_process_group()


def test_wheel_xhatshuffle(emu):
    """PH hub + Lagrangian + xhatshuffle: the hub stops on rel_gap; every inner
    bound the spoke sent is the oracle's evaluation of the donor values it came
    from; the final inner bound is not below the EF optimum."""
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker_wheel, args=(3, _free_port(), out), nprocs=3, join=True)
    res = [out[r] for r in range(3)]
    hub = [r for r in res if r["strata_rank"] == 0][0]
    xs = [r for r in res if r["strata_rank"] == 2][0]
    assert xs["char"] == "X"
    scens = [om.farmer("scen%d" % i, num_scens=WS) for i in range(WS)]
    ef, _, _ = oph.solve_ef(scens)
    gap = (hub["best_inner"] - hub["best_outer"]) / abs(hub["best_outer"])
    assert gap <= 0.01 and hub["iters"] < 200          # terminated on the gap, not the limit
    sent = [(v, b) for v, b, s in xs["tried"] if s]
    assert sent
    for v, b in sent:
        E, _, ok = oph.evaluate_xhat(scens, {"ROOT": v})
        assert ok.all()
        assert rel(b, E) < 1e-9
    assert xs["best"] == min(b for _, b in sent)
    assert hub["best_inner"] >= ef - 1e-7 * abs(ef)
    assert hub["best_outer"] <= ef + 1e-6 * abs(ef)


# ---------------------------------------------------------------- PH extensions
def _ph_with(emu, ext, extra):
    names = farmer.scenario_names_creator(3)
    opts = ph_options(5)
    opts.update(extra)
    ph = PH(opts, names, farmer.scenario_creator, scenario_creator_kwargs={"num_scens": 3}, extensions=ext,
            _native_lib=emu, _device="cpu")
    ph.ph_main()
    return ph, [om.farmer(n, num_scens=3) for n in names]


def test_xhatspecific_extension_emu(emu, tmp_path):
    csv = str(tmp_path / "xh")
    ph, scens = _ph_with(emu, XhatSpecific, {"xhat_specific_options": {
        "xhat_scenario_dict": {"ROOT": "scen1"}, "xhat_solver_options": {}, "csvname": csv}})
    assert hasattr(ph, "iterk_stats")                  # post_everything only: the device loop ran
    donor = ph.nonant_cache[1]
    E, _, ok = oph.evaluate_xhat(scens, {"ROOT": donor})
    assert ok.all() and rel(ph.extobject._xhat_specific_obj_final, E) < 1e-9
    # keep_solution: the nonants stay at the donor's values
    assert np.array_equal(ph.nonant_values(), np.tile(donor, (3, 1)))
    assert ph.tree_solution_available and ph.first_stage_solution_available
    line = open(csv + "_ROOT_scen1.csv").read().strip().split(", ")
    assert line[0] == "ROOT" and [float(v) for v in line[2::2]] == list(donor)


def test_xhatlooper_extension_emu(emu):
    ph, scens = _ph_with(emu, XhatLooper, {"xhat_looper_options": {
        "scen_limit": 3, "xhat_solver_options": {}, "keep_solution": False}})
    assert hasattr(ph, "iterk_stats")
    vals = [oph.evaluate_xhat(scens, {"ROOT": ph.nonant_cache[k]})[0] for k in range(3)]
    assert rel(ph.extobject._xhat_looper_obj_final, min(vals)) < 1e-9
    ph.disable_W_and_prox()                  # as post_everything does around the call (xhatlooper.py:117-123)
    obj, snamedict = ph.extobject.xhat_looper(scen_limit=2, restore_nonants=True)
    ph.reenable_W_and_prox()
    vals2 = [oph.evaluate_xhat(scens, {"ROOT": ph.nonant_cache[k]})[0] for k in range(2)]
    assert rel(obj, min(vals2)) < 1e-9 and snamedict == {"ROOT": "scen%d" % int(np.argmin(vals2))}
    # restored: nothing fixed, values as cached
    assert not ph._fixed.any() and np.array_equal(ph.nonant_values(), ph.nonant_cache)


# ---------------------------------------------------------------- the fixed module's source
@pytest.mark.parametrize("case", ["farmer", "aircond"])
def test_fixed_lane_source_compiles_gfx950(emu, case):
    """The fixed-nonant lane module's source (every nonant column fixed, every
    bound a per-scenario load) compiles for gfx950 with the library's kernel list."""
    import ctypes
    import test_jit_source as tj
    if not os.path.exists(tj._HIPRTC):
        pytest.skip("no hipRTC in this image")
    ev, _ = xc.make_eval(emu, "cpu", *(("farmer", 20) if case == "farmer" else ("aircond", (4, 3, 2))))
    fn = emu.lib.emu_phx_fixed_lane_source
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    src = fn(ev._ctx, 2).decode()
    assert "struct PT" in src and "bnd_vary() { return true; }" in src
    rc, log, code = tj.hiprtc_compile(src)
    assert rc == 0, log[-4000:]
    symbols = tj.elf_symbols(code)
    for k in tj.lane_kernels(emu):
        assert k in symbols, k
