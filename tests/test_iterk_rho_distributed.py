"""NormRhoUpdater inside the device loop on several ranks: every enqueued
iteration all-reduces the [NNS + 1] primal residuals between its absdev pass
and its rule (phx_iterk_norm_rho through the all-reduce callback), every rank
applies the rule to its own scenarios, and the run must match one process's
host loop as test_norm_rho_distributed.check_ranks asks: the same actions at
every iteration on the entries a rank holds, zeros on the others, the ranks'
rho stacked bit-equal, x-bar / W / conv to 1e-9 (the ranks' sums add in another
fixed order than one process's tiles).

gloo on the host emulation: farmer with 6 scenarios on 2 ranks, and hydro (9
scenarios, three stages) on 3 ranks, where no rank holds a scenario of every
tree node; one stop by convthresh on 2 ranks, where every rank must leave at
the same iteration with none left waiting in a collective.  One gpu case: hydro
on 3 processes, each with its own context on cuda:0, over gloo.
"""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_norm_rho_distributed import CASES, ROOT, _free_port, _rel


def _run_case(case, lib, device, native, mpicomm=None, conv_ranks=None, convthresh=None, extensions=None):
    import iterk_rho_cases as ic
    from mpisppy_amd.examples import farmer, hydro
    from mpisppy_amd.utils import sputils
    world, iters = CASES[case]
    options = {}
    if conv_ranks:
        options["conv_ranks"] = conv_ranks
    if convthresh is not None:
        options["convthresh"] = convthresh
    if case == "farmer":
        ph = ic.make(lib, device, farmer.scenario_creator, farmer.scenario_names_creator(6), {"num_scens": 6}, iters,
                     native, options=options, mpicomm=mpicomm, extensions=extensions)
    else:
        ph = ic.make(lib, device, hydro.scenario_creator, hydro.scenario_names_creator(9),
                     {"branching_factors": [3, 3]}, iters, native, options=options, mpicomm=mpicomm,
                     nodenames=sputils.create_nodenames_from_branching_factors([3, 3]), extensions=extensions)
    conv, Eobj, tb = ph.ph_main()
    present = np.zeros(ph.NNS, dtype=bool)
    present[np.unique(ph._xbar_idx)] = True
    out = {"conv": conv, "iters": ph._PHIter, "W": ph.W_array(), "rho": ph._host("rho").T.copy(),
           "xbar": {k: v[0] for k, v in ph.xbar_by_node().items()}, "present": present, "Eobj": Eobj, "tb": tb}
    if native:
        st = ph.iterk_stats
        out.update(actions=ic.update_rows(ph, st["rho_updates"]), not_optimal=st["not_optimal"], fused=st["fused"],
                   converged=st["converged"], updates=st["rho_updates"], have_prev=ph.extobject._have_prev)
    else:
        assert not hasattr(ph, "iterk_stats")
        out.update(actions=np.array(ph.extobject.seen), not_optimal=sum(s["not_optimal"] for s in ph.solve_stats),
                   convs=list(getattr(ph.extobject, "convs", [])), seen=ph.extobject.seen)
    return out


def _worker(rank, world, port, out, case, gpu, convthresh):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.comm import Comm
    if gpu:
        lib, device = _native.load(), "cuda:0"
    else:
        lib, device = _native.Lib(os.path.join(ROOT, "tests", "emu", "libphx_emu.so"), prefix="emu_phx_"), "cpu"
    # (an exception ends this rank at once: mp.spawn then stops its peers)
    out[rank] = _run_case(case, lib, device, True, mpicomm=Comm(), convthresh=convthresh)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(case, gpu, convthresh=None):
    world = CASES[case][0]
    # (a spawned manager: a parent holding a GPU context must not be forked)
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out, case, gpu, convthresh), nprocs=world, join=True)
    return [out[r] for r in range(world)]


def check_ranks(case, lib, device, gpu):
    world, iters = CASES[case]
    rs = _spawn(case, gpu)
    one = _run_case(case, lib, device, False, conv_ranks=world)
    assert one["present"].all() and one["actions"].shape == (iters - 1, len(one["present"]))
    assert len(set(one["actions"].ravel())) >= 3             # several kinds of action (and none) occurred
    covered = np.zeros_like(one["present"])
    for r in rs:
        assert r["iters"] == one["iters"] == iters and r["not_optimal"] == 0
        assert r["fused"] is False and r["updates"] == iters - 1 and r["have_prev"]
        if case == "hydro":
            assert not r["present"].all()                    # no rank covers every node
        # the same actions at every iteration; entries of absent nodes read 0
        assert np.array_equal(r["actions"][:, r["present"]], one["actions"][:, r["present"]])
        assert not r["actions"][:, ~r["present"]].any()
        covered |= r["present"]
        assert _rel(r["conv"], one["conv"]) < 1e-9
        for k, v in one["xbar"].items():
            assert _rel(r["xbar"][k], v) < 1e-9, k
    assert covered.all()
    assert np.array_equal(np.vstack([r["rho"] for r in rs]), one["rho"])
    assert not np.all(one["rho"] == 1.0)
    assert _rel(np.vstack([r["W"] for r in rs]), one["W"]) < 1e-9
    # one process with the emulated ranks' segments: its device loop equals its host loop bit for bit
    dev = _run_case(case, lib, device, True, conv_ranks=world)
    assert np.array_equal(dev["rho"], one["rho"]) and np.array_equal(dev["W"], one["W"])
    assert np.array_equal(dev["actions"], one["actions"])
    assert dev["conv"] == one["conv"] and dev["Eobj"] == one["Eobj"] and dev["tb"] == one["tb"]


@pytest.mark.parametrize("case", list(CASES))
def test_ranks_match_one_emu(emu, case):
    check_ranks(case, emu, "cpu", False)


@pytest.mark.timeout(120)
def test_convthresh_stop_on_two_ranks_emu(emu):
    """A stop chosen as iterk_rho_cases.check_convthresh_stop chooses it: both
    ranks leave at k* (the padded iterations' collectives pair up: none hangs),
    with the update of iteration k* applied."""
    import iterk_rho_cases as ic
    world, iters = CASES["farmer"]
    h = _run_case("farmer", emu, "cpu", False, conv_ranks=world, extensions=ic.ConvRecordingUpdater)
    kstar, thr = ic.conv_stop_threshold(h["convs"], h["seen"])
    assert kstar < iters
    one = _run_case("farmer", emu, "cpu", False, conv_ranks=world, convthresh=thr)
    assert one["iters"] == kstar and len(one["actions"]) == kstar - 1
    rs = _spawn("farmer", False, convthresh=thr)
    for r in rs:
        assert r["iters"] == kstar and r["converged"] and r["updates"] == kstar - 1
        assert _rel(r["conv"], one["conv"]) < 1e-9 and r["conv"] < thr
        assert np.array_equal(r["actions"], one["actions"])
    assert np.array_equal(np.vstack([r["rho"] for r in rs]), one["rho"])
    assert _rel(np.vstack([r["W"] for r in rs]), one["W"]) < 1e-9


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_ranks_match_one_hydro_gpu(gpu_lib):
    check_ranks("hydro", gpu_lib, "cuda:0", True)
