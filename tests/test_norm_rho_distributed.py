"""NormRhoUpdater on several ranks: the per-(node, slot) primal residuals are
all-reduced (one [NNS + 1] buffer per PH iteration), every rank applies the
rule to its own scenarios, and the run must match one process: the same
actions at every iteration, the same rho bit for bit, x-bar and W to rounding
(the ranks' sums add in another fixed order than one process's tiles).

gloo on the host emulation: farmer with 6 scenarios on 2 ranks, and hydro (9
scenarios, three stages) on 3 ranks, where no rank holds a scenario of every
tree node, so the residuals of absent nodes must travel as zeros.  One gpu
case: hydro on 3 processes, each with its own context on cuda:0, over gloo
with the host loop (as test_distributed_gpu.py runs its host-loop cases).
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"farmer": (2, 12), "hydro": (3, 12)}       # world size, PH iterations


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_case(case, lib, device, mpicomm=None, conv_ranks=None):
    from helpers import ph_options
    from mpisppy_amd.examples import farmer, hydro
    from mpisppy_amd.opt.ph import PH
    from mpisppy_amd.utils import sputils
    from test_norm_rho import RecordingUpdater
    world, iters = CASES[case]
    opts = ph_options(iters, 1.0)
    opts.update({"iter0_solver_options": {"native_loop": 0}, "iterk_solver_options": {"native_loop": 0},
                 "norm_rho_options": {"primal_dual_difference_factor": 10}})
    if conv_ranks:
        opts["conv_ranks"] = conv_ranks
    if case == "farmer":
        ph = PH(opts, farmer.scenario_names_creator(6), farmer.scenario_creator,
                scenario_creator_kwargs={"num_scens": 6}, extensions=RecordingUpdater, mpicomm=mpicomm,
                _native_lib=lib, _device=device)
    else:
        ph = PH(opts, hydro.scenario_names_creator(9), hydro.scenario_creator,
                scenario_creator_kwargs={"branching_factors": [3, 3]},
                all_nodenames=sputils.create_nodenames_from_branching_factors([3, 3]),
                extensions=RecordingUpdater, mpicomm=mpicomm, _native_lib=lib, _device=device)
    conv, Eobj, tb = ph.ph_main()
    present = np.zeros(ph.NNS, dtype=bool)
    present[np.unique(ph._xbar_idx)] = True
    return {"conv": conv, "iters": ph._PHIter, "W": ph.W_array(), "rho": ph._host("rho").T.copy(),
            "xbar": {k: v[0] for k, v in ph.xbar_by_node().items()}, "actions": np.array(ph.extobject.seen),
            "present": present, "not_optimal": sum(s["not_optimal"] for s in ph.solve_stats)}


def _worker(rank, world, port, out, case, gpu):
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
    out[rank] = _run_case(case, lib, device, mpicomm=Comm())
    dist.barrier()
    dist.destroy_process_group()


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def check_ranks(case, lib, device, gpu):
    world, iters = CASES[case]
    # (a spawned manager: a parent holding a GPU context must not be forked)
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out, case, gpu), nprocs=world, join=True)
    rs = [out[r] for r in range(world)]
    one = _run_case(case, lib, device, conv_ranks=world)
    assert one["present"].all() and one["actions"].shape == (iters - 1, len(one["present"]))
    assert len(set(one["actions"].ravel())) >= 3             # several kinds of action (and none) occurred
    covered = np.zeros_like(one["present"])
    for r in rs:
        assert r["iters"] == one["iters"] == iters and r["not_optimal"] == 0
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


@pytest.mark.parametrize("case", list(CASES))
def test_ranks_match_one_emu(emu, case):
    check_ranks(case, emu, "cpu", False)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_ranks_match_one_hydro_gpu(gpu_lib):
    check_ranks("hydro", gpu_lib, "cuda:0", True)
