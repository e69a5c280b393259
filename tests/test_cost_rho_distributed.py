"""Gradient_extension on several ranks: the candidate statistics are SUM- and
MAX-all-reduced (entries of nodes a rank does not hold travel as 0, 0, -inf,
-inf), the W difference is a mean of the ranks' means, every rank applies the
same per-entry rho to its own scenarios, and the run must match one process:
the same firing iterations, rho to rel 1e-12, x-bar and W to rounding (the
ranks' sums add in another fixed order than one process's tiles).

gloo on the host emulation: farmer with 6 scenarios on 2 ranks, and hydro (9
scenarios, three stages) on 3 ranks, where no rank holds a scenario of every
tree node.  One gpu case: hydro on 3 processes, each with its own context on
cuda:0, over gloo with the host loop.  Every child runs under a time limit of
its own, and after a failed child nothing further is started.
"""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"farmer": (2, 20), "hydro": (3, 20)}       # world size, PH iterations
CHILD_LIMIT_S = 240.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_case(case, lib, device, mpicomm=None, conv_ranks=None):
    import cost_rho_cases as cr
    world, iters = CASES[case]
    opts = cr.gradient_options()
    if conv_ranks:
        opts["conv_ranks"] = conv_ranks
    if case == "farmer":
        ph = cr.farmer_ph(lib, device, S=6, iters=iters, options=opts, extensions=cr.RecordingGradient,
                          mpicomm=mpicomm)
    else:
        # (hydro's own gradient cost is 0 for every nonant: cost_rho_cases.SyntheticCostGradient)
        ph = cr.hydro_ph(lib, device, iters=iters, options=opts, extensions=cr.SyntheticCostGradient,
                         mpicomm=mpicomm)
    conv, Eobj, tb = ph.ph_main()
    ext = ph.extobject
    present = np.zeros(ph.NNS, dtype=bool)
    present[np.unique(ph._xbar_idx)] = True
    return {"conv": conv, "iters": ph._PHIter, "W": ph.W_array(), "rho": ph._host("rho").T.copy(),
            "xbar": {k: v[0] for k, v in ph.xbar_by_node().items()},
            "fired": [f[0] for f in ext.fired], "rho_node": [f[1] for f in ext.fired],
            "kept": int(sum(f[2].sum() for f in ext.fired)), "dual": list(ext.dual_conv_cache),
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
    # (an exception ends this rank at once: the parent then stops its peers)
    out[rank] = _run_case(case, lib, device, mpicomm=Comm())
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, args):
    """The ranks as spawned children, each under CHILD_LIMIT_S: a child that fails
    raises here (its peers are stopped), one past its limit is killed with them."""
    ctx = mp.spawn(_worker, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_LIMIT_S
    while not ctx.join(timeout=5.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            for p in ctx.processes:
                p.join()
            pytest.fail("a rank ran past its %.0f s limit" % CHILD_LIMIT_S)


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def check_ranks(case, lib, device, gpu):
    world, iters = CASES[case]
    # (a spawned manager: a parent holding a GPU context must not be forked)
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    _spawn(world, (world, _free_port(), out, case, gpu))
    rs = [out[r] for r in range(world)]
    one = _run_case(case, lib, device, conv_ranks=world)
    assert one["present"].all() and one["iters"] == iters and one["kept"] == 0
    assert len(one["fired"]) >= 1 and len(one["fired"]) < iters - 1, one["fired"]
    covered = np.zeros_like(one["present"])
    for r in rs:
        assert r["iters"] == iters and r["not_optimal"] == 0 and r["kept"] == 0
        if case == "hydro":
            assert not r["present"].all()                    # no rank covers every node
        assert r["fired"] == one["fired"], (r["fired"], one["fired"])
        for a, b in zip(r["rho_node"], one["rho_node"]):
            assert np.max(np.abs(a - b) / np.abs(b)) < 1e-12
        covered |= r["present"]
        assert _rel(r["dual"], one["dual"]) < 1e-9
        assert _rel(r["conv"], one["conv"]) < 1e-9
        for k, v in one["xbar"].items():
            assert _rel(r["xbar"][k], v) < 1e-9, k
    assert covered.all()
    rho = np.vstack([r["rho"] for r in rs])
    assert np.max(np.abs(rho - one["rho"]) / np.abs(one["rho"])) < 1e-12
    assert not np.all(one["rho"] == 1.0)
    assert _rel(np.vstack([r["W"] for r in rs]), one["W"]) < 1e-9


@pytest.mark.parametrize("case", list(CASES))
def test_ranks_match_one_emu(emu, case):
    check_ranks(case, emu, "cpu", False)


@pytest.mark.gpu
def test_ranks_match_one_hydro_gpu(gpu_lib):
    check_ranks("hydro", gpu_lib, "cuda:0", True)
