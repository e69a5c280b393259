"""The fused PH loop's fold of the x-bar / convergence partials at its edges (GPU).

On one rank a fused launch (phx_lane.h warm_fused) ends its fold at the shard
level: the last arriver of each of the <= 8 arrival shards stores the shard's
partial, and the blocks of the NEXT launch add the shard partials, in shard
order, at their entry (the tail kernel does it after the last launch).  The
partials are double-buffered by launch parity, because blocks beyond the first
resident wave of a launch start after its early blocks have stored their own.
Several ranks keep the two-level fold (the all-reduce needs the sums in memory
between launches).

farmer, crops_multiplier 1, through phx_iterk in fused mode at the grid sizes
where the fold's arithmetic changes shape:

    S = 64        1 block     one shard
    S = 7*64 + 1  8 blocks    one block per shard, the last one partial
    S = 9*64      9 blocks    the first shard with two blocks
    S = 1,000     16 blocks   a typical small grid
    S = 65,600    1,025 blocks: above one wavefront per SIMD, so the two-wave
                  build (phx_lane_warm_fzr2) runs, with late-starting blocks

Bounds: 1e-9 against the host loop (the fused sums run in another fixed order
than k_xbar's tiles: the bound of the existing fused parity tests,
test_gpu_parity.py); 1e-12 against a math.fsum recheck from the engine's own x
(test_farmer_100k_reductions_recheck's bound); two runs of one case bit for bit.

Iteration 1 after Iter0 runs the unfused body (fresh active sets), iteration 2
is a fused segment's first launch (x-bar from k_xbar), so the shard partials
are first read by iteration 3's launch: the fsum recheck is made on iteration
3's x-bar and conv (from run 2's x), and the runs of 5 iterations read them
three times and end in the tail kernel.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import all_certified, rel, run_engine
from mpisppy_amd.examples import farmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [64, 7 * 64 + 1, 9 * 64, 1000, 65600]
STRAG = {"as_rounds": 1, "ipm_max_it": 3, "rescue_rounds": 1}
_RUNS = {}


def _run(lib, S, K, native, thresh=1e-10, so=None, fresh=False):
    """One PH run, kept as host arrays (shared by the tests; never modified)."""
    key = (S, K, native, thresh, tuple(sorted((so or {}).items())))
    if key in _RUNS and not fresh:
        return _RUNS[key]
    iterk = dict(so or {}, native_loop=native)
    if native:
        iterk["iterk_fused"] = 1
    opts = {"convthresh": thresh, "iter0_solver_options": dict(so or {}), "iterk_solver_options": iterk}
    ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), {"num_scens": S}, K,
                                    lib=lib, options=opts)
    xb, xsq = ph.xbar_by_node()["ROOT"]
    r = dict(S=S, iters=ph._PHIter, conv=conv, Eobj=Eobj, tb=tb, W=ph.W_array(), xn=ph.nonant_values(),
             xb=np.array(xb), xsq=np.array(xsq), pc=ph._prob_coeff.copy(), certified=all_certified(ph),
             seg=ph._seg_sums.cpu().numpy()[:ph._conv_R].copy(), stats=dict(getattr(ph, "iterk_stats", {})),
             jit=ph._native.jit_info(ph._ctx).decode(),
             host_stragglers=sum(s.get("stragglers", 0) for s in ph.solve_stats))
    del ph
    if not fresh:
        _RUNS[key] = r
    return r


def _fused_build_ran(r):
    """The device loop ran fused, on the lane solver's JIT kernels, and the build
    the grid size selects is the intended one: the two-wave build above one
    wavefront per SIMD (the library's rule, phx_kernels.hip fused_kernel; no
    override in the environment), the one-wave build at or below."""
    assert r["stats"]["fused"], r["stats"]
    assert r["jit"].startswith("on"), r["jit"]
    assert "PHX_FZR2" not in os.environ and "PHX_FUSED" not in os.environ
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    blocks = -(-r["S"] // 64)
    assert (blocks > simds) == (r["S"] == 65600), (blocks, simds)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("S", SIZES)
def test_fused_matches_host_loop_gpu(gpu_lib, S, K):
    a, b = _run(gpu_lib, S, K, 1), _run(gpu_lib, S, K, 0)
    _fused_build_ran(a)
    assert not b["stats"]
    assert a["iters"] == b["iters"] == K
    assert a["certified"] and b["certified"]
    d = {k: rel(a[k], b[k]) for k in ("xb", "xsq", "W", "xn", "conv", "Eobj")}
    print("[S=%d K=%d] fused vs host loop, max rel diffs: %s" % (S, K, d))
    for k, v in d.items():
        assert v < 1e-9, (k, d)
    assert a["tb"] == b["tb"]
    # what the tail kernel hands back behind the last launch: the left-over
    # count (the loop finishes what the last launch left, so in the end no lane
    # is without an optimal solve, as on the host loop) and the last test's
    # convergence sums (K = 1 is the unfused body alone: no fused launch, no
    # tail kernel behind one)
    assert a["stats"]["not_optimal"] == 0, a["stats"]
    if K > 1:
        assert rel(a["seg"], b["seg"]) < 1e-9, (a["seg"], b["seg"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_shard_sums_fsum_recheck_gpu(gpu_lib, S):
    """Iteration 3's x-bar, x-squared-bar, W and conv -- the first formed from the
    previous launch's shard partials -- against math.fsum over run 2's x."""
    prev, cur = _run(gpu_lib, S, 2, 1), _run(gpu_lib, S, 3, 1)
    _fused_build_ran(cur)
    x, pc = prev["xn"], cur["pc"]
    N = x.shape[1]
    xb = np.array([math.fsum(pc[j] * x[:, j]) for j in range(N)])
    xsq = np.array([math.fsum(pc[j] * x[:, j] * x[:, j]) for j in range(N)])
    W = prev["W"] + 1.0 * (x - xb[None, :])
    conv = math.fsum(np.abs(x - xb[None, :]).ravel()) / (S * N)
    d = {"xb": rel(cur["xb"], xb), "xsq": rel(cur["xsq"], xsq), "W": rel(cur["W"], W),
         "conv": abs(cur["conv"] - conv) / max(1.0, conv)}
    print("[S=%d] iteration 3 vs math.fsum: %s" % (S, d))
    for k, v in d.items():
        assert v < 1e-12, (k, d)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_two_runs_bit_equal_gpu(gpu_lib, S):
    a, b = _run(gpu_lib, S, 5, 1), _run(gpu_lib, S, 5, 1, fresh=True)
    for k in ("xb", "xsq", "W", "xn", "seg"):
        assert np.array_equal(a[k], b[k]), k
    assert a["conv"] == b["conv"] and a["Eobj"] == b["Eobj"] and a["iters"] == b["iters"]


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [10, 5])
def test_conv_stop_same_iteration_gpu(gpu_lib, limit):
    """A threshold between the host loop's conv of iterations 4 and 5 stops both
    loops at iteration 5 -- decided by launch 6's prologue from launch 5's shard
    partials (limit 10: the stop's sums go to the stage buffer before it is
    published), or by the tail kernel (limit 5: the last enqueued launch)."""
    S = 1000
    c4, c5 = _run(gpu_lib, S, 4, 0)["conv"], _run(gpu_lib, S, 5, 0)["conv"]
    assert c5 < c4
    thresh = 0.5 * (c4 + c5)
    a, b = _run(gpu_lib, S, limit, 1, thresh=thresh), _run(gpu_lib, S, limit, 0, thresh=thresh)
    _fused_build_ran(a)
    assert a["iters"] == b["iters"] == 5
    assert a["stats"]["converged"] and a["stats"]["iters"] == 5
    d = {k: rel(a[k], b[k]) for k in ("xb", "xsq", "W", "conv", "seg")}
    print("[conv stop, limit %d] fused vs host loop: %s" % (limit, d))
    for k, v in d.items():
        assert v < 1e-9, (k, d)
    assert rel(a["conv"], c5) < 1e-9


@pytest.mark.gpu
def test_straggler_stop_resumes_gpu(gpu_lib):
    """Starved lane solves leave lanes behind a fused launch: the next launch's
    prologue reads their count out of the shard partials, stops the pipeline and
    stores the stop's sums; the loop finishes the lanes, restarts (a segment's
    first launch: k_xbar's stage buffer) and matches the host loop."""
    S, K = 2000, 5
    a, b = _run(gpu_lib, S, K, 1, so=STRAG), _run(gpu_lib, S, K, 0, so=STRAG)
    _fused_build_ran(a)
    assert a["stats"]["straggler_stops"] > 0 and a["stats"]["stragglers"] > 0, a["stats"]
    assert a["iters"] == b["iters"] == K
    assert a["certified"] and b["certified"]
    d = {k: rel(a[k], b[k]) for k in ("xb", "xsq", "W", "xn", "conv", "Eobj", "seg")}
    print("[straggler stop] fused vs host loop: %s; stats %s" % (d, a["stats"]))
    for k, v in d.items():
        assert v < 1e-9, (k, d)


def _two_rank_case(lib, device, mpicomm=None, conv_ranks=None):
    S, K = 1000, 6
    opts = {"convthresh": 1e-10, "iterk_solver_options": {"native_loop": 1, "iterk_fused": 1}}
    if conv_ranks:
        opts["conv_ranks"] = conv_ranks
    ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S), {"num_scens": S}, K,
                                    lib=lib, device=device, mpicomm=mpicomm, options=opts)
    return {"conv": conv, "Eobj": Eobj, "W": ph.W_array(), "x": ph.nonant_values(), "iters": ph._PHIter,
            "xbar": np.array(ph.xbar_by_node()["ROOT"][0]), "fused": bool(ph.iterk_stats["fused"]),
            "not_optimal": int(ph.iterk_stats["not_optimal"])}


def _two_rank_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.comm import Comm
    out[rank] = _two_rank_case(_native.load(), "cuda:0", mpicomm=Comm())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_keep_two_level_fold_gpu(gpu_lib):
    """Two ranks (own processes, gloo through the callback): every fused launch's
    stage buffer is all-reduced between launches, so the launch's last block
    must fill it (the two-level fold) -- a rank that left its sums in the shard
    partials would all-reduce a stale buffer.  Against one process with
    conv_ranks = 2 (two segments: the unfused device loop)."""
    from test_distributed_gpu import _free_port
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_two_rank_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    rs = [out[r] for r in range(2)]
    one = _two_rank_case(gpu_lib, "cuda:0", conv_ranks=2)
    for r in rs:
        assert r["fused"] and r["iters"] == one["iters"] == 6 and r["not_optimal"] == 0
        assert rel(r["conv"], one["conv"]) < 1e-9 and rel(r["Eobj"], one["Eobj"]) < 1e-9
        assert rel(r["xbar"], one["xbar"]) < 1e-9
    assert rel(np.vstack([r["W"] for r in rs]), one["W"]) < 1e-9
    assert rel(np.vstack([r["x"] for r in rs]), one["x"]) < 1e-9
