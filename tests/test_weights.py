"""Non-uniform probabilities, unequal node probabilities, a rho_setter and
variable_probability through the ABI emulation (weight_cases.py: checks A-D at S = 70
on vary_all, eq_range_free and the three-stage multistage family).  The emulation's
device loop is not fused; the GPU versions are in test_weights_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import synth_cases as sc
import test_distributed_gpu as tdg
import test_synth_structures as ts
import weight_cases as wc


def test_weights_are_closed_forms():
    """The weights are what the module states, sum to one per tree node, do not depend
    on the batch size before normalisation, and a family built without them is the
    family it always was (the same creator output, scenario by scenario)."""
    p = wc.scenario_weights(70)
    assert abs(p.sum() - 1.0) < 1e-14 and np.allclose(p[:7] / p[0], [1, 6, 4, 2, 7, 5, 3], rtol=1e-14)
    assert np.allclose(wc.scenario_weights(1100)[:70] / wc.scenario_weights(1100)[0], p / p[0], rtol=1e-14)
    pt, node = wc.tree_weights((7, 10))
    assert abs(node.sum() - 1.0) < 1e-14 and np.allclose(node / node[0], [1, 4, 2, 5, 3, 1, 4], rtol=1e-14)
    assert np.allclose(pt.reshape(7, 10).sum(axis=1), node, rtol=1e-14) and len(set(pt.tolist())) > 20
    rho = wc.rho_values(70, 3)
    assert rho.min() == 0.125 and rho.max() == 8.0 and rho[4, 2] == 2.0 ** (((12 + 10) % 7) - 3)
    assert len(set(rho[:, 0].tolist())) == 7 and len(set(rho[0].tolist())) == 3
    P = wc.slot_probabilities(70, 3, zero=(5, 1))
    assert P[5, 1] == 0.0 and np.allclose(P.sum(axis=0), 1.0, rtol=1e-14)
    # the plumbing: weights reach the creator, the batch creator and the oracle's scenarios
    cs = wc.case("multistage", "p")
    m = cs.fam.creator("scen23")
    assert m._mpisppy_probability == pt[23] and m._mpisppy_node_list[1].cond_prob == node[2]
    s = cs.fam.scen(23)
    assert s.prob == pt[23] and s.nodes[1][1] == node[2]
    two = wc.case("vary_all", "p")
    assert two.fam.batch_creator_fn().batch_creator(["scen3", "scen69"]).prob == [p[3], p[69]]
    # without weights: bit-identical to a family that was never given any
    plain, again = ts.family("multistage", 1), sc.SynthFamily("multistage", 1)
    assert plain.prob is None and cs.base is plain and cs.fam.A is plain.A
    a, b = plain.creator("scen23"), again.creator("scen23")
    assert a._mpisppy_probability == b._mpisppy_probability == 1.0 / 70
    assert a._mpisppy_node_list[1].cond_prob == b._mpisppy_node_list[1].cond_prob == 1.0 / 7
    assert plain.scen(23).prob == 1.0 / 70 and plain.scen(23).nodes[1][1] == 1.0 / 7


@pytest.mark.parametrize("mode", list(wc.MODES))
@pytest.mark.parametrize("key", wc.FAMILIES)
def test_weighted_oracle_differs_from_uniform(key, mode):
    """Check A (oracle only): every case moves W and x-bar by more than 1e-3."""
    wc.check_not_vacuous(wc.case(key, mode))


@pytest.mark.parametrize("mode", list(wc.MODES))
@pytest.mark.parametrize("key", wc.FAMILIES)
def test_weighted_case_emu(emu, key, mode):
    """Checks B, C and D of one case; which loop ran (the device loop except under
    native_loop 0; Iter0 deferred only without a rho setter)."""
    wc.check_case(emu, "cpu", wc.case(key, mode))


@pytest.mark.parametrize("zero", [None, (5, 1)])
def test_variable_probability_synth_emu(emu, zero):
    wc.check_variable_probability(emu, "cpu", zero=zero)


def _rank_worker(rank, world, port, out, case):
    sys.path.insert(0, tdg.ROOT)
    sys.path.insert(0, os.path.join(tdg.ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.comm import Comm
    import test_distributed_gpu
    lib = _native.Lib(os.path.join(tdg.ROOT, "tests", "emu", "libphx_emu.so"), prefix="emu_phx_")
    out[rank] = test_distributed_gpu._run_case(case, lib, "cpu", mpicomm=Comm())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["weighted-fused", "weighted-unfused"])
def test_weighted_two_ranks_emu(emu, case):
    """The two-rank cases of test_distributed_gpu.py on the emulation (never fused
    there): each rank's rho_setter writes its own slice of rho, the ranks' x-bar sums
    add up under probabilities that sum to one over both ranks only."""
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_rank_worker, args=(2, tdg._free_port(), out, case), nprocs=2, join=True)
    one = tdg._run_case(case, emu, "cpu", conv_ranks=2)
    rs = [out[r] for r in range(2)]
    assert [r["n_local"] for r in rs] == [35, 35] and one["iters"] == 4
    for r in rs:
        assert r["iters"] == one["iters"] and r["stats"]["not_optimal"] == 0
        assert tdg._rel(r["conv"], one["conv"]) < 1e-9 and tdg._rel(r["Eobj"], one["Eobj"]) < 1e-9
        assert r["tb"] == pytest.approx(one["tb"], rel=1e-12)
        assert tdg._rel(r["xbar"]["ROOT"], one["xbar"]["ROOT"]) < 1e-9
    assert tdg._rel(np.vstack([r["W"] for r in rs]), one["W"]) < 1e-9
    assert tdg._rel(np.vstack([r["x"] for r in rs]), one["x"]) < 1e-9


def test_publish_rho_extension_emu(emu):
    """The one-copy rho of the large GPU batch (PublishRho, vectorised batch_creator)
    gives the rho_setter's run bit for bit, on the device loop."""
    cs = wc.case("vary_all", "p_rho")
    a = wc.snapshot(cs, *wc.run(emu, "cpu", cs, 3))
    b = wc.snapshot(cs, *wc.run(emu, "cpu", cs, 3, creator=cs.fam.batch_creator_fn(), extension=True))
    assert a["stats"] is not None and b["stats"] is not None
    wc.check_weights_uploaded(cs, b)
    assert np.array_equal(a["W"], b["W"]) and np.array_equal(a["xn"], b["xn"])
    assert (a["conv"], a["Eobj"], a["tb"]) == (b["conv"], b["Eobj"], b["tb"])
