"""The Fixer on the GPU: the phx_fixer_step and phx_fix_nonants_where kernels
against the numpy restatement, the fixed-subset lane module (a forced fix of
one slot: every following solve certified by the lane kernels alone, equal to
the generic path's answer, and the PH module's active sets untouched by it),
and the farmer-3 run against the oracle subclass.  fixer_cases.py holds the
shared cases."""
import numpy as np
import pytest
import torch

import fixer_cases as fc
from helpers import rel

pytestmark = pytest.mark.gpu

GPU = torch.device("cuda:0")


def test_decisions_gpu(gpu_lib):
    ph = fc.make_ph(gpu_lib, GPU, "farmer", 3, 1)
    fc.check_decisions(gpu_lib, ph._ctx, GPU)


@pytest.mark.parametrize("S", fc.S_LIST)
def test_bound_write_farmer_gpu(gpu_lib, S, monkeypatch):
    # (the kernel alone at most sizes: no hipRTC build of a subset module per batch
    # size; at 65 the following solve runs on the module)
    if S != 65:
        monkeypatch.setenv("PHX_FIX_LANE", "0")
    fc.check_bound_write(fc.make_ph(gpu_lib, GPU, "farmer", S, 1), lane=S == 65)


@pytest.mark.parametrize("bf", [(2, 2), (3, 2)])
def test_bound_write_aircond_gpu(gpu_lib, bf):
    # different slots fixed in different nodes: no subset module, the generic path
    fc.check_bound_write(fc.make_ph(gpu_lib, GPU, "aircond", bf, 1), lane=True)


def _forced_fix_run(gpu_lib, S):
    """Iter0, one x-bar / W update, slot 2 fixed at its x-bar, then two PH
    solves with an x-bar / W update between them; then the bounds restored and
    one more solve.  Returns what the solves gave."""
    ph = fc.make_ph(gpu_lib, GPU, "farmer", S, 5)
    ph.PH_Prep()
    ph.Iter0()
    ph.Compute_Xbar(False)
    ph.Update_W(False)
    fixed = torch.tensor([0, 0, 1], dtype=torch.int32, device=GPU)
    vals = ph._xbar_node[:3].clone()
    ph._fix_where_device(fixed, vals)
    info = gpu_lib.jit_info(ph._ctx).decode()
    out = {"info": info, "x": [], "obj": [], "stats": []}
    for _ in range(2):
        ph.solve_loop(solver_options=ph.current_solver_options)
        ph._settle()
        out["x"].append(ph._host("x").copy())
        out["obj"].append(ph._obj.cpu().numpy().copy())
        out["stats"].append(dict(ph.solve_stats[-1]))
        ph.Compute_Xbar(False)
        ph.Update_W(False)
    assert (out["x"][-1][ph.batch.nonant.slot_col[2]] == float(vals[2])).all()
    gpu_lib.check(ph._ctx, gpu_lib.fix_nonants_where(ph._ctx, None, None, None, None, None, ph._stream()),
                  "fix_nonants_where")
    ph._fixed[:] = False
    ph._fix_dev = None
    ph.solve_loop(solver_options=ph.current_solver_options)
    ph._settle()
    out["restored"] = dict(ph.solve_stats[-1])
    out["x"].append(ph._host("x").copy())
    return out


@pytest.mark.parametrize("S", [30, 1025])
def test_forced_fix_runs_on_subset_module_gpu(gpu_lib, S, monkeypatch):
    lane = _forced_fix_run(gpu_lib, S)
    print(lane["info"])
    assert "fixed-subset lane module on (1 of 3 slots)" in lane["info"]
    for st in lane["stats"]:
        print({k: st[k] for k in ("lane_certified", "stragglers", "not_optimal", "lane_ms", "lane_warm_ms")})
        assert st["lane_certified"] == S and st["stragglers"] == 0 and st["not_optimal"] == 0
    # back on the PH module and its own active sets
    assert lane["restored"]["lane_certified"] == S and lane["restored"]["stragglers"] == 0
    assert lane["restored"]["not_optimal"] == 0
    monkeypatch.setenv("PHX_FIX_LANE", "0")
    gen = _forced_fix_run(gpu_lib, S)
    assert "fixed-subset lane module off: PHX_FIX_LANE=0" in gen["info"]
    assert gen["stats"][0]["lane_certified"] == 0
    for a, b in zip(lane["x"], gen["x"]):
        assert rel(a, b) < 1e-9
    for a, b in zip(lane["obj"], gen["obj"]):
        assert rel(a, b) < 1e-9


def test_farmer3_with_fixer_matches_oracle_gpu(gpu_lib):
    o = fc.run_oracle("farmer", 3, 2.2, 3, 25)
    fc.check_oracle_case(o)
    ph = fc.run_engine_case(gpu_lib, GPU, "farmer", 3, 2.2, 3, 25)
    fc.compare_with_oracle(ph, o)
    info = gpu_lib.jit_info(ph._ctx).decode()
    print(info)
    assert "fixed-subset lane module on (3 of 3 slots)" in info
    assert all(s["not_optimal"] == 0 for s in ph.solve_stats)
    # the solves after the fixes ran on a subset module: no generic-path lanes
    assert ph.solve_stats[-1]["lane_certified"] == 3 and ph.solve_stats[-1]["stragglers"] == 0
