"""The real kernels on synthetic LP structures (synth_cases.py), against the oracle.

The lane solver's kernels are generated per problem structure (csrc/phx_jit.h) and
compiled by hipRTC; the emulation instantiates the same templates with a run-time
pattern, so a wrong ``if constexpr`` branch, literal table or fill pattern shows only
here.  Six structures (n <= 10, m <= 6; each carries several features the example
models lack) are compiled once per process -- the module is cached by source text,
and a family's scenarios do not depend on the batch size -- and every path that
shares a structure runs on that one compile, with the asserts of the CPU tests
(test_synth_structures.py).  The structure at the lane limits is never compiled
in a test (minutes of hipRTC)."""
import time

import numpy as np
import pytest
import torch

import synth_cases as sc
import test_synth_structures as ts
from helpers import all_certified, ph_options, rel
from mpisppy_amd.opt.ph import PH
from oracle import ph as oph

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", sc.GPU_FAMILIES)
def test_structure_paths_gpu(gpu_lib, key):
    """One lane structure, S = 70 (a full and a partial wavefront): the default device
    loop against the oracle and the host recheck of its x, then native_loop 0,
    iterk_fused 0, as_rounds 0, lane_solver 0 and starved lanes (which finish on the
    generic path) against the default trajectory.  The first context pays the
    structure's hipRTC compile; its time is printed, not asserted."""
    fam = ts.family(key, 1)
    t0 = time.perf_counter()
    first = ts.run(gpu_lib, None, fam, 0)[0]
    t1 = time.perf_counter()
    again = ts.run(gpu_lib, None, fam, 0)[0]
    t2 = time.perf_counter()
    info = first._native.jit_info(first._ctx).decode()
    print("%s: %s; first context %.1f s, second %.2f s (the difference: the hipRTC compile)"
          % (key, info, t1 - t0, t2 - t1))
    assert info.startswith("on: register-resident lane solver n=%d m=%d nnz=%d" % (fam.n, fam.m, fam.nnz)), info
    assert first.solve_stats[0]["lane_certified"] == fam.S and again.solve_stats[0]["lane_certified"] == fam.S
    out = ts.check_paths(gpu_lib, None, fam)
    ts.host_recheck(out["default"][0], fam)
    for name in ("host_loop", "ipm", "starved"):
        ts.host_recheck(out[name][0], fam)
    solve_s = [s["wall_s"] for s in out["host_loop"][0].solve_stats]
    print("%s: host-loop solves %s s" % (key, ["%.4f" % v for v in solve_s]))


def test_seeded_iter0_gpu(gpu_lib, monkeypatch):
    """Iter0 seeded from templates (PHX_FORCE_SEED at S = 192: three wavefronts) and
    unseeded certify every lane at the same objectives, on a structure with varying
    costs, bounds and row sides; both at the oracle's."""
    fam = ts.family("vary_all", 1, S=192)
    runs = []
    for force in (False, True):
        if force:
            monkeypatch.setenv("PHX_FORCE_SEED", "1")
        ph = PH(ph_options(0), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs, _native_lib=gpu_lib)
        conv, Eobj, tb = ph.ph_main()
        assert ph._native.jit_info(ph._ctx).decode().startswith("on")
        runs.append((ph._host("obj").copy(), tb, ph._status.cpu().numpy().copy()))
    (o0, tb0, s0), (o1, tb1, s1) = runs
    assert (s0 == 1).all() and (s1 == 1).all()
    assert rel(o0, o1) < 1e-9
    assert abs(tb0 - tb1) <= 1e-9 * max(1.0, abs(tb0))
    o = ts.oracle_iter0(fam)
    assert rel(o1, o.obj) < 1e-8 and rel(tb1, o.trivial_bound) < 1e-9


def test_fixed_nonant_module_gpu(gpu_lib):
    """phx_fix_nonants on one synthetic structure (fixed + empty + upper-only columns, a
    range row): its fixed-nonant module is a second compile."""
    ts.check_xhat(gpu_lib, "cuda:0", ts.family("fixed_empty_upper", 1), lane=True)


@pytest.mark.parametrize("S", [66000, 197120])
def test_large_batch_gpu(gpu_lib, S):
    """A vectorised batch of one structure through the device loop.  66,000 scenarios
    are 1,032 wavefronts, more than the 1,024 SIMDs: the fused loop's two-waves-per-SIMD
    kernel (phx_lane_warm_fzr2).  197,120 are 3,080, more than three per SIMD, from
    where Iter0 seeds from templates unforced (phx_solve).  Every lane certified, the
    host recheck on all lanes, and 32 scenarios plus the first and the last re-solved
    by the oracle from the engine's W / x-bar (as test_farmer_100k_sampled_oracle)."""
    fam = ts.family("vary_all", 1, S=S)
    t0 = time.perf_counter()
    ph, conv, Eobj, tb = ts.run(gpu_lib, None, fam, 3, creator=fam.batch_creator_fn())
    wall = time.perf_counter() - t0
    assert all_certified(ph)
    assert ph._native.jit_info(ph._ctx).decode().startswith("on")
    assert ph.iterk_stats["fused"] and ph.iterk_stats["iters"] == 3
    print("S = %d: PH x3 in %.2f s wall (device loop %.3f s)" % (S, wall, ph.iterk_stats["wall_s"]))
    ts.host_recheck(ph, fam, exact=False)
    sample = sorted(set(np.random.RandomState(7).randint(0, S, 32).tolist()) | {0, S - 1})
    o = oph.OraclePH(fam.scens(sample), rho=1.0)
    o.W_on = o.prox_on = 1
    o.W[:] = ph.W_array()[sample]
    o.xbar[:] = ph.xbar_by_node()["ROOT"][0][None, :]
    o.solve_loop()
    assert rel(o.xn(), ph.nonant_values()[sample]) < 1e-6
    assert rel(o.obj, ph._host("obj")[sample]) < 1e-8
    assert 0.0 < conv < 1e4 and np.isfinite(Eobj) and np.isfinite(tb)
    del ph
    torch.cuda.empty_cache()


def test_generic_tiers_gpu(gpu_lib, monkeypatch):
    """Beyond the lane limits at (65, 6) and (30, 25), and a small family with the JIT
    off: the default path, wg_warm 0, and PHX_NO_JIT with lane_solver 0, each against
    the oracle.  On the emulation (65, 6) and (30, 25) are served by the workgroup warm
    pass with the sparse solver behind it, by the sparse solver alone under wg_warm 0,
    and the small family by PDHG + polish at Iter0 and the workgroup pass after it
    (PDHG + polish throughout under wg_warm 0); what served them here is printed, and
    each of the three tiers must have certified lanes."""
    ts.check_generic_tiers(gpu_lib, None, monkeypatch)
