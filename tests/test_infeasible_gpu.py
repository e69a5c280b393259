"""Infeasible and unbounded subproblems on the real kernels (infeasible_cases.py; the
emulation: test_infeasible.py), one test per tier so that a failure names it.

The sparse solver's Farkas test (sp_farkas: three workgroup reductions through LDS,
the verdict uniform over 256 threads) runs serially on the emulation; on a
sparse-solver context (n30_m25, n65_m6) every status 4 here comes from it, since the
dense interior-point workspace is not allocated there.  On the lane-size contexts the
certificates come from farkas_lane in k_ipm, after the fixed-nonant lane module let
the lane fall through: a lane that module certifies on an infeasible pair is the false
OPTIMAL.  Each lane structure costs its PH module and its fixed module in hipRTC."""
import pytest

import infeasible_cases as ic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ic.LANE_CASES)
def test_ladder_lane_gpu(gpu_lib, monkeypatch, case):
    """The fixed-nonant lane module with the generic path behind it."""
    ic.check_ladder(gpu_lib, "cuda:0", case, monkeypatch, lane=True)


def test_ladder_lane_weighted_gpu(gpu_lib, monkeypatch):
    ic.check_ladder(gpu_lib, "cuda:0", "vary_all", monkeypatch, weights=True, lane=True)


def test_ladder_sparse_behind_workgroup_gpu(gpu_lib, monkeypatch):
    ic.check_ladder(gpu_lib, "cuda:0", "n30_m25", monkeypatch)


def test_ladder_sparse_alone_gpu(gpu_lib, monkeypatch):
    ic.check_ladder(gpu_lib, "cuda:0", "n30_m25/no_wg", monkeypatch)


def test_ladder_workgroup_gpu(gpu_lib, monkeypatch):
    ic.check_ladder(gpu_lib, "cuda:0", "n65_m6", monkeypatch)


def test_ladder_pdhg_ipm_gpu(gpu_lib, monkeypatch):
    """PDHG, polish and k_ipm: the lane solver off."""
    ic.check_ladder(gpu_lib, "cuda:0", "vary_all/no_jit", monkeypatch)


@pytest.mark.parametrize("case", sorted(ic.BROKEN))
def test_broken_iter0_gpu(gpu_lib, case):
    ic.check_broken_iter0(gpu_lib, None, case)


@pytest.mark.parametrize("case", ["vary_all", "n65_m6", "n30_m25/no_wg", "vary_all/shifted"])
def test_broken_ph_main_gpu(gpu_lib, case):
    """Lane mode, workgroup mode and sparse mode of the device loop, and lane mode with
    every broken scenario proven infeasible."""
    ic.check_broken_ph_main(gpu_lib, None, case, adopts=case.startswith("vary_all"))
