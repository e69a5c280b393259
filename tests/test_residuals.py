"""The adaptive-rho entry points (phx_node_absdev, phx_norm_rho, phx_rho_sums),
each fed chosen inputs at the sizes where it changes kernels and compared with
a high-precision sum or an exact numpy restatement (residual_cases.py: cases,
references, derived bounds).  Every check runs on the host emulation (the
harness and the reference) and, marked gpu, on the HIP kernels."""
import pytest

import residual_cases as rs


@pytest.fixture(autouse=True)
def _no_jit(monkeypatch):
    # read at every phx_set_problem: no lane-solver compile for objects that never solve
    monkeypatch.setenv("PHX_NO_JIT", "1")


@pytest.mark.parametrize("case", list(rs.ABSDEV_CASES))
def test_absdev_emu(emu, case):
    rs.check_absdev(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rs.ABSDEV_CASES))
def test_absdev_gpu(gpu_lib, case):
    rs.check_absdev(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("case", list(rs.SLICE_CASES))
def test_absdev_rank_slices_emu(emu, case):
    rs.check_absdev_slices(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rs.SLICE_CASES))
def test_absdev_rank_slices_gpu(gpu_lib, case):
    rs.check_absdev_slices(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("case", list(rs.NORM_RHO_CASES))
def test_norm_rho_emu(emu, case):
    rs.check_norm_rho(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rs.NORM_RHO_CASES))
def test_norm_rho_gpu(gpu_lib, case):
    rs.check_norm_rho(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("N,S", rs.RHO_SUMS_CASES)
def test_rho_sums_emu(emu, N, S):
    rs.check_rho_sums(emu, "cpu", N, S)


@pytest.mark.gpu
@pytest.mark.parametrize("N,S", rs.RHO_SUMS_CASES)
def test_rho_sums_gpu(gpu_lib, N, S):
    rs.check_rho_sums(gpu_lib, "cuda:0", N, S)
