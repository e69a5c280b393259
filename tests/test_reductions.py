"""PH's cross-scenario reductions, each fed chosen inputs at the sizes where
phx_xbar / phx_update_w / phx_expect change kernels and compared with a
high-precision sum (reduction_cases.py: cases, reference, derived bounds).
Every check runs on the host emulation (the harness and the reference) and,
marked gpu, on the HIP kernels."""
import pytest

import reduction_cases as rc


@pytest.fixture(autouse=True)
def _no_jit(monkeypatch):
    # read at every phx_set_problem: no lane-solver compile for objects that never solve
    monkeypatch.setenv("PHX_NO_JIT", "1")


@pytest.mark.parametrize("case", list(rc.XBAR_CASES))
def test_xbar_emu(emu, case):
    rc.check_xbar(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rc.XBAR_CASES))
def test_xbar_gpu(gpu_lib, case):
    rc.check_xbar(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("case", list(rc.SLICE_CASES))
def test_xbar_rank_slices_emu(emu, case):
    rc.check_xbar_slices(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rc.SLICE_CASES))
def test_xbar_rank_slices_gpu(gpu_lib, case):
    rc.check_xbar_slices(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("case", list(rc.UW_CASES))
def test_update_w_emu(emu, case):
    rc.check_update_w(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rc.UW_CASES))
def test_update_w_gpu(gpu_lib, case):
    rc.check_update_w(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("case", list(rc.UW_DIRECT_CASES))
def test_update_w_direct_emu(emu, case):
    rc.check_update_w_direct(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rc.UW_DIRECT_CASES))
def test_update_w_direct_gpu(gpu_lib, case):
    rc.check_update_w_direct(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("S", rc.EXPECT_SIZES)
def test_expect_emu(emu, S):
    rc.check_expect(emu, "cpu", S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", rc.EXPECT_SIZES)
def test_expect_gpu(gpu_lib, S):
    rc.check_expect(gpu_lib, "cuda:0", S)
