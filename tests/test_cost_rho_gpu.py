"""Cost-proportional rho on the HIP kernels: the checks of cost_rho_cases.py
(cases, references, derived bounds) that test_cost_rho.py and
test_gradient_rho.py run on the host emulation."""
import pytest

import cost_rho_cases as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def no_jit(monkeypatch):
    # read at every phx_set_problem: no lane-solver compile for objects that never solve
    monkeypatch.setenv("PHX_NO_JIT", "1")


@pytest.mark.parametrize("case", list(cr.STATS_CASES))
def test_stats_gpu(gpu_lib, no_jit, case):
    cr.check_stats(gpu_lib, DEV, case)


@pytest.mark.parametrize("case", list(cr.SLICE_CASES))
def test_stats_rank_slices_gpu(gpu_lib, no_jit, case):
    cr.check_stats_slices(gpu_lib, DEV, case)


@pytest.mark.parametrize("case", list(cr.APPLY_CASES))
def test_apply_gpu(gpu_lib, no_jit, case):
    cr.check_apply(gpu_lib, DEV, case)


def test_apply_rejects_order_stat_gpu(gpu_lib, no_jit):
    cr.check_apply_rejects_order_stat(gpu_lib, DEV)


@pytest.mark.parametrize("N,S", cr.W_ABSDIFF_CASES)
def test_w_absdiff_gpu(gpu_lib, no_jit, N, S):
    cr.check_w_absdiff(gpu_lib, DEV, N, S)


def test_reference_pins_gpu(gpu_lib, tmp_path):
    cr.check_reference_pins(gpu_lib, DEV, tmp_path)


def test_multistage_gpu(gpu_lib):
    cr.check_multistage(gpu_lib, DEV)


@pytest.mark.parametrize("case", list(cr.E2E_CASES))
def test_end_to_end_gpu(gpu_lib, case):
    cr.check_end_to_end(gpu_lib, DEV, case)
