"""NormRhoUpdater inside the device loop (phx_iterk_norm_rho) on the MI355X:
the gated absdev / rule / scale kernels of phx_reduce.h in the pipelined loop
against the host loop with the same update, bit for bit (iterk_rho_cases.py)."""
import pytest

import iterk_rho_cases as ic
from test_norm_rho import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_parity_through_the_device_loop_gpu(gpu_lib, case):
    """farmer 3: the one-block k_small_xw / k_absdev_small_rho path; hydro 9: three stages, NNS > N"""
    ic.check_oracle_parity(case, gpu_lib, None)


@pytest.mark.parametrize("S", ic.SIZE_EDGES)
def test_size_edges_gpu(gpu_lib, S):
    ic.check_size_edge(gpu_lib, None, S)


def test_convthresh_stop_runs_its_own_update_gpu(gpu_lib):
    ic.check_convthresh_stop(gpu_lib, None)


@pytest.mark.parametrize("so", ic.STRAGGLERS)
def test_straggler_stops_gpu(gpu_lib, so):
    a, b = ic.check_straggler_stops(gpu_lib, None, so)
    assert a.iterk_stats["straggler_stops"] > 0


@pytest.mark.parametrize("extra", [None, {"ipm_max_it": 2}])
def test_straggler_stops_workgroup_gpu(gpu_lib, extra):
    ic.check_straggler_stops_wg(gpu_lib, None, 300, extra)


@pytest.mark.parametrize("nro", [{"rho_update_stop_iterations": 5}, {"iterations_converged_before_decrease": 6}])
def test_options_gpu(gpu_lib, nro):
    ic.check_option(gpu_lib, None, nro)


def test_verbose_and_subclasses_keep_the_host_loop_gpu(gpu_lib):
    ic.check_keeps_host_loop(gpu_lib, None)


def test_iteration_limits_0_and_1_gpu(gpu_lib):
    ic.check_iteration_limits(gpu_lib, None)
