"""The PH objective terms (phx_set_ph_terms + phx_objective) at the sizes where
launch_ph_terms changes kernels, and the slot export (phx_export_slots), each fed
chosen inputs and compared with a high-precision host evaluation (glue_cases.py:
creator, cases, reference, derived bound).  Every check runs on the host emulation
(the harness and the reference) and, marked gpu, on the HIP kernels."""
import pytest

import glue_cases as gc


@pytest.fixture(autouse=True)
def _no_jit(monkeypatch):
    # read at every phx_set_problem: no lane-solver compile for objects that never solve
    monkeypatch.setenv("PHX_NO_JIT", "1")


@pytest.mark.parametrize("case", list(gc.OBJ_CASES))
def test_ph_objective_emu(emu, case):
    gc.check_ph_objective(emu, "cpu", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(gc.OBJ_CASES))
def test_ph_objective_gpu(gpu_lib, case):
    gc.check_ph_objective(gpu_lib, "cuda:0", case)


@pytest.mark.parametrize("N,S", gc.EXPORT_SIZES)
def test_export_slots_emu(emu, N, S):
    gc.check_export_slots(emu, "cpu", N, S)


@pytest.mark.gpu
@pytest.mark.parametrize("N,S", gc.EXPORT_SIZES)
def test_export_slots_gpu(gpu_lib, N, S):
    gc.check_export_slots(gpu_lib, "cuda:0", N, S)
