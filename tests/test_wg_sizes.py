"""The workgroup and generic tiers above 64 active rows (wg_size_cases.py) through the
ABI emulation.  The emulation runs the workgroup solver serially (one thread, no quads,
no row groups), so it checks the cases, the algorithm at these sizes and the
assertions; the device-only code is reached by test_wg_sizes_gpu.py."""
import pytest

import wg_size_cases as wc


@pytest.mark.parametrize("key", list(wc.CASES))
def test_wg_size_case_emu(emu, key):
    wc.check_case(emu, "cpu", key)


@pytest.mark.parametrize("key", wc.PATH_CASES)
def test_wg_size_paths_bit_equal_emu(emu, monkeypatch, key):
    wc.check_paths(emu, "cpu", key, monkeypatch)


@pytest.mark.parametrize("key", wc.NO_WG_CASES)
def test_wg_size_sparse_alone_emu(emu, key):
    wc.check_no_wg(emu, "cpu", key)
