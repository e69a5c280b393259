"""The workgroup and generic tiers above 64 active rows (wg_size_cases.py) on the HIP
kernels: the scalar explicit inverse of L (more than 64 active rows), the paired-pivot
Cholesky's two-thread row groups (67 or more), the LDS carve at its limit (m = 134 fits,
135 does not), PDHG + the dense polish factor + k_ipm at m = 120 and 135, and the sparse
solver's separator factor at 42 and 61 rows -- with the assertions of the emulation's
tests (test_wg_sizes.py), the per-tier count among them."""
import pytest

import wg_size_cases as wc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", list(wc.CASES))
def test_wg_size_case_gpu(gpu_lib, key):
    wc.check_case(gpu_lib, None, key, gpu=True)


@pytest.mark.parametrize("key", wc.PATH_CASES)
def test_wg_size_paths_bit_equal_gpu(gpu_lib, monkeypatch, key):
    wc.check_paths(gpu_lib, None, key, monkeypatch, gpu=True)


@pytest.mark.parametrize("key", wc.NO_WG_CASES)
def test_wg_size_sparse_alone_gpu(gpu_lib, key):
    wc.check_no_wg(gpu_lib, None, key)
