"""Cost-proportional rho on the host emulation: the three entry points
(phx_cost_rho_stats, phx_cost_rho_apply, phx_w_absdiff) fed chosen inputs at the
sizes where the reduction's dispatch and tiling change, and the multistage and
end-to-end checks of the host layer (cost_rho_cases.py: cases, references,
derived bounds).  test_cost_rho_gpu.py runs the same checks on the HIP kernels."""
import ctypes
import os
import subprocess

import pytest

import cost_rho_cases as cr
from mpisppy_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_jit(monkeypatch):
    # read at every phx_set_problem: no lane-solver compile for objects that never solve
    monkeypatch.setenv("PHX_NO_JIT", "1")


@pytest.mark.parametrize("case", list(cr.STATS_CASES))
def test_stats_emu(emu, case):
    cr.check_stats(emu, "cpu", case)


@pytest.mark.parametrize("case", list(cr.SLICE_CASES))
def test_stats_rank_slices_emu(emu, case):
    cr.check_stats_slices(emu, "cpu", case)


@pytest.mark.parametrize("case", list(cr.APPLY_CASES))
def test_apply_emu(emu, case):
    cr.check_apply(emu, "cpu", case)


def test_apply_rejects_order_stat_emu(emu):
    cr.check_apply_rejects_order_stat(emu, "cpu")


@pytest.mark.parametrize("N,S", cr.W_ABSDIFF_CASES)
def test_w_absdiff_emu(emu, N, S):
    cr.check_w_absdiff(emu, "cpu", N, S)


def test_multistage_emu(emu):
    cr.check_multistage(emu, "cpu")


@pytest.mark.parametrize("case", list(cr.E2E_CASES))
def test_oracle_run_meets_its_conditions(case):
    """the trigger fires and declines at least twice, never within 1e-6 of 0.05, and keeps no entry"""
    cr.oracle_gradient_run(case)


@pytest.mark.parametrize("case", list(cr.E2E_CASES))
def test_end_to_end_emu(emu, case):
    cr.check_end_to_end(emu, "cpu", case)


def test_bundles_refused_emu(emu):
    cr.check_bundles_refused(emu, "cpu")


def test_opts_layout_matches_header(tmp_path):
    """The ctypes mirror of phx_cost_rho_opts against the header, by a compiled probe (as test_abi_layout.py)."""
    cls, cname = _native.CostRhoOpts, "phx_cost_rho_opts"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "phx.h"', "int main(void) {",
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = dict((k, int(v)) for k, v in (ln.split() for ln in out.splitlines()))
    for f in cls._fields_:
        assert getattr(cls, f[0]).offset == c["%s.%s" % (cname, f[0])], f[0]
    assert ctypes.sizeof(cls) == c[cname]
    assert len(c) == 1 + len(cls._fields_)
