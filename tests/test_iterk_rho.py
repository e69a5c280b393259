"""NormRhoUpdater inside the device loop (phx_iterk_norm_rho), on the host
emulation: the sequential restatement of the loop (tests/emu/phx_emu_iterk_rho.cpp)
against the host loop, bit for bit (iterk_rho_cases.py), and the ABI additions."""
import ctypes
import os
import subprocess

import pytest

import iterk_rho_cases as ic
from mpisppy_amd import _native
from test_norm_rho import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_parity_through_the_device_loop_emu(emu, case):
    ic.check_oracle_parity(case, emu, "cpu")


@pytest.mark.parametrize("S", ic.SIZE_EDGES)
def test_size_edges_emu(emu, S):
    ic.check_size_edge(emu, "cpu", S)


def test_convthresh_stop_runs_its_own_update_emu(emu):
    ic.check_convthresh_stop(emu, "cpu")


@pytest.mark.parametrize("so", ic.STRAGGLERS)
def test_straggler_stops_emu(emu, so):
    ic.check_straggler_stops(emu, "cpu", so)          # (the stop count: GPU test)


@pytest.mark.parametrize("extra", [None, {"ipm_max_it": 2}])
def test_straggler_stops_workgroup_emu(emu, extra):
    ic.check_straggler_stops_wg(emu, "cpu", 20, extra)


@pytest.mark.parametrize("nro", [{"rho_update_stop_iterations": 5}, {"iterations_converged_before_decrease": 6}])
def test_options_emu(emu, nro):
    a, b = ic.check_option(emu, "cpu", nro)
    if "rho_update_stop_iterations" in nro:
        assert a.iterk_stats["rho_updates"] == 4                   # iterations 2..5
    else:
        rows = ic.update_rows(a, 11)
        assert not (rows[:4] == 2).any() and (rows == 2).any()      # no decrease before iteration 6, some after


def test_verbose_and_subclasses_keep_the_host_loop_emu(emu):
    ic.check_keeps_host_loop(emu, "cpu")


def test_iteration_limits_0_and_1_emu(emu):
    ic.check_iteration_limits(emu, "cpu")


def test_iterk_rho_layout_matches_header(tmp_path):
    """The ctypes mirror of phx_iterk_rho against the header, by a compiled probe (as test_abi_layout.py)."""
    cls, cname = _native.IterkRho, "phx_iterk_rho"
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
