"""Infeasible and unbounded subproblems on every solver tier, through the ABI emulation
(infeasible_cases.py; the kernels: test_infeasible_gpu.py).  The emulation runs the
sparse solver's Farkas test serially, so a reduction or uniformity fault of sp_farkas
shows only on the kernels; what is checked here is the acceptance rule itself and the
host code around the per-lane verdicts."""
import pytest

import infeasible_cases as ic


@pytest.mark.parametrize("case", sorted(ic.LADDERS))
def test_ladder_oracle(case):
    """The ladders are what the table says, by the oracle alone."""
    key, _, _, steps, counts = ic.LADDERS[case]
    ic.check_ladder_oracle(ic.base_family(key), steps, counts, all_or_nothing=key == "eq_range_free")


@pytest.mark.parametrize("case", sorted(ic.LADDERS))
def test_ladder_emu(emu, monkeypatch, case):
    ic.check_ladder(emu, "cpu", case, monkeypatch)


def test_ladder_weighted_emu(emu, monkeypatch):
    """Under p = 1 / S a wrong lane's probability changes nothing: the default
    vary_all ladder under p_k proportional to 1 + (5k mod 7)."""
    ic.check_ladder(emu, "cpu", "vary_all", monkeypatch, weights=True)


@pytest.mark.parametrize("case", sorted(ic.BROKEN))
def test_broken_iter0_emu(emu, case):
    ic.check_broken_iter0(emu, "cpu", case)


@pytest.mark.parametrize("case", ["vary_all", "n65_m6", "n30_m25/no_wg"])
def test_broken_ph_main_emu(emu, case):
    """Lane mode, workgroup mode and sparse mode of the device loop."""
    ic.check_broken_ph_main(emu, "cpu", case, adopts=case == "vary_all")


def test_proven_infeasible_only_ph_main_emu(emu):
    """Every broken scenario proven infeasible, none merely without a verdict: the
    adopted Iter0 still stops the device loop (it counted its not_optimal lanes alone,
    which leave the proven ones out, and ran every iteration before the checks quit)."""
    ph = ic.check_broken_ph_main(emu, "cpu", "vary_all/shifted", adopts=True)
    assert ph.solve_stats[0]["not_optimal"] == 0 and ph.solve_stats[0]["infeasible"] == 3
