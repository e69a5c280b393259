"""The host API of cost-proportional rho on the host emulation -- Find_Rho,
Set_Rho, Find_Grad (utils/find_rho.py, utils/gradient.py) -- against the numbers
the reference pins in mpisppy/tests/test_gradient_rho.py, on farmer with three
scenarios and the reference's own cost and rho fixtures (tests/golden/
ref_grad_cost.csv, ref_rho.csv).  The checks live in cost_rho_cases.py;
test_cost_rho_gpu.py runs them on the HIP kernels."""
import os

import numpy as np

import cost_rho_cases as cr
from mpisppy_amd.utils.find_rho import Find_Rho, rho_cfg, cfg_get


def test_reference_pins_emu(emu, tmp_path):
    cr.check_reference_pins(emu, "cpu", tmp_path)


def test_cfg_defaults():
    """missing attributes take the reference's defaults"""
    class Bare:
        pass
    for name, want in (("whatpath", ""), ("rho_file", ""), ("rho_path", ""), ("grad_cost_file", ""),
                       ("grad_rho_file", ""), ("order_stat", -1.0), ("rho_relative_bound", 1e3),
                       ("rho_setter", False)):
        assert cfg_get(Bare(), name) == want and getattr(rho_cfg(), name) == want
    assert rho_cfg(order_stat=0.4).order_stat == 0.4


def test_what_file_is_required(emu):
    ph = cr.farmer_ph(emu, "cpu")
    try:
        Find_Rho(ph, rho_cfg(rho_file="out.csv"))
    except AssertionError as e:
        assert "to compute rhos you have to give the name of a What csv file (using --whatpath)" in str(e)
    else:
        raise RuntimeError("an empty whatpath accepted")
    assert Find_Rho(ph, rho_cfg()).c == {}


def test_device_rule_matches_order_stat_of_lists(emu):
    """compute_rho equals Find_Rho._order_stat applied to the per-scenario lists
    formed on the host, for every branch of the order statistic"""
    ph = cr.farmer_ph(emu, "cpu", S=6)
    ph.ph_main()
    ph.Compute_Xbar()
    what = os.path.join(cr.GOLDEN, "ref_grad_cost.csv")
    s_all = list(ph.local_scenarios.values())
    for alpha in cr.ALPHAS:
        cfg = rho_cfg(whatpath=what, rho_file="x", order_stat=alpha)
        fr = Find_Rho(ph, cfg)
        fr.c = {(s.name, v): fr.c[("scen0", v)] for s in s_all for v in ph.batch.nonant.var_names}
        got = fr.compute_rho()
        denom = [np.max((fr._w_denom(s, "ROOT"), fr._prox_denom(s, "ROOT"))) for s in s_all]
        for j, v in enumerate(ph.batch.nonant.var_names):
            want = fr._order_stat([abs(fr.c[(s.name, v)]) / d for s, d in zip(s_all, denom)])
            assert abs(got[v] - want) <= 1e-12 * abs(want), (alpha, v)
