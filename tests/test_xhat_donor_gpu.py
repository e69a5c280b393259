"""Scenario-donor xhat inner bounds on the GPU: the phx_donor_gather /
phx_fix_nonants kernels against the numpy restatement, and XhatBase._try_one on
the fixed-nonant lane module against the oracle's fixed-xhat evaluation --
every fixed solve certified by the lane kernels alone (lane_certified == S, no
stragglers), which the generic path of an explicit phx_set_bounds never is.
One context per model (module-scoped): the second module's hipRTC build is the
expensive part."""
import numpy as np
import pytest

import xhat_cases as xc
from helpers import ph_options, rel
from mpisppy_amd.examples import farmer
from mpisppy_amd.extensions.xhatspecific import XhatSpecific
from mpisppy_amd.opt.ph import PH
from oracle import models as om, ph as oph

pytestmark = pytest.mark.gpu

MODELS = {"farmer3": ("farmer", 3), "farmer65": ("farmer", 65), "farmer300": ("farmer", 300),
          "aircond32": ("aircond", (3, 2)), "aircond432": ("aircond", (4, 3, 2))}


@pytest.fixture(scope="module")
def evals(gpu_lib):
    made = {}

    def get(key):
        if key not in made:
            model, size = MODELS[key]
            made[key] = xc.make_eval(gpu_lib, "cuda:0", model, size)[0]
        return made[key]
    return get


@pytest.mark.parametrize("S", xc.S_LIST)
def test_gather_and_fix_farmer_gpu(gpu_lib, S, monkeypatch):
    # (the two kernels alone: no hipRTC build of the fixed module per batch size;
    # test_try_one_lane_gpu runs them with it)
    monkeypatch.setenv("PHX_FIX_LANE", "0")
    ev, _ = xc.make_eval(gpu_lib, "cuda:0", "farmer", S)
    xc.check_gather(ev)
    xc.check_fix(ev)


@pytest.mark.parametrize("bf", [(2, 2), (3, 2)])
def test_gather_and_fix_aircond_gpu(gpu_lib, bf, monkeypatch):
    monkeypatch.setenv("PHX_FIX_LANE", "0")
    ev, _ = xc.make_eval(gpu_lib, "cuda:0", "aircond", bf)
    xc.check_gather(ev)
    xc.check_fix(ev)


def _aircond_donors(bf, picks):
    """One donor per non-leaf node: the picks[t]-th scenario (mod the node's count) of each."""
    from mpisppy_amd.utils import sputils
    S = int(np.prod(bf))
    nl = sputils.nonleaf_tree_nodes(sputils.create_nodenames_from_branching_factors(list(bf)), S)
    out = []
    for p in picks:
        out.append({nd.name: "scen%d" % (nd.scenfirst + p % (nd.scenlast - nd.scenfirst + 1)) for nd in nl.values()})
    return out


@pytest.mark.parametrize("key", list(MODELS))
def test_try_one_lane_gpu(evals, key):
    """Three donors in a row: the first fixed solve is cold, the next two start
    from the previous candidate's active set; then the bounds are restored and
    a plain solve is the pre-trial one again, lane-certified."""
    model, size = MODELS[key]
    ev = evals(key)
    assert "on" == ev._native.jit_info(ev._ctx).decode()[:2]
    ev.solve_loop()
    before = ev.nonant_values().copy()
    st = xc.last_stats(ev)
    assert st.lane_certified == ev._S and st.jit == 1
    if model == "farmer":
        S = size
        donors = [{"ROOT": "scen%d" % k} for k in (S - 1, 0, S // 2)]
        sample = None if S <= 65 else [0, 1, 64, 65, 128, 255, 256, S - 1]
    else:
        donors = _aircond_donors(size, (1, 0, 2))
        sample = None
    xc.check_try_one(ev, model, size, donors, lane=True, sample=sample)
    assert "fixed-nonant lane module on" in ev._native.jit_info(ev._ctx).decode()
    xc.check_restored_solve(ev, before, lane=True)


def test_try_one_infeasible_gpu(gpu_lib):
    ev, _ = xc.make_eval(gpu_lib, "cuda:0", "farmer", 3)
    xc.check_infeasible(ev)


def test_ph_device_loop_then_xhatspecific_gpu(gpu_lib):
    """PH on the device loop with an XhatSpecific extension (it acts after the
    loop): the trial runs on the fixed module, and a further solve with the
    bounds restored reproduces the last PH solve's x -- the PH module's active
    sets were not touched by the trial."""
    S = 300
    names = farmer.scenario_names_creator(S)
    opts = ph_options(6)
    opts["xhat_specific_options"] = {"xhat_scenario_dict": {"ROOT": "scen123"}, "xhat_solver_options": {},
                                     "keep_solution": False}
    ph = PH(opts, names, farmer.scenario_creator, scenario_creator_kwargs={"num_scens": S}, extensions=XhatSpecific,
            _native_lib=gpu_lib, _device="cuda:0")
    ph.ph_main()
    assert hasattr(ph, "iterk_stats") and ph.iterk_stats["iters"] == 6       # the device loop ran
    assert "fixed-nonant lane module on" in gpu_lib.jit_info(ph._ctx).decode()
    last_x = ph.nonant_cache.copy()          # saved by post_everything before the trial: the last PH solve's
    scens = [om.farmer(n, num_scens=S) for n in names]
    E, _, ok = oph.evaluate_xhat(scens, {"ROOT": last_x[123]})
    assert ok.all() and rel(ph.extobject._xhat_specific_obj_final, E) < 1e-9
    assert np.array_equal(ph.nonant_values(), last_x) and not ph._fixed.any()
    ph.solve_loop(solver_options=ph.current_solver_options)
    assert rel(ph.nonant_values(), last_x) < 1e-9
    st = xc.last_stats(ph)
    assert st.lane_certified == S and st.stragglers == 0
