"""The Fixer extension on the ABI emulation: phx_fixer_step against a numpy
restatement of the two rules, phx_fix_nonants_where's bound write, PH end to
end against an oracle subclass that applies the same rules (one and two gloo
ranks), the options / warnings / errors of the extension, the sslp example's
id_fix_list_fct, and an offline gfx950 compile of the fixed-subset lane module's
source.  fixer_cases.py holds the shared cases and says how the thresholds of
the end-to-end cases were chosen."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fixer_cases as fc
from helpers import ph_options
from mpisppy_amd.examples import farmer, sslp
from mpisppy_amd.extensions.fixer import Fixer, Fixer_tuple
from mpisppy_amd.opt.ph import PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")

# (model, size, th, nb, PH iteration limit)
CASES = {"farmer3": ("farmer", 3, 2.2, 3, 25),
         "farmer30": ("farmer", 30, fc.FARMER30_TH, 3, 40),
         "aircond22": ("aircond", (2, 2), fc.AIRCOND_TH, fc.AIRCOND_NB, 30)}
_ORACLE = {}


def oracle_run(case):
    """The oracle's run of a case, computed once and shared (never modified)."""
    if case not in _ORACLE:
        _ORACLE[case] = fc.run_oracle(*CASES[case])
    return _ORACLE[case]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------- the two entry points
def test_symbols_exported(emu):
    for name in ("fixer_step", "fix_nonants_where"):
        assert hasattr(emu.lib, "emu_phx_" + name)
    assert hasattr(emu.lib, "emu_phx_subset_lane_source")


def test_decisions_emu(emu):
    ph = fc.make_ph(emu, CPU, "farmer", 3, 1)
    fc.check_decisions(emu, ph._ctx, CPU)


@pytest.mark.parametrize("S", fc.S_LIST)
def test_bound_write_farmer_emu(emu, S):
    fc.check_bound_write(fc.make_ph(emu, CPU, "farmer", S, 1))


@pytest.mark.parametrize("bf", [(2, 2), (3, 2)])
def test_bound_write_aircond_emu(emu, bf):
    fc.check_bound_write(fc.make_ph(emu, CPU, "aircond", bf, 1))


def test_where_errors_emu(emu):
    ph = fc.make_ph(emu, CPU, "farmer", 3, 1)
    ph.PH_Prep(attach_prox=False)
    ph.Iter0()
    ph._settle()
    v = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(Exception, match="node_fixed and xbar_idx required"):
        emu.check(ph._ctx, emu.fix_nonants_where(ph._ctx, v.data_ptr(), None, None, None, None, None), "where")
    ph._bundles = object()
    with pytest.raises(NotImplementedError):
        ph._fix_where_device(torch.zeros(3, dtype=torch.int32), v)


# ---------------------------------------------------------------- PH against the oracle
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_case_is_decisive(case):
    """On the oracle run alone: no sd within 1 % of th, and something is fixed."""
    o = oracle_run(case)
    fc.check_oracle_case(o)
    if case == "farmer3":
        # the issue's run
        assert [(e[0], e[2]) for e in o.events] == [(15, 2), (19, 0), (19, 1)] and o.last_iter == 20
        assert np.allclose([e[4] for e in o.events], [174.2070, 78.1786, 247.6144], atol=5e-5)
    if case == "aircond22":
        its = {}
        for e in o.events:
            its.setdefault(e[1], set()).add(e[0])
        assert len(set(min(v) for v in its.values())) >= 2       # nodes that fix at different iterations


@pytest.mark.parametrize("case", list(CASES))
def test_ph_with_fixer_matches_oracle_emu(emu, case):
    model, size, th, nb, iters = CASES[case]
    o = oracle_run(case)
    fc.check_oracle_case(o)
    ph = fc.run_engine_case(emu, CPU, model, size, th, nb, iters)
    fc.compare_with_oracle(ph, o)
    # the host's fixedness follows the device's flags
    how = ph.extobject._fixed.numpy()
    assert np.array_equal(ph._fixed, (how[ph._xbar_idx] != 0).T)
    assert ph.extobject.fixed_so_far == len(o.events)


def _worker2(rank, world, port, out, case):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.comm import Comm
    emu = _native.Lib(os.path.join(ROOT, "tests", "emu", "libphx_emu.so"), prefix="emu_phx_")
    model, size, th, nb, iters = CASES[case]
    ph = fc.run_engine_case(emu, CPU, model, size, th, nb, iters, mpicomm=Comm())
    out[rank] = (fc.engine_events(ph), ph._PHIter, ph._host("xbar").copy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["farmer3", "farmer30"])
def test_fixer_two_ranks(emu, case):
    """Two gloo ranks take the same decisions (no collective in the step: its
    inputs are all-reduced) and the same as one rank."""
    model, size, th, nb, iters = CASES[case]
    one = fc.run_engine_case(emu, CPU, model, size, th, nb, iters)
    ev1 = fc.engine_events(one)
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker2, args=(2, _free_port(), out, case), nprocs=2, join=True)
    o = oracle_run(case)
    assert [e[:4] for e in ev1] == [e[:4] for e in sorted(o.events)]
    for r in range(2):
        ev, its, xbar = out[r]
        assert [e[:4] for e in ev] == [e[:4] for e in ev1], r
        assert np.allclose([e[4] for e in ev], [e[4] for e in ev1], rtol=1e-9, atol=0)
        assert its == one._PHIter
    assert out[0][0] == out[1][0]          # identical on both ranks, value bits included


# ---------------------------------------------------------------- the extension's surface
def _farmer_ph(emu, fct, S=3, iters=3, per_scenario=False, **fo):
    opts = ph_options(iters, 1.0, 1e-8)
    opts["fixeroptions"] = dict({"verbose": False, "boundtol": 1e-2, "id_fix_list_fct": fct}, **fo)
    if per_scenario:
        opts["per_scenario_models"] = True
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator,
              scenario_creator_kwargs={"num_scens": S}, extensions=Fixer, _native_lib=emu, _device=CPU)


def test_fixer_tuple_warnings(capsys):
    class V:
        name = "x[1]"
    v = V()
    assert Fixer_tuple(v, th=0.5, nb=3) == (id(v), 0.5, 3, None, None)
    assert Fixer_tuple(v, nb=1)[1] == 0
    Fixer_tuple(v)
    assert "but no arguments were given" in capsys.readouterr().out
    Fixer_tuple(v, th=1, nb=1, lb=2)
    assert "with nb < lb, which means lb will be ignored." in capsys.readouterr().out
    Fixer_tuple(v, th=1, nb=1, ub=2)
    assert "with nb < ub, which means ub will be ignored." in capsys.readouterr().out


def test_model_variable_ids_emu(emu):
    """With per-scenario models the tuples carry id(var) of the model's
    variables, as rho_setter lists do; the run is the view-based one."""
    def fct(m):
        return [], [Fixer_tuple(m.DevotedAcreage[c], th=2.2, nb=3) for c in m.DevotedAcreage]
    ph = _farmer_ph(emu, fct, iters=25, per_scenario=True)
    ph.ph_main()
    ref = fc.run_engine_case(emu, CPU, "farmer", 3, 2.2, 3, 25)
    assert fc.engine_events(ph) == fc.engine_events(ref) and len(ph.extobject.events) == 3
    s = ph.local_scenarios[ph.local_scenario_names[0]]
    m = ph._models[ph.local_scenario_names[0]]
    keys = s._keys()
    cols = list(ph.batch.nonant.slot_col)
    for c in m.DevotedAcreage:
        v = m.DevotedAcreage[c]
        assert s._mpisppy_data.varid_to_nonant_index[id(v)] == keys[cols.index(v.index)]
    with pytest.raises(KeyError):
        s._mpisppy_data.varid_to_nonant_index[id(object())]


def test_threshold_variation_errors_emu(emu):
    def fct_k(s):
        th = 1.0 if s.name == "scen0" else 2.0
        return [], [Fixer_tuple(v, th=th, nb=1) for v in s._mpisppy_data.nonant_indices.values()]

    def fct_0(s):
        th = 1.0 if s.name == "scen0" else 2.0
        return [Fixer_tuple(v, th=th, nb=1) for v in s._mpisppy_data.nonant_indices.values()], []
    with pytest.raises(RuntimeError, match="Attempt to vary fixer threshold across scenarios"):
        _farmer_ph(emu, fct_k).ph_main()
    with pytest.raises(RuntimeError, match="Attempt to vary iter0 fixer threshold across scenarios."):
        _farmer_ph(emu, fct_0).ph_main()


def test_missing_lists_warn_emu(emu, capsys):
    ph = _farmer_ph(emu, lambda s: (None, None), iters=3)
    ph.ph_main()
    out = capsys.readouterr().out
    assert "WARNING: No Iter0 fixer tuple for s.name= scen0" in out
    assert "MAJOR WARNING: No Iter k fixer tuple for s.name= scen0" in out
    assert ph.extobject.events == [] and not ph._native_loop_ok()


def test_progress_lines_and_verbose_emu(emu, capsys):
    ph = _farmer_ph(emu, fc.nb_fct(2.2, 3), iters=25, verbose=True)
    ph.ph_main()
    out = capsys.readouterr().out
    assert "(rank0) Unique vars fixed so far - 0 (0 prior to iteration 0)" in out
    assert "(rank0) Unique vars fixed so far - 1 (0 prior to iteration 0)" in out
    assert "(rank0) Unique vars fixed so far - 3 (0 prior to iteration 0)" in out
    assert "(rank0) Fixed nb scen0 DevotedAcreage[WHEAT0] at 174.2069" in out
    assert "(rank0) Fixed nb scen2 DevotedAcreage[SUGAR_BEETS0] at 247.6144" in out
    assert "(rank0) Final unique vars fixed by fixer= 3.0" in out


def test_iter0_rule_and_lb_lag_emu(emu):
    """The iter0 list fixes at iteration 1 (nb: at x-bar when converged); an lb
    lag fixes a nonant whose x-bar sits on its lower bound."""
    def fct(s):
        vs = list(s._mpisppy_data.nonant_indices.values())
        # a huge threshold: every entry is "converged" at once
        return [Fixer_tuple(vs[0], th=1e6, nb=1)], [Fixer_tuple(v, th=1e6, lb=0, ub=0) for v in vs]
    ph = _farmer_ph(emu, fct, iters=4)
    ph.PH_Prep()
    ph.Iter0()
    ph.options["PHIterLimit"] = 1
    ph.iterk_loop()
    ev = ph.extobject.events
    xb0 = ph._host("xbar")[0]
    assert ev == [(1, 0, 1, xb0)]
    assert ph._fixed[:, 0].all() and not ph._fixed[:, 1:].any()
    assert (ph.nonant_values()[:, 0] == xb0).all()


def test_differing_bounds_raise_emu(emu):
    """An lb lag on a column whose lower bound differs within its node."""
    def creator(name, num_scens=None):
        m = farmer.scenario_creator(name, num_scens=num_scens)
        if name == "scen1":
            v = m.DevotedAcreage[list(m.DevotedAcreage)[0]]
            v.lb = 1.0
        return m

    def fct(m):
        return [], [Fixer_tuple(m.DevotedAcreage[c], th=1.0, lb=1) for c in m.DevotedAcreage]
    opts = ph_options(3, 1.0, 1e-8)
    opts["fixeroptions"] = {"verbose": False, "boundtol": 1e-2, "id_fix_list_fct": fct}
    opts["per_scenario_models"] = True
    ph = PH(opts, farmer.scenario_names_creator(3), creator, scenario_creator_kwargs={"num_scens": 3},
            extensions=Fixer, _native_lib=emu, _device=CPU)
    with pytest.raises(ValueError, match="differ between the scenarios of its node"):
        ph.ph_main()


def test_sslp_id_fix_list_fct_emu(emu):
    """The reference's sslp lists (th 0, lb / ub lags of 20 on the facility
    variables): five iterations run and fix nothing ("we don't run long enough")."""
    S = 5
    opts = ph_options(5, 1.0, 1e-8)
    opts["fixeroptions"] = {"verbose": False, "boundtol": 0.01, "id_fix_list_fct": sslp.id_fix_list_fct}
    ph = PH(opts, sslp.scenario_names_creator(S), sslp.scenario_creator,
            scenario_creator_kwargs={"instance": 5, "num_scens": S}, extensions=Fixer, _native_lib=emu, _device=CPU)
    ph.ph_main()
    assert ph._PHIter == 5 and ph.extobject.events == [] and ph.extobject.fixed_so_far == 0
    t0, tk = ph.extobject.iter0_fixer_tuples["Scenario1"], ph.extobject.fixer_tuples["Scenario1"]
    assert t0 is None and len(tk) == 15 and all(t[1:] == (0, None, 20, 20) for t in tk)


# ---------------------------------------------------------------- the subset module's source
def test_mask_structure_helper_under_sanitizers(tmp_path):
    """phx_jit.h's masked fixed_nonant_structure and the source generator in a
    stand-alone program built with AddressSanitizer and UBSan (host code only,
    its own main, run as a process of its own)."""
    import subprocess
    exe = str(tmp_path / "jit_mask_main")
    src = os.path.join(ROOT, "tests", "emu", "jit_mask_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _subset_source(emu, ph, mask, waves=2):
    fn = emu.lib.emu_phx_subset_lane_source
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    return fn(ph._ctx, m.ctypes.data, waves).decode()


def test_subset_source_all_ones_is_fixed_source(emu):
    ph = fc.make_ph(emu, CPU, "farmer", 20, 1)
    fn = emu.lib.emu_phx_fixed_lane_source
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    full = fn(ph._ctx, 2).decode()
    assert _subset_source(emu, ph, [1, 1, 1]) == full and "struct PT" in full
    part = _subset_source(emu, ph, [0, 0, 1])
    assert part != full and "bnd_vary() { return true; }" in part


@pytest.mark.parametrize("case", ["farmer-2", "farmer-01", "farmer-012", "aircond"])
def test_subset_lane_source_compiles_gfx950(emu, case):
    import test_jit_source as tj
    if not os.path.exists(tj._HIPRTC):
        pytest.skip("no hipRTC in this image")
    if case == "aircond":
        ph = fc.make_ph(emu, CPU, "aircond", (4, 3, 2), 1)
        mask = [j % 2 for j in range(ph.batch.nonant.N)]
    else:
        ph = fc.make_ph(emu, CPU, "farmer", 20, 1)
        mask = [int(str(j) in case.split("-")[1]) for j in range(3)]
    src = _subset_source(emu, ph, mask)
    assert "struct PT" in src and "bnd_vary() { return true; }" in src
    rc, log, code = tj.hiprtc_compile(src)
    assert rc == 0, log[-4000:]
    symbols = tj.elf_symbols(code)
    for k in tj.lane_kernels(emu):
        assert k in symbols, k
