"""The solver tiers on synthetic LP structures (synth_cases.py) through the ABI
emulation, against the oracle: structures the example models do not reach --
equality and range rows, free / upper-only / fixed / empty columns, varying costs,
bounds and row sides, Cholesky fill, a non-example tree -- at two seeds each, then the
paths that share one structure, the lane solver's dispatch edges, the scenario-donor
xhat and the hipRTC compile of the small families' sources.  The GPU versions of
these checks are in test_synth_structures_gpu.py and use the helpers below."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import synth_cases as sc
import xhat_cases as xc
from helpers import all_certified, kkt_recheck, oracle_continue_from, rel, run_engine
from oracle import ph as oph

SEEDS = (1, 2)
ITERS = 4
LIMIT = sc.sized_family(64, 24, nnz=384)              # every feature at the lane limits
TRAJ_FAMILIES = ["eq_range_free", "fixed_empty_upper", "vary_all", "nvar0", "fill", "multistage", "plain",
                 "c_only", "bnd_only", "limit"]
# the solver options of the paths that share one lane structure
PATHS = {"pdhg": {"lane_solver": 0}, "ipm": {"as_rounds": 0}, "host_loop": {"native_loop": 0},
         "unfused": {"iterk_fused": 0},
         # starved lanes: the interior point cut short, so lanes finish on the generic path
         "starved": {"as_rounds": 0, "ipm_max_it": 2}}

_FAMS, _IT0 = {}, {}


def family(key, seed, S=70):
    """The SynthFamily of a name in synth_cases.FAMILIES ("limit": LIMIT), made once."""
    k = (key if isinstance(key, str) else tuple(sorted((a, str(b)) for a, b in key.items())), seed, S)
    if k not in _FAMS:
        _FAMS[k] = sc.SynthFamily(LIMIT if key == "limit" else key, seed, S=S)
    return _FAMS[k]


def oracle_iter0(fam):
    """The oracle's Iter0 of a family (shared by every test of it; not modified)."""
    if id(fam) not in _IT0:
        o = oph.OraclePH(fam.scens(), rho=1.0)
        o.iter0()
        _IT0[id(fam)] = o
    return _IT0[id(fam)]


def solver(so):
    return {"iter0_solver_options": dict(so or {}), "iterk_solver_options": dict(so or {})}


def run(lib, device, fam, iters, so=None, creator=None):
    return run_engine(creator or fam.creator, fam.names, fam.kwargs, iters, lib=lib, device=device,
                      all_nodenames=fam.nodenames, options=solver(so))


def node_name(fam, k, j):
    return "ROOT" if j < fam.stage_N[0] else "ROOT_%d" % (k // fam.bf[1])


def engine_xbar(ph, fam, ks=None):
    """(S, N) x-bar of every scenario's nodes from the engine's per-node values."""
    xb = ph.xbar_by_node()
    loc = ph.batch.nonant.slot_local
    ks = range(fam.S) if ks is None else ks
    if fam.bf is None:
        return np.tile(xb["ROOT"][0][loc], (len(ks), 1))
    return np.array([[xb[node_name(fam, k, j)][0][loc[j]] for j in range(fam.N)] for k in ks])


def check_vs_oracle(lib, device, fam, so=None, iters=ITERS):
    """Iter0's trivial bound against OraclePH.iter0(), iterations 1..iters against the
    oracle continued from the engine's Iter0 point, every solve certified; the
    project's tolerances (trivial bound 1e-9, E[obj] 1e-8, x-bar 1e-8, W 1e-7, nonants
    1e-6)."""
    ph, conv, Eobj, tb = run(lib, device, fam, iters, so)
    assert all_certified(ph), (ph.solve_stats, getattr(ph, "iterk_stats", None))
    # (a property of the generator: the scenarios disagree, so every iteration ran)
    assert ph._PHIter == iters, (ph._PHIter, conv)
    o0 = oracle_iter0(fam)
    ph0 = run(lib, device, fam, 0, so)[0]
    assert all_certified(ph0)
    oc = oracle_continue_from(ph0, fam.scens(), iters)
    errs = {"tb": rel(tb, o0.trivial_bound), "Eobj": rel(Eobj, oc.Eobjective()),
            "xbar": rel(engine_xbar(ph, fam), oc.xbar), "W": rel(ph.W_array(), oc.W),
            "nonants": rel(ph.nonant_values(), oc.xn()), "conv": rel(conv, oc.conv)}
    print(fam.family, fam.flags["n"], fam.flags["m"], fam.flags["nnz"], so, {k: "%.1e" % v for k, v in errs.items()})
    assert errs["tb"] < 1e-9
    assert errs["Eobj"] < 1e-8
    assert errs["xbar"] < 1e-8
    assert errs["W"] < 1e-7
    assert errs["nonants"] < 1e-6
    return ph, conv, Eobj, tb


def host_recheck(ph, fam, exact=True):
    """The engine's own x, independent of the kernel's certificate, in float64: every
    row and bound of every scenario violated by at most 1e-9 (1 + |bound|) (the
    certificate's tolerance, as oracle/qp.py states it), and the returned objective
    equal to c'x + c0 + W'x_N + sum rho/2 (x_N - x-bar)^2 recomputed from x, W, rho and
    x-bar to 1e-12 relative.  exact: math.fsum per scenario; else vectorised numpy (the
    large batches).  Then the row duals of the same solve (helpers.kkt_recheck)."""
    x = ph._host("x")                                  # (n, S)
    S, N = fam.S, fam.N
    W, rho, xb, obj = ph.W_array(), ph._host("rho").T, engine_xbar(ph, fam), ph._host("obj")
    A, xT = fam.A, x.T
    terms = A * xT[:, fam.colidx]
    if exact:
        act = np.array([[math.fsum(terms[k, fam.rowptr[i]:fam.rowptr[i + 1]]) for i in range(fam.m)]
                        for k in range(S)])
    else:
        act = np.zeros((S, fam.m))
        np.add.at(act.T, fam.rowof, terms.T)
    fin = lambda a: np.where(np.isfinite(a), a, 0.0)
    viol = max(float(np.max((fam.bl - act) / (1.0 + np.abs(fin(fam.bl))))),
               float(np.max((act - fam.bu) / (1.0 + np.abs(fin(fam.bu))))),
               float(np.max((fam.lb - xT) / (1.0 + np.abs(fin(fam.lb))))),
               float(np.max((xT - fam.ub) / (1.0 + np.abs(fin(fam.ub))))))
    xn = xT[:, :N]
    parts = np.concatenate([fam.c * xT, W * xn, 0.5 * rho * (xn - xb) ** 2, np.full((S, 1), fam.c0)], axis=1)
    f = np.array([math.fsum(p) for p in parts]) if exact else parts.sum(axis=1)
    oerr = float(np.max(np.abs(f - obj) / np.maximum(1.0, np.abs(f))))
    print(fam.family, "host recheck: violation %.2e objective %.2e" % (viol, oerr))
    assert viol <= 1e-9
    assert oerr <= 1e-12
    kkt_recheck(ph, tag=fam.family)
    return viol, oerr


def emitted_table(src, name):
    """An integer / bool table of the emitted PT struct, as a list."""
    body = re.search(r" %s\(int k\) \{ constexpr \w+ a\[\] = \{([^}]*)\}" % name, src).group(1)
    return [int(v) for v in body.split(",")]


def lane_source(lib, fam, fixed=False):
    """The lane-kernel source of a family (emulation only: the same phx_jit.h code)."""
    import test_jit_source as tj
    if not fixed:
        return tj.lane_source(lib, fam.creator, fam.names, fam.kwargs, fam.nodenames)
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    ev = Xhat_Eval(xc.xhat_options(), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs,
                   all_nodenames=fam.nodenames, _native_lib=lib, _device="cpu")
    fn = lib.lib.emu_phx_fixed_lane_source
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return fn(ev._ctx, 2).decode()


# ---------------------------------------------------------------- the generator itself
def test_generator_features():
    """Every feature the issue lists is realised by a family, the nonants include a
    lower-only and a boxed column, and a scenario does not depend on the batch size."""
    fl = {k: family(k, 1).flags for k in TRAJ_FAMILIES + ["finvary"]}
    for feat in ("eq", "range", "le", "ge"):
        assert any(f["rows"][feat] for f in fl.values()), feat
    for feat in ("lo", "up", "box", "free", "fixed"):
        assert any(f["cols"][feat] for f in fl.values()), feat
    assert fl["fixed_empty_upper"]["empty_cols"] == 1 and fl["fixed_empty_upper"]["cols"]["fixed"] == 1
    assert fl["eq_range_free"]["cols"]["free"] == 2
    assert fl["nvar0"]["nvar"] == 0 and fl["plain"]["nvar"] > 0
    only = lambda f: (f["c_vary"], f["bnd_vary"], f["rhs_vary"])
    assert only(fl["c_only"]) == (True, False, False) and only(fl["bnd_only"]) == (False, True, False)
    assert only(fl["nvar0"]) == (False, False, True) and only(fl["vary_all"]) == (True, True, True)
    assert fl["multistage"]["stages"] == 3 and fl["finvary"]["finiteness_varies"]
    assert (fl["limit"]["n"], fl["limit"]["m"], fl["limit"]["nnz"]) == (64, 24, 384)
    assert all(not f["finiteness_varies"] for k, f in fl.items() if k != "finvary")
    a, b = sc.SynthFamily("vary_all", 1, S=70), sc.SynthFamily("vary_all", 1, S=200)
    for name in ("A", "bl", "bu", "lb", "ub", "c"):
        assert np.array_equal(getattr(a, name), getattr(b, name)[:70]), name
    assert not np.array_equal(a.A, sc.SynthFamily("vary_all", 2).A)
    creator, scens, flags = sc.synth_family("plain", 1, n=7, m=3, N=2, S=5)
    assert (flags["n"], flags["m"], flags["N"], len(scens)) == (7, 3, 2, 5)
    sf = creator("scen4").standard_form()
    assert np.array_equal(sf["c"], scens[4].c) and np.array_equal(sf["lb"], scens[4].lb)
    assert np.array_equal(sf["bu"], scens[4].bu) and sf["c0"] == scens[4].c0
    dense = np.zeros_like(scens[4].A)
    dense[np.repeat(np.arange(3), np.diff(sf["rowptr"])), sf["colidx"]] = sf["vals"]
    assert np.array_equal(dense, scens[4].A)


def test_fill_pattern_in_emitted_source(emu):
    """The fill family's symbolic Cholesky has fill: the emitted lnz table is set at
    positions that are no pair position, and equals a host recomputation."""
    fam = family("fill", 1)
    src = lane_source(emu, fam)
    lnz = np.array(emitted_table(src, "lnz"), dtype=bool)
    pairs = np.zeros(len(lnz), dtype=bool)
    pairs[emitted_table(src, "pair_pos")] = True
    want_pair, want_lnz = sc.symbolic_fill(fam.rowptr, fam.colidx, fam.m)
    diag = [i * (i + 1) // 2 + i for i in range(fam.m)]
    assert np.array_equal(pairs | np.isin(np.arange(len(lnz)), diag), want_pair)
    assert np.array_equal(lnz, want_lnz)
    assert int((lnz & ~want_pair).sum()) >= 6, "no fill"
    # and the other literal tables are the family's
    kinds = fam.ckind
    assert emitted_table(src, "lfin") == [int(k in ("lo", "box", "fixed")) for k in kinds]
    assert emitted_table(src, "ufin") == [int(k in ("up", "box", "fixed")) for k in kinds]
    assert emitted_table(src, "eq") == [int(k == "eq") for k in fam.rkind]
    kvar = emitted_table(src, "kvar")
    assert [k for k in range(fam.nnz) if kvar[k] >= 0] == fam.vark.tolist()


# ---------------------------------------------------------------- trajectories
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("key", TRAJ_FAMILIES)
def test_trajectory_vs_oracle_emu(emu, key, seed):
    """Every family at two seeds, S = 70, 4 PH iterations, on the lane solver; then the
    host recheck of the engine's own x."""
    fam = family(key, seed)
    ph, conv, _, _ = check_vs_oracle(emu, "cpu", fam)
    assert ph._native.jit_info(ph._ctx).decode().startswith("on"), ph._native.jit_info(ph._ctx)
    if conv < 1e-10:
        # consensus at the last iteration: the loop stops before that iteration's solve
        # (phbase.py:930-934), so the last solve is the one of the run with an iteration
        # less (a deterministic prefix), whose W / x-bar are still the solve's
        ph = run(emu, "cpu", fam, ITERS - 1)[0]
    host_recheck(ph, fam)


def check_paths(lib, device, fam, paths=PATHS):
    """The paths that share one structure give the default path's trajectory, to the
    tolerances of test_lane_and_generic_paths_agree."""
    base = check_vs_oracle(lib, device, fam)
    assert hasattr(base[0], "iterk_stats")
    out = {"default": base}
    for name, so in paths.items():
        ph, conv, Eobj, tb = out[name] = run(lib, device, fam, ITERS, so)
        assert all_certified(ph), name
        errs = (rel(ph.W_array(), base[0].W_array()), rel(engine_xbar(ph, fam), engine_xbar(base[0], fam)),
                rel(Eobj, base[2]), rel(tb, base[3]))
        print(fam.family, name, ["%.1e" % e for e in errs])
        assert errs[0] < 1e-8, name
        assert errs[1] < 1e-9, name
        assert errs[2] < 1e-9 and errs[3] < 1e-9, name
    assert not hasattr(out["host_loop"][0], "iterk_stats")
    st = out["starved"][0]
    assert st.iterk_stats["stragglers"] + sum(r.get("stragglers", 0) for r in st.solve_stats) > 0
    # the row duals of every path's last solve (the starved path's: written by the tier
    # that finished its lanes)
    for name, res in out.items():
        kkt_recheck(res[0], tag="%s %s" % (fam.family, name))
    return out


@pytest.mark.parametrize("key", sc.GPU_FAMILIES)
def test_paths_agree_emu(emu, key):
    check_paths(emu, "cpu", family(key, 1))


# ---------------------------------------------------------------- dispatch edges
def check_beyond_limits(lib, device, fam, so=None, want="off: size"):
    """A family the lane solver does not serve: the reason, the oracle's trajectory on
    the generic tiers (host loop: per-solve statistics), and which tier certified."""
    so = dict(so or {}, native_loop=0)
    res = check_vs_oracle(lib, device, fam, so)
    ph = res[0]
    ph.main_result = res[1:]                           # (conv, E[obj], trivial bound) of this run
    info = ph._native.jit_info(ph._ctx).decode()
    assert info.startswith(want), info
    served = {k: sum(s[k] for s in ph.solve_stats) for k in ("wg_certified", "sp_certified", "lane_certified")}
    served["pdhg"] = sum(s["pdhg_iters"] for s in ph.solve_stats)
    print(fam.flags["n"], fam.flags["m"], fam.flags["nnz"], info, served)
    assert served["lane_certified"] == 0
    kkt_recheck(ph, tag="%s %s" % (fam.family, so))
    return ph, served


def test_lane_limit_is_served_emu(emu):
    fam = family("limit", 1)
    ph = run(emu, "cpu", fam, 0)[0]
    assert ph._native.jit_info(ph._ctx).decode().startswith("on")
    assert ph.solve_stats[0]["lane_certified"] == fam.S
    assert "NMAX_N = 64, NMAX_M = 24, NMAX_K = 384," in lane_source(emu, fam)


BEYOND = {"n65": sc.sized_family(65, 24), "m25": sc.sized_family(64, 25), "nnz385": sc.sized_family(64, 24, nnz=385),
          "n65_m6": sc.sized_family(65, 6), "n30_m25": sc.sized_family(30, 25)}


@pytest.mark.parametrize("key", sorted(BEYOND))
def test_beyond_lane_limits_emu(emu, key):
    fam = family(BEYOND[key], 1)
    if key == "nnz385":
        assert (fam.n, fam.m, fam.nnz) == (64, 24, 385)
    ph, served = check_beyond_limits(emu, "cpu", fam)
    assert served["wg_certified"] + served["sp_certified"] > 0, served
    host_recheck(ph, fam)


def test_bound_finiteness_varies_emu(emu):
    fam = family("finvary", 1)
    ph, served = check_beyond_limits(emu, "cpu", fam, want="off: bound finiteness varies across scenarios")
    host_recheck(ph, fam)


GENERIC_CASES = {
    # family, solver options, environment, the lane solver's state on the GPU library
    "n65_m6": ("n65_m6", {}, {}, "off: size"),
    "n30_m25": ("n30_m25", {}, {}, "off: size"),
    "n65_m6/no_wg": ("n65_m6", {"wg_warm": 0}, {}, "off: size"),
    "n30_m25/no_wg": ("n30_m25", {"wg_warm": 0}, {}, "off: size"),
    # a small family with the lane solver off: Iter0 on PDHG + polish, then the
    # workgroup warm pass; without that pass, PDHG + polish throughout
    "vary_all/no_jit": ("vary_all", {"lane_solver": 0}, {"PHX_NO_JIT": "1"}, "off: PHX_NO_JIT set"),
    "vary_all/no_jit/no_wg": ("vary_all", {"lane_solver": 0, "wg_warm": 0}, {"PHX_NO_JIT": "1"},
                              "off: PHX_NO_JIT set"),
}


def check_generic_tiers(lib, device, monkeypatch, emulated=False):
    """The workgroup, sparse and PDHG + polish tiers: each case against the oracle,
    which tier certified its lanes printed, and each tier certifies lanes in at
    least one case (PDHG's count: the certified lanes no other tier claims).
    emulated: the emulation gives no reason with its "off"."""
    seen = {"wg_certified": 0, "sp_certified": 0, "pdhg_certified": 0}
    for name, (key, so, env, want) in GENERIC_CASES.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fam = family(BEYOND.get(key, key), 1)
        ph, served = check_beyond_limits(lib, device, fam, so, want="off" if emulated and env else want)
        for k in env:
            monkeypatch.delenv(k)
        lanes = fam.S * len(ph.solve_stats)
        served["pdhg_certified"] = lanes - served["wg_certified"] - served["sp_certified"] if served["pdhg"] else 0
        print(name, "served by", {k: served[k] for k in seen}, "of", lanes)
        if so.get("wg_warm", 1) == 0:
            assert served["wg_certified"] == 0
        for k in seen:
            seen[k] += served[k]
    assert all(v > 0 for v in seen.values()), seen
    return seen


def test_generic_tiers_emu(emu, monkeypatch):
    check_generic_tiers(emu, "cpu", monkeypatch, emulated=True)


def test_sp_off_on_sparse_context_raises_emu(emu):
    """As the library (test_sp_off_on_sparse_context_raises_gpu): sp = 0 on a context
    that holds the sparse solver's workspaces only is refused, not run on the dense
    polish factor the context does not hold."""
    from mpisppy_amd._native import NativeError
    with pytest.raises(NativeError, match="sp = 0"):
        run(emu, "cpu", family(BEYOND["n30_m25"], 1), 2, {"wg_warm": 0, "sp": 0})


def test_batch_creator_equals_models_emu(emu):
    """The vectorised batch_creator of a family (the large GPU batches) is the
    per-scenario creator's batch, bit for bit."""
    fam = family("vary_all", 1)
    a = run(emu, "cpu", fam, 3)
    b = run(emu, "cpu", fam, 3, creator=fam.batch_creator_fn())
    assert np.array_equal(a[0].W_array(), b[0].W_array()) and np.array_equal(a[0]._host("x"), b[0]._host("x"))
    assert a[1:] == b[1:]


# ---------------------------------------------------------------- scenario-donor xhat
def feasible_donor(fam, o):
    """The first scenario whose Iter0 nonants the oracle finds feasible in every
    scenario (the families have no complete recourse), and two more after it."""
    scens = fam.scens()
    found = []
    for k in range(fam.S):
        if oph.evaluate_xhat(scens, xc.donor_cache(o, {"ROOT": fam.names[k]}))[2].all():
            found.append({"ROOT": fam.names[k]})
            if len(found) == 3:
                break
    assert found, "no donor is feasible in every scenario"
    return found


def check_xhat(lib, device, fam, lane):
    """Xhat_Eval.evaluate at the known point's nonants (explicit bounds), then
    XhatBase._try_one over donors (phx_fix_nonants) against oracle.ph.evaluate_xhat to
    1e-9, then the bounds restored and the plain solve recovered."""
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    ev = Xhat_Eval(xc.xhat_options(), fam.names, fam.creator, scenario_creator_kwargs=fam.kwargs,
                   _native_lib=lib, _device=device)
    ev.solve_loop()
    before = ev.nonant_values().copy()
    o = oracle_iter0(fam)
    assert rel(ev._host("obj"), o.obj) < 1e-8
    scens = fam.scens()
    xhat = {"ROOT": fam.x0[:fam.N].copy()}
    E = ev.evaluate(xhat)
    Eo, objs, feas = oph.evaluate_xhat(scens, xhat)
    assert feas.all() and ev.infeas_prob() == 0.0
    assert rel(E, Eo) < 1e-9
    assert rel(np.array([ev.objs_dict[nm] for nm in fam.names]), objs) < 1e-9
    ev._unfix_nonants()
    ev.solve_loop()
    assert rel(ev.nonant_values(), before) < 1e-9
    xc.check_try_one(ev, fam.family, fam.S, feasible_donor(fam, o), lane=lane, scens=scens)
    if lane:
        assert "fixed-nonant lane module on" in ev._native.jit_info(ev._ctx).decode()
    xc.check_restored_solve(ev, before, lane=lane)


def test_xhat_donor_emu(emu):
    check_xhat(emu, "cpu", family("fixed_empty_upper", 1), lane=False)


# ---------------------------------------------------------------- hipRTC compile of the sources
@pytest.mark.parametrize("key", sc.GPU_FAMILIES + ["fixed_empty_upper/fixed"])
def test_synth_lane_source_compiles_gfx950(emu, key):
    """The small families' lane sources (and one fixed-nonant structure) compile with
    the library's hipRTC options for gfx950 and export every kernel the library loads.
    (The structure at the lane limits is not compiled in any test: minutes of hipRTC.)"""
    import test_jit_source as tj
    if not os.path.exists(tj._HIPRTC):
        pytest.fail("no hipRTC in this image")
    name, _, fixed = key.partition("/")
    fam = family(name, 1)
    assert fam.n <= 10 and fam.m <= 6
    src = lane_source(emu, fam, fixed=bool(fixed))
    assert "struct PT" in src
    if fixed:
        assert "bnd_vary() { return true; }" in src
        assert emitted_table(src, "fixed")[:fam.N] == [1] * fam.N
    rc, log, code = tj.hiprtc_compile(src)
    assert rc == 0, log[-4000:]
    kernels = tj.lane_kernels(emu)
    symbols = tj.elf_symbols(code)
    for k in kernels:
        assert k in symbols and k + ".kd" in symbols, k
