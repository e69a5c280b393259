"""Shared cases of the scenario-donor xhat tests (test_xhat_donor.py on the
ABI emulation, test_xhat_donor_gpu.py on the kernels): the numpy restatements
of phx_donor_gather / phx_fix_nonants and the ``_try_one`` checks against the
oracle's fixed-xhat evaluation."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel
from mpisppy_amd import _native
from mpisppy_amd.examples import aircond, farmer
from mpisppy_amd.extensions.xhatbase import XhatBase
from mpisppy_amd.utils import sputils
from mpisppy_amd.utils.xhat_eval import Xhat_Eval
from oracle import models as om, ph as oph

S_LIST = [1, 63, 64, 65, 257, 1025]


def xhat_options(solver_options=None):
    return {"iter0_solver_options": None, "iterk_solver_options": None, "display_timing": False,
            "solver_name": "phx", "verbose": False, "solver_options": solver_options}


def make_eval(lib, device, model, size, mpicomm=None, solver_options=None):
    """(Xhat_Eval, node names) for ("farmer", S) or ("aircond", branching factors)."""
    if model == "farmer":
        ev = Xhat_Eval(xhat_options(solver_options), farmer.scenario_names_creator(size), farmer.scenario_creator,
                       scenario_creator_kwargs={"num_scens": size}, mpicomm=mpicomm, _native_lib=lib,
                       _device=device)
        return ev, ["ROOT"]
    bf = list(size)
    S = int(np.prod(bf))
    nodes = sputils.create_nodenames_from_branching_factors(bf)
    ev = Xhat_Eval(xhat_options(solver_options), aircond.scenario_names_creator(S), aircond.scenario_creator,
                   all_nodenames=nodes, scenario_creator_kwargs={"branching_factors": bf, "start_seed": 0},
                   mpicomm=mpicomm, _native_lib=lib, _device=device)
    return ev, nodes


def oracle_scens(model, size):
    if model == "farmer":
        return [om.farmer("scen%d" % i, num_scens=size) for i in range(size)]
    bf = list(size)
    return [om.aircond("scen%d" % i, bf, start_seed=0) for i in range(int(np.prod(bf)))]


# ---------------------------------------------------------------- the two entry points
def local_nodes(ev):
    """[(node index, first local scenario, last + 1, first slot, slots)] of the
    local tree nodes, in the tree descriptor's order."""
    out = []
    for v in sorted(set(t[0] for t in ev._tiles)):
        ts = [t for t in ev._tiles if t[0] == v]
        out.append((v, min(t[1] for t in ts), max(t[2] for t in ts), ts[0][3], ts[0][4]))
    return out


def gather_ref(ev, vals, donor, nodes=None):
    """phx_donor_gather restated: vals (N, S) host, donor per local node."""
    out = np.zeros(max(ev.NNS, 1))
    for k, (v, lo, hi, slot, nlen) in enumerate(nodes if nodes is not None else local_nodes(ev)):
        if donor[k] >= 0:
            out[ev._node_off[v]:ev._node_off[v] + nlen] = vals[slot:slot + nlen, donor[k]]
    return out


def call_gather(ev, vals_t, donor, tree=None):
    out = torch.full((max(ev.NNS, 1),), -7.0, dtype=torch.float64, device=ev.device)
    d = np.ascontiguousarray(donor, dtype=np.int32)
    lib = ev._native
    lib.check(ev._ctx, lib.donor_gather(ev._ctx, ctypes.byref(tree if tree is not None else ev._tree),
                                        vals_t.data_ptr(), d.ctypes.data_as(_native.P_i32), out.data_ptr(),
                                        ev._stream()), "donor_gather")
    return out.cpu().numpy()


def tree_without_last_node(ev):
    """A copy of the tree descriptor in which the last local node is absent (as
    on a rank that holds none of its scenarios): its entries read zero."""
    t = _native.TreeDesc()
    ctypes.pointer(t)[0] = ev._tree
    nodes = local_nodes(ev)
    t.nnodes = len(nodes) - 1
    t.nnodes_cover = int(sum(n[4] for n in nodes[:-1]))
    return t, nodes[:-1]


def check_gather(ev):
    """First / last scenario of every node, a node without a local donor, a node
    absent locally, and the rejected donors: exact equality."""
    rng = np.random.default_rng(11)
    N, S = ev.batch.nonant.N, ev._S
    vals = rng.standard_normal((N, S)) * 100.0
    vals_t = torch.as_tensor(vals, device=ev.device).contiguous()
    nodes = local_nodes(ev)
    first = [n[1] for n in nodes]
    last = [n[2] - 1 for n in nodes]
    mixed = [(lo + hi - 1) // 2 if k % 2 else hi - 1 for k, (_, lo, hi, _, _) in enumerate(nodes)]
    for donor in (first, last, mixed):
        assert np.array_equal(call_gather(ev, vals_t, donor), gather_ref(ev, vals, donor))
    # one node has no local donor: zeros there, the others as before
    for k in range(len(nodes)):
        donor = list(last)
        donor[k] = -1
        got = call_gather(ev, vals_t, donor)
        v, _, _, _, nlen = nodes[k]
        assert not got[ev._node_off[v]:ev._node_off[v] + nlen].any()
        assert np.array_equal(got, gather_ref(ev, vals, donor))
    if len(nodes) > 1:
        tree, kept = tree_without_last_node(ev)
        got = call_gather(ev, vals_t, first[:-1], tree=tree)
        assert np.array_equal(got, gather_ref(ev, vals, first[:-1], nodes=kept))
        v, _, _, _, nlen = nodes[-1]
        assert not got[ev._node_off[v]:ev._node_off[v] + nlen].any()
    # a donor outside its node's local scenarios
    for k, bad in ((0, S), (len(nodes) - 1, nodes[-1][1] - 1 if nodes[-1][1] > 0 else -2), (0, -5)):
        donor = list(first)
        donor[k] = bad
        with pytest.raises(_native.NativeError, match="outside the node's local scenarios"):
            call_gather(ev, vals_t, donor)


def check_fix(ev):
    """phx_fix_nonants: x's nonant columns are node_vals[xbar_idx] bit for bit,
    the other columns untouched; NULL restores."""
    rng = np.random.default_rng(5)
    n, S = ev.batch.n, ev._S
    nv = rng.standard_normal(max(ev.NNS, 1)) * 50.0 + 100.0
    nv_t = torch.as_tensor(nv, device=ev.device)
    x0 = rng.standard_normal((n, S))
    x_t = torch.as_tensor(x0, device=ev.device).contiguous()
    lib = ev._native
    lib.check(ev._ctx, lib.fix_nonants(ev._ctx, nv_t.data_ptr(), ev._xbar_idx_t.data_ptr(), x_t.data_ptr(),
                                       ev._stream()), "fix_nonants")
    want = x0.copy()
    want[ev.batch.nonant.slot_col] = nv[ev._xbar_idx]
    assert np.array_equal(x_t.cpu().numpy(), want)
    # without x: only the bounds
    lib.check(ev._ctx, lib.fix_nonants(ev._ctx, nv_t.data_ptr(), ev._xbar_idx_t.data_ptr(), None, ev._stream()),
              "fix_nonants")
    lib.check(ev._ctx, lib.fix_nonants(ev._ctx, None, None, None, ev._stream()), "fix_nonants")
    if ev.device.type == "cuda":
        torch.cuda.synchronize()


# ---------------------------------------------------------------- _try_one against the oracle
def donor_cache(o, donors):
    """{node: the donor's Iter0 nonants of that node} from the oracle's x."""
    xn = o.xn()
    names = [s.name for s in o.scens]
    cache = {}
    for ndn, sname in donors.items():
        k = names.index(sname)
        cache[ndn] = np.array([xn[k, j] for j in range(o.N) if o.node_of[k][j] == ndn])
    return cache


def last_stats(ev):
    st = _native.SolveStats()
    ev._native.check(ev._ctx, ev._native.last_solve_stats(ev._ctx, ctypes.byref(st)), "last_solve_stats")
    return st


def prepare(ev, o):
    """The oracle's Iter0 nonants as the engine's nonant cache and current values
    (what the spoke does with the hub's nonants)."""
    ev._save_original_nonants()
    ev._lazy_create_solvers()
    ev._save_nonants()
    ev._put_nonant_cache(o.xn().ravel())
    ev._restore_nonants()


def check_try_one(ev, model, size, donor_dicts, lane=False, sample=None, scens=None):
    """_try_one for each donor dict in turn (restore_nonants False, True, False,
    ...) against oracle.ph.evaluate_xhat; with ``lane`` every solve must be
    certified by the lane solver alone.  scens: the oracle's scenarios of a
    model other than farmer / aircond."""
    scens = scens if scens is not None else oracle_scens(model, size)
    o = oph.OraclePH(scens, rho=1.0)
    o.iter0()
    prepare(ev, o)
    cached = ev.nonant_cache.copy()
    xb = XhatBase(ev)
    xb.post_iter0()
    S = ev._S
    names = ev.local_scenario_names
    views = list(ev.local_scenarios[names[0]]._mpisppy_data.nonant_indices.values())
    for t, donors in enumerate(donor_dicts):
        restore = t % 2 == 1
        cache = donor_cache(o, donors)
        Eo, objs, feas = oph.evaluate_xhat(scens, cache)
        assert feas.all()
        E = xb._try_one(dict(donors), restore_nonants=restore)
        print("try_one", model, size, donors, "E", E, "oracle", Eo, "rel", rel(E, Eo))
        assert E is not None and rel(E, Eo) < 1e-9
        if lane:
            st = last_stats(ev)
            print("   lane_certified", st.lane_certified, "stragglers", st.stragglers, "jit", st.jit)
            assert st.lane_certified == S and st.stragglers == 0 and st.jit == 1
            assert ev.solve_stats[-1]["lane_certified"] == S and ev.solve_stats[-1]["stragglers"] == 0
        if restore:
            # values and fixedness as before the trial (xhatbase.py:227-228)
            assert np.array_equal(ev.nonant_values(), cached)
            assert not ev._fixed.any() and not any(v.fixed for v in views)
        else:
            # the nonants stay fixed at the donors' values, bit for bit
            want = np.empty_like(cached)
            for s in range(S):
                for j in range(o.N):
                    want[s, j] = cache[o.node_of[s][j]][ev.batch.nonant.slot_local[j]]
            assert np.array_equal(ev.nonant_values(), want)
            assert ev._fixed.all() and all(v.fixed for v in views)
            ev._fill_objs_dict()
            got = np.array([ev.objs_dict[nm] for nm in names])
            idx = np.arange(S) if sample is None else np.asarray(sample)
            assert rel(got[idx], objs[idx]) < 1e-9
    # the cache the donors are read from is untouched by the trials
    assert np.array_equal(ev.nonant_cache, cached)
    return xb, o


def check_restored_solve(ev, before, lane=False, solver_options=None):
    """After phx_fix_nonants(NULL) a plain solve returns the pre-trial nonants."""
    ev._restore_nonants_device()
    ev.solve_loop(solver_options=solver_options)
    assert rel(ev.nonant_values(), before) < 1e-9
    if lane:
        st = last_stats(ev)
        assert st.lane_certified == ev._S and st.stragglers == 0 and st.jit == 1


def check_infeasible(ev, lane=False):
    """A farmer candidate above the 500 acres: None, nonants restored, every
    scenario proven infeasible (through the generic path's interior point)."""
    S = ev._S
    ev._save_original_nonants()
    ev._lazy_create_solvers()
    ev._save_nonants()
    bad = np.tile([300.0, 300.0, 300.0], S)
    ev._put_nonant_cache(bad)
    ev._restore_nonants()
    xb = XhatBase(ev)
    assert xb._try_one({"ROOT": "scen0"}, restore_nonants=False) is None
    assert ev.solve_stats[-1]["infeasible"] == S
    assert np.array_equal(ev.nonant_values(), bad.reshape(S, 3))
    assert not ev._fixed.any()
