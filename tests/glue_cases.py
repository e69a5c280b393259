"""Direct checks of the PH objective terms (phx_set_ph_terms + phx_objective) and of
the slot export (phx_export_slots) on chosen inputs, at the sizes where the host
entry point of the terms changes kernels.

As reduction_cases.py: every ``check_*(lib, device, ...)`` builds a ``PH`` object on
a synthetic scenario creator, never calls ``ph_main``, writes its own values into
the device state and calls the library.  ``test_glue.py`` runs each check on the
host emulation (which validates the harness and the reference) and on the HIP
kernels.

The creator: k1 first-stage nonants, optionally k2 second-stage nonants under the
stage-2 nodes of the uneven tree ``T3U``; columns that are no nonants before the
first nonant, after every third and at the end; each node's nonants declared in a
seeded order that is neither the column order nor monotone (``slot_col`` /
``col_slot`` are real maps); one trivial row; a non-zero cost on every column,
shared by the scenarios or different in each (``c_vary``: k_objective's two
strides).

Inputs: seeded, all distinct, mixed sign with magnitudes in [0.5, 2] for x, W and
x-bar, rho in [0.5, 2], costs alike.  The narrow range is deliberate: every term is
then a fixed fraction of sum|term| (at least 1 / (128 T)), so a dropped, doubled or
misplaced term exceeds the bound below by more than 1e5; over a range of 1e-3..1e3
a small term could hide inside it.

Reference of the objective: ``math.fsum`` per scenario over the float64 terms
``c_j x_j`` (n of them) and, per nonant slot, ``W x``, ``-(rho xbar) x``,
``rho/2 x^2`` and ``rho/2 xbar^2`` (those switched on): T = n + 4 N terms with both on.
Bound (derived, not tuned; u = 2**-53): ``|got - ref| <= (T + 6) u sum|term|``.
The library forms q = W - rho xbar once, rounded, then q x + p/2 x^2 + c x + k:
against the exact terms each contributes at most 4 roundings of its own size,
contracted or not, and a sum of T terms in any order at most (T - 1) u sum|term|;
the reference's own products add at most 2 u per term and fsum one rounding of the
total; the rest is second order.

The run (check_ph_objective), on one context: (W_on, prox_on) = (1,1), (0,0), (1,0),
(0,1), (1,1) in that order, so that qN / pN / kN / kpart left by the call before
would show; phx_objective twice per setting into buffers prefilled with different
sentinels, bit for bit equal (the second reads the cached terms); the last (1,1)
bit for bit the first; a term switched off reads neither its NULL nor its NaN-filled
array; W changed in place behind the same pointer is picked up by the next
phx_set_ph_terms.

Dispatch paths (launch_ph_terms): N < 16 k_ph_terms; 16 <= N with at most 8 chunks
(of 8 slots below N = 64, of 32 from there: N <= 256) k_ph_terms2 alone; more chunks
k_ph_terms2 + kpart + k_ph_terms_k.

The bound was fixed before any GPU run, against the host emulation only (one loop
for all three paths; worst error-to-bound ratio there 0.17 at N < 16 -- N = 1, both
terms off --, 0.081 for 16 <= N <= 256, 0.0082 from N = 257).  First measurement on
the MI355X, worst ratio per path: k_ph_terms 0.20 (N = 1, both terms off; 0.12 at
the T3U tree), k_ph_terms2 alone 0.054, k_ph_terms2 + k_ph_terms_k 0.0074.  The
ratios fall with N because the bound grows with T while rounding errors mostly
cancel.  The slot export is exact on both.
"""
import functools
import math

import numpy as np
import torch

import mpisppy_amd  # noqa: F401
from mpisppy_amd import model as lm
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.scenario_tree import ScenarioNode
from helpers import ph_options
from reduction_cases import SENTINEL, T3U, U, _get, _put, _ratio

T3U_COUNTS = T3U["counts"]


# ---------------------------------------------------------------- the PH object
def _order(k, seed):
    """a seeded order of range(k), for k >= 3 neither the identity nor monotone"""
    p = np.random.default_rng(100 + 7 * k + seed).permutation(k)
    if k >= 3 and (np.all(np.diff(p) > 0) or np.all(np.diff(p) < 0)):
        p[[0, 1]] = p[[1, 0]]
    if k == 2:
        p = np.array([1, 0])
    return [int(v) for v in p]


def signed(rng, shape, lo=0.5, hi=2.0):
    """mixed sign, magnitudes in [lo, hi]"""
    return rng.choice([-1.0, 1.0], size=shape) * rng.uniform(lo, hi, size=shape)


@functools.lru_cache(maxsize=None)
def cost_table(n, S, c_vary):
    """(S, n) costs: one row repeated, or a row per scenario"""
    rng = np.random.default_rng(31 + n + 1000 * S + int(c_vary))
    c = signed(rng, (S, n) if c_vary else (1, n))
    return np.ascontiguousarray(np.broadcast_to(c, (S, n)))


def ncols(k1, k2):
    return k1 + k2 + (k1 + k2 + 2) // 3 + 1


def _creator(name, k1=1, k2=0, counts=None, S=1, c_vary=False):
    i = int(name[4:])
    m = lm.LinearModel(name)
    a, b, f = [], [], []
    for j in range(k1 + k2):
        if j % 3 == 0:
            f.append(m.add_var("f%d" % len(f), -1e4, 1e4))
        if j < k1:
            a.append(m.add_var("a%d" % j, -1e4, 1e4))
        else:
            b.append(m.add_var("b%d" % (j - k1), -1e4, 1e4))
    f.append(m.add_var("f%d" % len(f), -1e4, 1e4))
    n = m.nvars
    assert n == ncols(k1, k2)
    m.add_constraint(a[0] + f[0], None, 4e4)
    c = cost_table(n, S, bool(c_vary))[i]
    m.set_objective(lm.LinExpr({j: float(c[j]) for j in range(n)}, 0.0, m), lm.minimize)
    m._mpisppy_probability = 1.0 / S
    nodes = [ScenarioNode("ROOT", 1.0, 1, f[0], [a[p] for p in _order(k1, 0)], m)]
    if counts:
        v = int(np.searchsorted(np.cumsum(counts), i, side="right"))
        nodes.append(ScenarioNode("ROOT_%d" % v, counts[v] / S, 2, f[-1], [b[p] for p in _order(k2, 1)], m,
                                  parent_name="ROOT"))
    m._mpisppy_node_list = nodes
    return m


def build_ph(lib, device, k1, S=None, k2=0, counts=None, c_vary=False):
    if counts:
        S = int(sum(counts))
        nodenames = (["ROOT"] + ["ROOT_%d" % v for v in range(len(counts))]
                     + ["ROOT_%d_0" % v for v in range(len(counts))])
    else:
        nodenames, k2 = None, 0
    names = ["scen%d" % i for i in range(S)]
    ph = PH(ph_options(1), names, _creator, all_nodenames=nodenames,
            scenario_creator_kwargs=dict(k1=k1, k2=k2, counts=counts, S=S, c_vary=c_vary),
            _native_lib=lib, _device=device)
    ph.attach_Ws_and_prox()
    b = ph.batch
    N = k1 + k2
    assert (b.nonant.N, b.n, bool(b.c_vary)) == (N, ncols(k1, k2), bool(c_vary) and S > 1)
    col = b.nonant.slot_col
    assert len(set(col.tolist())) == N and N < b.n            # columns that are no nonants
    if k1 >= 3:
        assert np.any(np.diff(col[:k1]) < 0) and np.any(np.diff(col[:k1]) > 0), "slot_col is monotone"
    return ph


# ---------------------------------------------------------------- the objective
def terms_path(N):
    """which kernels launch_ph_terms runs for N slots"""
    if N < 16:
        return "k_ph_terms"
    nch = -(-N // (32 if N >= 64 else 8))
    return "k_ph_terms2" if nch <= 8 else "k_ph_terms2+k_ph_terms_k"


def objective_reference(c, x, cols, W, rho, xb, W_on, prox_on):
    """(ref, bound) per scenario from c, x (n, S) and W, rho, x-bar (N, S)"""
    xn = x[cols]
    parts = [c * x]
    if W_on:
        parts.append(W * xn)
    if prox_on:
        parts += [-(rho * xb) * xn, 0.5 * rho * xn * xn, 0.5 * rho * xb * xb]
    t = np.concatenate(parts, axis=0)
    T, S = t.shape
    ref = np.array([math.fsum(t[:, s]) for s in range(S)])
    bound = (T + 6) * U * np.array([math.fsum(np.abs(t[:, s])) for s in range(S)])
    return ref, bound


SETTINGS = ((1, 1), (0, 0), (1, 0), (0, 1), (1, 1))

OBJ_CASES = {}
for _N in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 256, 257, 300):
    OBJ_CASES["N%d" % _N] = [dict(k1=_N, S=65)]
OBJ_CASES.update({
    "N300-then-N257": [dict(k1=300, S=65), dict(k1=257, S=65)],       # two contexts alive in one process
    "S1-N17": [dict(k1=17, S=1)],
    "S1-N257": [dict(k1=257, S=1)],
    "S257-N17": [dict(k1=17, S=257)],                                 # a second 256-thread block, one live thread
    "S257-N257": [dict(k1=257, S=257)],
    "T3u-N5": [dict(k1=3, k2=2, counts=T3U_COUNTS)],                  # node-indexed xbar_idx, k_ph_terms
    "T3u-N17": [dict(k1=14, k2=3, counts=T3U_COUNTS)],                # ... and k_ph_terms2
    "N17-cvary": [dict(k1=17, S=65, c_vary=True)],
    "N257-cvary": [dict(k1=257, S=65, c_vary=True)],
})


class _Obj:
    """One objective problem: its PH object, inputs and device arrays."""

    def __init__(self, lib, device, cfg):
        self.lib = lib
        self.ph = ph = build_ph(lib, device, **cfg)
        b = ph.batch
        self.N, self.S, self.n, self.NNS = b.nonant.N, ph._S, b.n, ph.NNS
        N, S, n, NNS = self.N, self.S, self.n, self.NNS
        rng = np.random.default_rng(4000 + S + 13 * N + NNS)
        self.x = signed(rng, (n, S))
        self.W = signed(rng, (N, S))
        self.W2 = signed(rng, (N, S))
        self.rho = rng.uniform(0.5, 2.0, size=(N, S))
        self.xbar = signed(rng, NNS)
        every = np.concatenate([v.ravel() for v in (self.x, self.W, self.W2, self.rho, self.xbar)])
        assert np.unique(np.abs(every)).size == every.size, "inputs are not all distinct"
        self.c = cost_table(n, S, bool(cfg.get("c_vary"))).T
        self.cols = b.nonant.slot_col
        self.xb = self.xbar[ph._xbar_idx]
        if NNS > N:
            assert np.unique(ph._xbar_idx).size == NNS          # every node's entries are read
        _put(ph._x, self.x)
        _put(ph._W, self.W)
        _put(ph._rho, self.rho)
        buf = np.full(ph._node_buf.numel(), SENTINEL)
        buf[:NNS] = self.xbar
        _put(ph._node_buf, buf)
        nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device=ph.device)
        self.nanW, self.nanrho, self.nanxb = nan(N * S), nan(N * S), nan(NNS)

    def call(self, W_on, prox_on, nan_off=False):
        """phx_set_ph_terms, then phx_objective twice; a term switched off is given
        NULL, or (nan_off) an array of NaN"""
        ph, lib = self.ph, self.lib
        off = (lambda t: t.data_ptr()) if nan_off else (lambda t: None)
        W = ph._W.data_ptr() if W_on else off(self.nanW)
        rho = ph._rho.data_ptr() if prox_on else off(self.nanrho)
        xb = ph._xbar_node.data_ptr() if prox_on else off(self.nanxb)
        idx = ph._xbar_idx_t.data_ptr() if (prox_on or nan_off) else None
        lib.check(ph._ctx, lib.set_ph_terms(ph._ctx, W, rho, xb, idx, W_on, prox_on, ph._stream()), "set_ph_terms")
        outs = []
        for fill in (SENTINEL, -SENTINEL):
            out = torch.full((self.S,), fill, dtype=torch.float64, device=ph.device)
            lib.check(ph._ctx, lib.objective(ph._ctx, ph._x.data_ptr(), out.data_ptr(), ph._stream()), "objective")
            outs.append(_get(out))
        assert np.array_equal(outs[0], outs[1]), "phx_objective does not repeat bit for bit"
        return outs[0]

    def ratio(self, got, W, W_on, prox_on):
        ref, bound = objective_reference(self.c, self.x, self.cols, W, self.rho, self.xb, W_on, prox_on)
        return _ratio(got, ref, bound)


def check_ph_objective(lib, device, case):
    worst = {}
    alive = []
    for cfg in OBJ_CASES[case]:
        o = _Obj(lib, device, cfg)
        alive.append(o)                                     # (the contexts before stay alive)
        got, ratios = [], []
        for W_on, prox_on in SETTINGS:
            g = o.call(W_on, prox_on)
            assert np.isfinite(g).all()
            if not (W_on and prox_on):
                assert np.array_equal(o.call(W_on, prox_on, nan_off=True), g), \
                    "a term switched off was read (%d, %d)" % (W_on, prox_on)
            got.append(g)
            ratios.append(o.ratio(g, o.W, W_on, prox_on))
        assert np.array_equal(got[0], got[4]), "(1,1) after the other settings differs from the first (1,1)"
        # W changed in place behind the same pointer
        _put(o.ph._W, o.W2)
        g2 = o.call(1, 1)
        assert not np.array_equal(g2, got[0])
        ratios.append(o.ratio(g2, o.W2, 1, 1))
        path = terms_path(o.N)
        print("[ph objective %s] S=%d N=%d n=%d NNS=%d %s worst error/bound per setting %s, new W %.3g" % (
            case, o.S, o.N, o.n, o.NNS, path, ["%.3g" % r for r in ratios[:5]], ratios[5]))
        assert max(ratios) <= 1.0, (case, cfg, ratios)
        worst[path] = max(worst.get(path, 0.0), max(ratios))
    return worst


# ---------------------------------------------------------------- the slot export
EXPORT_SIZES = ((1, 1), (3, 65), (17, 257), (257, 65), (300, 257))


def check_export_slots(lib, device, N, S):
    """phx_export_slots: out[s*N + j] == src[j*S + s] exactly and nothing written
    behind; at (17, 257) also PHBase._populate_W_cache / W_from_flat_list, the same
    wire format from the object's own W."""
    ph = build_ph(lib, device, k1=N, S=S)
    rng = np.random.default_rng(6000 + N + 1000 * S)
    src = signed(rng, (N, S), 1e-3, 1e3)
    assert np.unique(src).size == src.size
    src_t = torch.empty(N * S, dtype=torch.float64, device=ph.device)
    _put(src_t, src)
    out_t = torch.full((S * N + 3,), SENTINEL, dtype=torch.float64, device=ph.device)
    lib.check(ph._ctx, lib.export_slots(ph._ctx, src_t.data_ptr(), out_t.data_ptr(), ph._stream()), "export_slots")
    out = _get(out_t)
    assert np.array_equal(out[:S * N].reshape(S, N), src.T)
    assert np.all(out[S * N:] == SENTINEL), "phx_export_slots wrote behind S*N"
    assert np.array_equal(_get(src_t).reshape(N, S), src)
    if (N, S) == (17, 257):
        _put(ph._W, src)
        cache = np.full(N * S + 3, SENTINEL)
        ph._populate_W_cache(cache, 3)
        assert np.array_equal(cache[:N * S], out[:N * S]) and np.all(cache[N * S:] == SENTINEL)
        ph.W_from_flat_list(list(cache[:N * S] * 2))
        assert np.array_equal(ph.W_array(), 2 * src.T)
        assert np.array_equal(_get(ph._W).reshape(N, S), 2 * src)
