"""Direct checks of PH's cross-scenario reductions (phx_xbar, phx_update_w,
phx_expect) on chosen inputs, at the sizes where their host entry points
change kernels.

Every ``check_*(lib, device, ...)`` builds a ``PH`` object on a synthetic
scenario creator (k1 first-stage nonants, optionally k2 second-stage nonants
under stage-2 nodes ``ROOT_v`` of ``counts[v]`` scenarios each, one trivial
row, a trivial objective), never calls ``ph_main``, writes its own values into
the device state and calls the reduction.  ``test_reductions.py`` runs each
check on the host emulation (which validates the harness and the reference)
and on the HIP kernels.

Inputs: seeded values of mixed sign over 1e-3..1e3, distinct per (slot,
scenario); non-uniform ``pc`` and ``rho``; every output buffer prefilled with a
sentinel so that an entry never written shows.

Reference: ``math.fsum`` over the same float64 terms, formed in numpy as
``pc*x`` and ``(pc*x)*x``.  Tolerances (derived, not tuned; u = 2**-53):

* a sum of n terms in any order, with or without FMA contraction:
  ``|got - ref| <= (n + 2) u sum|term|`` per entry (any summation tree has a
  first-order error of at most (n - 1) u sum|term|; a contracted ``v*x`` differs
  from the rounded product by at most u|term|; the rest covers second order);
* W elementwise: ``|got - ref| <= 2 u (|W_in| + |rho (x - xbar)|)``, the
  reference being ``W_in + rho*(x - xbar)`` of the float64 difference evaluated
  in extended precision (one rounding of the product when it is not contracted,
  one of the sum).

A dropped or doubled scenario moves a sum by about sum|term|/n, orders of
magnitude above the bound.  Every call is made twice and must repeat bit for
bit (the kernels claim a fixed summation order).  Each check returns its worst
error-to-bound ratios and prints them.

The bounds were fixed before any GPU run, against the host emulation only
(worst there: x-bar 0.16, W 0.99 -- its product is not contracted --, dsum 0.55,
segment sums 0.19, expectations 0.0098).  First measurement on the MI355X,
worst ratio per path: x-bar 0.19 (k_small_xw) and 0.14 (k_xbar; the same for two slices added up);
W 0.50 on every path (the product is contracted there); dsum 0.39 (k_small_xw),
0.55 (k_update_w_seg), 0.26 (k_update_w_seg2), 0.29 (k_update_w); segment
sums 0.17 / 0.0012 / 0.0054 / 0.015 in that order; expectations 0.0011
(k_expect) and 0.00013 (k_expect_part + k_expect_fold).
"""
import math

import numpy as np
import torch

import mpisppy_amd  # noqa: F401
from mpisppy_amd import _native
from mpisppy_amd import model as lm
from mpisppy_amd.examples import farmer
from mpisppy_amd.opt.ph import PH
from mpisppy_amd.scenario_tree import ScenarioNode
from helpers import ph_options

U = 2.0 ** -53
SENTINEL = 7.0

# the uneven three-stage tree: node boundaries 1, 63, 65, 195, 200 straddle the
# wavefront boundaries 64, 128, 192 and the tile boundary 256
T3U = dict(k1=3, k2=2, counts=[1, 62, 2, 130, 5, 300])


# ---------------------------------------------------------------- the PH object
def _creator(name, k1=1, k2=0, counts=None, S=1):
    i = int(name[4:])
    m = lm.LinearModel(name)
    a = [m.add_var("a%d" % j, -1e4, 1e4) for j in range(k1)]
    b = [m.add_var("b%d" % j, -1e4, 1e4) for j in range(k2)]
    z = m.add_var("z", 0.0, 1.0)
    m.add_constraint(a[0] + z, None, 2e4)
    m.set_objective(z, lm.minimize)
    m._mpisppy_probability = 1.0 / S
    nodes = [ScenarioNode("ROOT", 1.0, 1, z, a, m)]
    if counts:
        v = int(np.searchsorted(np.cumsum(counts), i, side="right"))
        nodes.append(ScenarioNode("ROOT_%d" % v, counts[v] / S, 2, z, b, m, parent_name="ROOT"))
    m._mpisppy_node_list = nodes
    return m


def build_ph(lib, device, k1, S=None, k2=0, counts=None, lo=0, hi=None, options=None):
    """PH over scenarios [lo, hi) of the S = sum(counts) scenarios of the tree
    (the global node list: a slice holds the global NNS and its local nodes
    only, as a rank of a multi-rank run does; no process group is needed)."""
    if counts:
        S = int(sum(counts))
        nodenames = (["ROOT"] + ["ROOT_%d" % v for v in range(len(counts))]
                     + ["ROOT_%d_0" % v for v in range(len(counts))])
    else:
        nodenames = None
    opts = ph_options(1)
    opts.update(options or {})
    names = ["scen%d" % i for i in range(S)][lo:hi]
    ph = PH(opts, names, _creator, all_nodenames=nodenames,
            scenario_creator_kwargs=dict(k1=k1, k2=k2 if counts else 0, counts=counts, S=S),
            _native_lib=lib, _device=device)
    ph.attach_Ws_and_prox()
    assert ph.batch.nonant.N == k1 + (k2 if counts else 0)
    return ph


def values(rng, shape):
    """mixed sign, magnitudes 1e-3..1e3"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def _put(t, a):
    t.copy_(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel()).to(t.device))


def _get(t):
    return t.detach().cpu().numpy().copy()


def _ratio(got, ref, bound):
    """worst |got - ref| / bound (an entry with a zero bound must be exact)"""
    got, ref, bound = (np.atleast_1d(np.asarray(v)) for v in (got, ref, bound))
    err = np.abs(got - ref).astype(np.float64)      # (ref may be extended precision)
    exact = bound == 0.0
    assert np.all(err[exact] == 0.0), (got[exact], ref[exact])
    r = err[~exact] / bound[~exact]
    return float(r.max()) if r.size else 0.0


def _sum_ref(terms):
    """(fsum, the any-order bound) of a 1-D array of float64 terms"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(t), (t.size + 2) * U * math.fsum(np.abs(t))


# ---------------------------------------------------------------- x-bar
def xbar_reference(xbar_idx, NNS, xn, pc):
    """[sum pc x | sum (pc x) x] per (node, slot) entry over the given
    scenarios: (ref, bound, present) arrays of length 2 NNS."""
    ref = np.zeros(2 * NNS)
    bnd = np.zeros(2 * NNS)
    present = np.zeros(2 * NNS, dtype=bool)
    t1 = pc * xn
    t2 = t1 * xn
    for j in range(xbar_idx.shape[0]):
        idx = xbar_idx[j]
        for e in np.unique(idx):
            m = idx == e
            ref[e], bnd[e] = _sum_ref(t1[j, m])
            ref[NNS + e], bnd[NNS + e] = _sum_ref(t2[j, m])
            present[e] = present[NNS + e] = True
    return ref, bnd, present


def _fill_x_pc(ph, X, PC):
    """the nonant columns of x from X (N, S), the other columns zero; pc from PC"""
    S = ph._S
    x = np.zeros((ph.batch.n, S))
    x[ph.batch.nonant.slot_col] = X
    _put(ph._x, x)
    _put(ph._pc, PC)


def _xbar_call(ph, prefill):
    _put(ph._node_buf, prefill)
    ph.Compute_Xbar()
    return _get(ph._node_buf)


XBAR_CASES = {}
for _S in (1, 2, 63, 64, 65, 1023, 1024):
    for _N in (1, 8):
        XBAR_CASES["one-block-S%d-N%d" % (_S, _N)] = dict(k1=_N, S=_S)
XBAR_CASES.update({
    "one-block-T3u": dict(T3U),
    "one-block-200-nodes": dict(k1=3, k2=1, counts=[1] * 200),           # NNS = 203 <= 237
    # just outside the one-block path
    "S1025-N3": dict(k1=3, S=1025),
    "S64-N9": dict(k1=9, S=64),
    "300-nodes": dict(k1=3, k2=1, counts=[1] * 300),                     # NNS = 303 > 237; thread-per-node fold
    # k_xbar's folds: a ragged last tile of 20, N around XB_CH = 4
    "S1300-N3": dict(k1=3, S=1300),
    "S1300-N4": dict(k1=4, S=1300),
    "S1300-N5": dict(k1=5, S=1300),
    "S1300-N3-tile100": dict(k1=3, S=1300, options={"xbar_tile": 100}),
    "S1300-N4-tile100": dict(k1=4, S=1300, options={"xbar_tile": 100}),
    "S1300-N5-tile100": dict(k1=5, S=1300, options={"xbar_tile": 100}),
    "S1300-N5-tile16": dict(k1=5, S=1300, options={"xbar_tile": 16}),   # 82 tiles > XB_SEQ_TILES: block-reduction fold
    "S1300-N70": dict(k1=70, S=1300),                                    # N >= XB_SEQ_SLOTS
    "S1300-N70-tile16": dict(k1=70, S=1300, options={"xbar_tile": 16}),
    "5-nodes-S1340": dict(k1=3, k2=2, counts=[1, 600, 255, 257, 227]),   # 2..15 nodes, S > 1024
    "20-nodes-S1100": dict(k1=3, k2=2, counts=[1, 299] + [40, 50] * 8 + [30, 50]),   # >= 16 nodes, S > 1024
})


def check_xbar(lib, device, case):
    cfg = dict(XBAR_CASES[case])
    ph = build_ph(lib, device, **cfg)
    N, S, NNS = ph.batch.nonant.N, ph._S, ph.NNS
    rng = np.random.default_rng(1000 + S + 7 * N)
    X, PC = values(rng, (N, S)), rng.uniform(0.05, 1.0, size=(N, S)) / S
    _fill_x_pc(ph, X, PC)
    ref, bnd, present = xbar_reference(ph._xbar_idx, NNS, X, PC)
    assert present.all()
    got = _xbar_call(ph, np.full(2 * NNS, SENTINEL))
    r = _ratio(got[:2 * NNS], ref, bnd)
    print("[xbar %s] S=%d N=%d NNS=%d tiles=%d worst error/bound = %.3g" % (case, S, N, NNS, len(ph._tiles), r))
    assert r <= 1.0, (case, r)
    again = _xbar_call(ph, np.full(2 * NNS, -SENTINEL))
    assert np.array_equal(got, again), case
    return r


SLICE_CASES = {
    # the one-block path: no local scenario for the last node in the first
    # slice, or for the first five in the second
    "T3u": (dict(T3U), [(0, 200), (200, 500)]),
    # k_xbar
    "two-nodes-2x1300": (dict(k1=3, k2=2, counts=[1300, 1300]), [(0, 1300), (1300, 2600)]),
}


def check_xbar_slices(lib, device, case):
    """Each slice as one rank of a multi-rank host loop sees it: node sums of
    absent nodes read exactly zero (PHBase.Compute_Xbar all-reduces the buffer
    in place), also on a second call into the already all-reduced buffer."""
    cfg, slices = SLICE_CASES[case]
    S = int(sum(cfg["counts"]))
    N = cfg["k1"] + cfg["k2"]
    rng = np.random.default_rng(77 + S)
    X, PC = values(rng, (N, S)), rng.uniform(0.05, 1.0, size=(N, S)) / S
    whole = build_ph(lib, device, **cfg)
    NNS = whole.NNS
    gref, gbnd, gpresent = xbar_reference(whole._xbar_idx, NNS, X, PC)
    assert gpresent.all()
    phs, gots, worst = [], [], 0.0
    for lo, hi in slices:
        ph = build_ph(lib, device, lo=lo, hi=hi, **cfg)
        assert ph.NNS == NNS and ph._tree.nnodes_cover < NNS
        _fill_x_pc(ph, X[:, lo:hi], PC[:, lo:hi])
        ref, bnd, present = xbar_reference(ph._xbar_idx, NNS, X[:, lo:hi], PC[:, lo:hi])
        assert not present.all()
        got = _xbar_call(ph, np.full(2 * NNS, SENTINEL))[:2 * NNS]
        assert np.all(got[~present] == 0.0), (
            "slice [%d,%d): node sums of absent nodes are not zero: %s" % (lo, hi, got[~present][:8]))
        worst = max(worst, _ratio(got[present], ref[present], bnd[present]))
        phs.append(ph)
        gots.append(got)
    total = np.sum(gots, axis=0)
    rt = _ratio(total, gref, gbnd)
    print("[xbar slices %s] worst error/bound: slices %.3g, summed over slices %.3g" % (case, worst, rt))
    assert worst <= 1.0 and rt <= 1.0, (case, worst, rt)
    # the second Compute_Xbar of a host loop: the buffer holds the all-reduced sums
    for ph, got in zip(phs, gots):
        again = _xbar_call(ph, total)[:2 * NNS]
        assert np.array_equal(again, got), "stale node sums were kept or re-added"
    return worst, rt


# ---------------------------------------------------------------- Update_W
def uw_reference(ph, X, xbar, Win, rho, segs):
    idx = ph._xbar_idx
    diff = X - xbar[idx]                                   # the kernels' one rounded difference
    d = np.abs(diff)
    ld = np.longdouble
    if np.finfo(ld).nmant >= 63:
        W = Win.astype(ld) + rho.astype(ld) * diff.astype(ld)
    else:
        W = Win + rho * diff
    Wb = 2 * U * (np.abs(Win) + np.abs(rho * diff))
    N = d.shape[0]
    ds = np.array([math.fsum(d[:, s]) for s in range(d.shape[1])])
    dsb = (N + 2) * U * ds
    seg = [_sum_ref(d[:, a:b]) for a, b in segs]
    return dict(W=W, Wb=Wb, dsum=ds, dsumb=dsb, seg=np.array([s[0] for s in seg]),
                segb=np.array([s[1] for s in seg]))


def _update_w(ph, lib, Win_t, W_t, update, dsum_t, segs, seg_t):
    n = len(segs)
    s0 = (_native.c_int32 * max(n, 1))(*[a for a, _ in segs])
    s1 = (_native.c_int32 * max(n, 1))(*[b for _, b in segs])
    return lib.update_w(ph._ctx, ph._x.data_ptr(), ph._xbar_node.data_ptr(), ph._xbar_idx_t.data_ptr(),
                        ph._rho.data_ptr(), Win_t.data_ptr(), W_t.data_ptr(), int(update),
                        dsum_t.data_ptr() if dsum_t is not None else None, n, s0, s1,
                        seg_t.data_ptr() if seg_t is not None else None, ph._stream())


class _UW:
    """One Update_W problem: its PH object, inputs and reference."""

    def __init__(self, lib, device, cfg, segs=None):
        cfg = dict(cfg)
        R = cfg.pop("R", 1)
        opts = dict(cfg.pop("options", None) or {}, conv_ranks=R)
        self.lib = lib
        self.ph = ph = build_ph(lib, device, options=opts, **cfg)
        N, S, NNS = ph.batch.nonant.N, ph._S, ph.NNS
        self.N, self.S, self.NNS = N, S, NNS
        rng = np.random.default_rng(5000 + S + 11 * N + R)
        self.X = values(rng, (N, S))
        self.xbar = values(rng, NNS)
        self.Win = values(rng, (N, S))
        self.rho = rng.uniform(0.1, 10.0, size=(N, S))
        self.segs = list(ph._conv_seg) if segs is None else list(segs)
        _fill_x_pc(ph, self.X, np.ones((N, S)))
        buf = np.full(ph._node_buf.numel(), SENTINEL)
        buf[:NNS] = self.xbar
        _put(ph._node_buf, buf)
        _put(ph._rho, self.rho)
        self.ref = uw_reference(ph, self.X, self.xbar, self.Win, self.rho, self.segs)
        self.worst = {"W": 0.0, "dsum": 0.0, "seg": 0.0}

    def note(self, key, got, ref, bound):
        r = _ratio(got, ref, bound)
        self.worst[key] = max(self.worst[key], r)
        assert r <= 1.0, (key, r)

    def check_seg(self, seg):
        self.note("seg", seg[:len(self.segs)], self.ref["seg"], self.ref["segb"])

    def through_ph(self, update):
        """PHBase._update_w_and_diff (in place, no dsum), twice"""
        ph = self.ph
        outs = []
        for _ in range(2):
            _put(ph._W, self.Win)
            _put(ph._seg_sums, np.full(ph._seg_sums.numel(), SENTINEL))
            ph._update_w_and_diff(update)
            outs.append((_get(ph._W).reshape(self.N, self.S), _get(ph._seg_sums)))
        W, seg = outs[0]
        assert np.array_equal(W, outs[1][0]) and np.array_equal(seg, outs[1][1])
        if update:
            self.note("W", W, self.ref["W"], self.ref["Wb"])
        else:
            assert np.array_equal(W, self.Win), "update_w = 0 wrote W"
        self.check_seg(seg)

    def direct(self, update, in_place, with_dsum, with_segs=True):
        """phx_update_w with the test's own buffers, twice"""
        ph, dev = self.ph, self.ph.device
        outs = []
        for _ in range(2):
            Win_t = torch.empty(self.N * self.S, dtype=torch.float64, device=dev)
            _put(Win_t, self.Win)
            W_t = Win_t if in_place else torch.full_like(Win_t, SENTINEL)
            dsum_t = torch.full((self.S,), SENTINEL, dtype=torch.float64, device=dev) if with_dsum else None
            seg_t = (torch.full((len(self.segs) + 1,), SENTINEL, dtype=torch.float64, device=dev)
                     if with_segs else None)
            rc = _update_w(ph, self.lib, Win_t, W_t, update, dsum_t, self.segs if with_segs else [], seg_t)
            self.lib.check(ph._ctx, rc, "update_w")
            outs.append((_get(Win_t), _get(W_t), None if dsum_t is None else _get(dsum_t),
                         None if seg_t is None else _get(seg_t)))
        for a, b in zip(outs[0], outs[1]):
            assert (a is None and b is None) or np.array_equal(a, b)
        Win, W, dsum, seg = outs[0]
        W = W.reshape(self.N, self.S)
        if not in_place:
            assert np.array_equal(Win.reshape(self.N, self.S), self.Win), "W_in was written"
        if update:
            self.note("W", W, self.ref["W"], self.ref["Wb"])
        else:
            assert np.array_equal(W, self.Win if in_place else np.full_like(W, SENTINEL)), "update_w = 0 wrote W"
        if dsum is not None:
            self.note("dsum", dsum, self.ref["dsum"], self.ref["dsumb"])
        if seg is not None:
            self.check_seg(seg)
            assert seg[len(self.segs)] == SENTINEL

    def report(self, tag):
        print("[update_w %s] S=%d N=%d segments=%s worst error/bound: %s" % (
            tag, self.S, self.N, self.segs if len(self.segs) <= 4 else len(self.segs),
            {k: "%.3g" % v for k, v in self.worst.items()}))
        return self.worst


UW_CASES = {}
for _S in (1, 65, 1024):
    for _N in (1, 8):
        for _R in (1, 3, 8):
            UW_CASES["one-block-S%d-N%d-R%d" % (_S, _N, _R)] = dict(k1=_N, S=_S, R=_R)
UW_CASES["S65-N8-R9"] = dict(k1=8, S=65, R=9)            # nseg > 8 leaves the one-block path
for _N in (3, 8, 9, 15):
    for _R in (1, 3):
        UW_CASES["seg-S1300-N%d-R%d" % (_N, _R)] = dict(k1=_N, S=1300, R=_R)   # bounds 433, 866
for _N in (16, 17, 63, 64, 70):
    for _S in (65, 1300):
        UW_CASES["seg2-S%d-N%d-R3" % (_S, _N)] = dict(k1=_N, S=_S, R=3)
UW_CASES["T3u-R3"] = dict(T3U, R=3)                      # node-indexed xbar_idx
UW_CASES["20-nodes-S1100-R3"] = dict(XBAR_CASES["20-nodes-S1100"], R=3)


def check_update_w(lib, device, case):
    """Update_W and the convergence sums through PHBase._update_w_and_diff
    (update 0 and 1, in place) and through phx_update_w with the test's own
    W_in / W / dsum."""
    c = _UW(lib, device, UW_CASES[case])
    c.through_ph(0)
    c.through_ph(1)
    c.direct(1, in_place=False, with_dsum=False)
    c.direct(1, in_place=True, with_dsum=True)
    c.direct(0, in_place=False, with_dsum=True)
    return c.report(case)


# segments chosen by the test: (tree, segments or None for nseg = 0, do they cover [0, S)?)
UW_DIRECT_CASES = {
    "nseg0-S65": (dict(k1=5, S=65), None, False),
    "nseg0-S1300": (dict(k1=5, S=1300), None, False),
    "empty-middle-S65": (dict(k1=5, S=65), [(0, 30), (30, 30), (30, 65)], True),
    "empty-middle-S1300": (dict(k1=5, S=1300), [(0, 433), (433, 433), (433, 1300)], True),
    "empty-middle-S1300-N20": (dict(k1=20, S=1300), [(0, 433), (433, 433), (433, 1300)], True),
    "not-covering-S65": (dict(k1=5, S=65), [(3, 20), (40, 64)], False),
    "not-covering-S1300": (dict(k1=5, S=1300), [(3, 300), (700, 1299)], False),
    "not-covering-S1300-N20": (dict(k1=20, S=1300), [(3, 300), (700, 1299)], False),
}


def check_update_w_direct(lib, device, case):
    cfg, segs, covering = UW_DIRECT_CASES[case]
    c = _UW(lib, device, cfg, segs=segs if segs is not None else [])
    ws = segs is not None
    c.direct(1, in_place=False, with_dsum=True, with_segs=ws)
    c.direct(1, in_place=True, with_dsum=True, with_segs=ws)
    c.direct(0, in_place=False, with_dsum=True, with_segs=ws)
    if covering:
        c.direct(1, in_place=False, with_dsum=False)
        c.direct(0, in_place=True, with_dsum=False)
    elif ws and c.S <= 1024:
        # the one-block path sums the segments from registers: no dsum needed
        c.direct(1, in_place=False, with_dsum=False)
    elif ws and lib.prefix == "phx_":
        # (the host emulation always keeps its own dsum)
        ph, dev = c.ph, c.ph.device
        Win_t = torch.empty(c.N * c.S, dtype=torch.float64, device=dev)
        _put(Win_t, c.Win)
        W_t = torch.full_like(Win_t, SENTINEL)
        seg_t = torch.full((len(segs),), SENTINEL, dtype=torch.float64, device=dev)
        rc = _update_w(ph, lib, Win_t, W_t, 1, None, segs, seg_t)
        assert rc != 0
        assert b"dsum required when segments do not cover the scenarios" in lib.last_error(ph._ctx)
        assert np.all(_get(W_t) == SENTINEL) and np.all(_get(seg_t) == SENTINEL)
        assert np.array_equal(_get(Win_t).reshape(c.N, c.S), c.Win)
    return c.report(case)


# ---------------------------------------------------------------- expectations
# 263,000 > 256 x 1024: the block count clamps at 256 and the chunk passes 1024
EXPECT_SIZES = (1, 1023, 1024, 1025, 8192, 8193, 263000)
OPTIMAL = 1


def check_expect(lib, device, S):
    ph = PH(ph_options(1), farmer.scenario_names_creator(S), farmer.scenario_creator,
            scenario_creator_kwargs={"num_scens": S}, _native_lib=lib, _device=device)
    assert ph._S == S
    rng = np.random.default_rng(9000 + S)
    p = rng.uniform(0.05, 1.0, size=S)
    p /= p.sum()
    obj = values(rng, S)
    status = rng.integers(1, 5, size=S).astype(np.int32)
    dev = ph.device
    p_t, obj_t = torch.as_tensor(p).to(dev), torch.as_tensor(obj).to(dev)
    st_t = torch.as_tensor(status).to(dev)
    refs = [_sum_ref(p * obj), _sum_ref(p), _sum_ref(np.where(status == OPTIMAL, p, 0.0))]
    outs = []
    for fill in (SENTINEL, -SENTINEL):
        out_t = torch.full((4,), fill, dtype=torch.float64, device=dev)
        lib.check(ph._ctx, lib.expect(ph._ctx, p_t.data_ptr(), obj_t.data_ptr(), st_t.data_ptr(),
                                      out_t.data_ptr(), ph._stream()), "expect")
        outs.append(_get(out_t))
    assert outs[0][3] == SENTINEL and np.array_equal(outs[0][:3], outs[1][:3])
    r = [_ratio(outs[0][k], refs[k][0], refs[k][1]) for k in range(3)]
    print("[expect S=%d] worst error/bound (sum p obj, sum p, sum p [optimal]) = %s" % (
        S, ["%.3g" % v for v in r]))
    assert max(r) <= 1.0, (S, r)
    return r
