"""The workgroup and generic tiers above 64 active rows (test_wg_sizes.py on the ABI
emulation, test_wg_sizes_gpu.py on the kernels).

The workgroup warm solver (csrc/phx_wg.h) serves every m whose LDS carve fits the
device (phx_kernels.hip: wg_lds_bytes against 163,840 B), but no example model and no
other synthetic family has more than 61 rows, so three parts of it that exist only in
the device build never ran under an assertion: the scalar explicit inverse of L (a
quad per column; Schur complements of more than WG_BLK_MAX = 64 active rows), the
paired-pivot Cholesky's two-thread row groups (more than 64 trailing rows: 67 active
rows or more) and the carve next to the LDS limit.  The generic path (PDHG, the dense
per-lane polish factor, k_ipm) and the sparse solver's dense separator factor were not
run at these sizes either.

The cases are synth_cases.sized_family at seed 1 with other row kinds: a row-kind
list of ["eq"] makes every row an equality, so the active-row count is m in every
round of every lane.  The lane solver is "off: size" throughout (no hipRTC compile).

A trajectory that agrees with the oracle does not show that the workgroup pass works:
a lane it fails to certify goes on to the sparse solver or to PDHG + polish, which
certify it at the same point.  So the condition here is per tier: the number of lanes
the workgroup pass certified in the last solve (check_case, GATE).
"""
import re
import time

import numpy as np

import synth_cases as sc
import test_synth_structures as ts
from helpers import all_certified

SEED, S, ITERS = 1, 70, 4
# Lanes of the last solve (of S = 70) the workgroup pass must have certified: 0.8 S.
# A cap, not a measurement: the emulation certifies 65 (eq65) and 70 (every other
# gated case) there, which leaves 9 lanes for active-set paths that depend on
# rounding; a workgroup pass that is broken for a size certifies none.
GATE = 56
LDS_LIMIT = 163840          # bytes of LDS a workgroup of the MI355X may take


def _case(n, m, rows, nvar=6, ma=None, sep=None, wg=True):
    return dict(spec=dict(sc.sized_family(n, m), rows=list(rows), nvar=nvar), ma=ma, sep=sep, wg=wg)


# ma: (min, max) bound of the rows at a side over the lanes of the last solve: "m" both
# equal to m, else the least count wanted; sep: the sparse solver's separator rows
# (None: it does not serve the pattern; -1: not pinned); wg: the carve fits.
CASES = {
    # control: the last size on the MFMA inverse (WG_BLK_MAX = 64)
    "eq64": _case(140, 64, ["eq"], ma="m", sep=39),
    # the first size on the scalar inverse, an odd count (the Cholesky's tail pivot)
    "eq65": _case(140, 65, ["eq"], ma="m", sep=40),
    # the first count at which the Cholesky takes two-thread row groups
    "eq67": _case(140, 67, ["eq"], ma="m", sep=42),
    # a separator of 61 rows (SP_MAX_C = 64)
    "eq97": _case(200, 97, ["eq"], ma="m", sep=61),
    # A the same in every scenario: the split layout with the shared a_const
    "eq97_nvar0": _case(200, 97, ["eq"], nvar=0, ma="m", sep=-1),
    # no sparse solver: Iter0 on PDHG + the dense polish factor + k_ipm at m = 120
    "eqrange120": _case(200, 120, ["eq", "range", "eq", "le"], ma=67, sep=None),
    # the largest m whose carve fits the LDS limit (163,040 B), and the first that does
    # not (165,168 B): there the generic path serves every solve
    "mix134": _case(200, 134, sc._ALL_ROWS, ma=67, sep=-1),
    "mix135": _case(200, 135, sc._ALL_ROWS, ma=None, sep=-1, wg=False),
}
PATH_CASES = ["eq67", "mix134", "eq97_nvar0"]
NO_WG_CASES = ["eq67", "eq97"]


_HOST = {}                  # (library, case): the host loop's (W, conv, E[obj], trivial bound); not modified


def fam(key):
    return ts.family(CASES[key]["spec"], SEED, S=S)


def wg_lds_bytes(n, m, nnz, split=False):
    """csrc/phx_wg.h wg_lds_bytes, restated: the Schur complement m (m + 1) doubles, four
    row vectors, (all-LDS layout) A's values and four column vectors, the reduction and
    flag words, the 16-bit pattern and active-row lists, the column and row codes."""
    moved = 0 if split else nnz + 4 * n
    idx16 = n + 1 + (1 if split else 3) * nnz + m + 1 + 2 * m
    b = 8 * (m * (m + 1) + 4 * m + moved) + 16 + 64 + 2 * idx16 + n + m
    return (b + 15) & ~15


def rows_at_side(ph, f):
    """Per lane, the rows of the engine's returned x that sit at a side:
    |a'x - b| <= 1e-9 (1 + |b|) for b the lower or the upper side."""
    xT = ph._host("x").T
    act = np.zeros((f.S, f.m))
    np.add.at(act.T, f.rowof, (f.A * xT[:, f.colidx]).T)
    with np.errstate(invalid="ignore"):
        at = ((np.abs(act - f.bl) <= 1e-9 * (1.0 + np.abs(np.where(np.isfinite(f.bl), f.bl, 0.0)))) |
              (np.abs(act - f.bu) <= 1e-9 * (1.0 + np.abs(np.where(np.isfinite(f.bu), f.bu, 0.0)))))
    return at.sum(axis=1)


def per_solve(ph):
    return [(s["wg_certified"], s["sp_certified"], s["pdhg_iters"]) for s in ph.solve_stats]


def check_info(key, f, info, gpu):
    """The info string: the lane solver off by size, the workgroup solver on exactly
    where the carve fits, the separator the case names; on the library the scalar
    Cholesky and the carve's bytes as wg_lds_bytes gives them."""
    c = CASES[key]
    assert info.startswith("off: size"), info
    assert ("workgroup solver on" in info) == c["wg"], info
    sep = re.search(r"sparse solver on: separator (\d+) rows", info)
    if c["sep"] is None:
        assert sep is None, info
    elif c["sep"] >= 0:
        assert sep and int(sep.group(1)) == c["sep"], info
    full = wg_lds_bytes(f.n, f.m, f.nnz)
    assert (full <= LDS_LIMIT) == c["wg"], full
    if c["wg"]:
        assert "factor cache %d B/scenario" % (8 * (f.m * (f.m | 1) + f.m)) in info, info
    if not gpu:
        return
    if c["wg"]:
        split = "(split)" in info
        want = wg_lds_bytes(f.n, f.m, f.nnz, split)
        assert "workgroup solver on: %d B LDS" % want in info, (info, want)
        assert "scalar Cholesky" in info, info
    else:
        assert "workgroup solver off: %d B of LDS per scenario" % full in info, info


def check_case(lib, device, key, gpu=False):
    """One case on the host loop (per-solve statistics): check_beyond_limits (the oracle's
    trajectory at the project's tolerances, every lane certified, none by the lane solver,
    the row duals), host_recheck, then that the case reaches what it names and that the
    workgroup pass certified at least GATE lanes of the last solve -- or, where the carve
    does not fit, that neither it nor the sparse solver certified any lane of any solve."""
    c, f = CASES[key], fam(key)
    t0 = time.perf_counter()
    ph, served = ts.check_beyond_limits(lib, device, f)
    ts.host_recheck(ph, f)
    info = ph._native.jit_info(ph._ctx).decode()
    counts = per_solve(ph)
    at = rows_at_side(ph, f)
    print("%s: n=%d m=%d nnz=%d; %s" % (key, f.n, f.m, f.nnz, info))
    print("%s: rows at a side in the last solve %d..%d; (wg_certified, sp_certified, pdhg iterations) per solve %s"
          % (key, at.min(), at.max(), counts))
    print("%s: host-loop solves %s s; test %.2f s" % (key, ["%.4f" % s["wall_s"] for s in ph.solve_stats],
                                                      time.perf_counter() - t0))
    assert (f.n, f.m) == (c["spec"]["n"], c["spec"]["m"]) and len(counts) == ITERS + 1
    check_info(key, f, info, gpu)
    if c["ma"] == "m":
        assert at.min() == f.m and at.max() == f.m, (at.min(), at.max())
    elif c["ma"]:
        assert at.min() >= c["ma"], at.min()
    if c["wg"]:
        assert counts[ITERS][0] >= GATE, counts
    else:
        assert all(w == 0 and sp == 0 for w, sp, _ in counts), counts
        assert all(it > 0 for _, _, it in counts), counts
    _HOST[(id(lib), key)] = (ph.W_array().copy(),) + tuple(ph.main_result)
    return ph, counts


def _traj(res):
    ph, conv, Eobj, tb = res
    assert all_certified(ph)
    return ph.W_array().copy(), conv, Eobj, tb


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    assert a[1:] == b[1:], (what, a[1:], b[1:])


def check_paths(lib, device, key, monkeypatch, gpu=False):
    """Same arithmetic, other path, bit for bit: the device loop (phx_iterk in workgroup
    mode) against the host loop; the factor cache against a factor recomputed in every
    round; with A the same in every scenario, the split layout against the all-LDS one."""
    f = fam(key)
    t0 = time.perf_counter()
    if (id(lib), key) not in _HOST:                    # (else check_case's run of this process)
        r = ts.run(lib, device, f, ITERS, {"native_loop": 0})
        assert not hasattr(r[0], "iterk_stats") and r[0]._PHIter == ITERS
        _HOST[(id(lib), key)] = _traj(r)
    host = _HOST[(id(lib), key)]
    loop = ts.run(lib, device, f, ITERS)
    assert hasattr(loop[0], "iterk_stats") and loop[0]._PHIter == ITERS
    info = loop[0]._native.jit_info(loop[0]._ctx).decode()
    assert "factor cache" in info, info
    _same(_traj(loop), host, "device loop")
    monkeypatch.setenv("PHX_WG_NO_FACTOR_CACHE", "1")
    nocache = ts.run(lib, device, f, ITERS)
    monkeypatch.delenv("PHX_WG_NO_FACTOR_CACHE")
    info_nc = nocache[0]._native.jit_info(nocache[0]._ctx).decode()
    assert "workgroup solver on" in info_nc and "factor cache" not in info_nc, info_nc
    _same(_traj(nocache), _traj(loop), "no factor cache")
    if f.flags["nvar"] == 0:
        if gpu:
            # the automatic layout: split (two workgroups per CU instead of one)
            assert "(split)" in info, info
        for v in ("0", "1"):
            monkeypatch.setenv("PHX_WG_SPLIT", v)
            r = ts.run(lib, device, f, ITERS)
            monkeypatch.delenv("PHX_WG_SPLIT")
            inf = r[0]._native.jit_info(r[0]._ctx).decode()
            print("%s: PHX_WG_SPLIT=%s: %s" % (key, v, inf))
            if gpu:
                assert ("(split)" in inf) == (v == "1"), inf
                assert "workgroup solver on: %d B LDS" % wg_lds_bytes(f.n, f.m, f.nnz, v == "1") in inf, inf
            _same(_traj(r), _traj(loop), "PHX_WG_SPLIT=" + v)
    print("%s: device loop %s; test %.2f s" % (key, {k: loop[0].iterk_stats.get(k) for k in ("iters", "wall_s")},
                                               time.perf_counter() - t0))


def check_no_wg(lib, device, key):
    """wg_warm 0: the sparse solver alone (its dense separator factor at 42 and 61 rows)
    on the oracle's trajectory."""
    f = fam(key)
    t0 = time.perf_counter()
    ph, served = ts.check_beyond_limits(lib, device, f, {"wg_warm": 0})
    ts.host_recheck(ph, f)
    counts = per_solve(ph)
    print("%s wg_warm 0: %s; per solve %s; host-loop solves %s s; test %.2f s"
          % (key, ph._native.jit_info(ph._ctx).decode(), counts, ["%.4f" % s["wall_s"] for s in ph.solve_stats],
             time.perf_counter() - t0))
    assert served["wg_certified"] == 0 and served["sp_certified"] > 0, served
