"""PHX_XBAR_FROM_TILES=1 (phx_iterk, one rank, few tree nodes: k_xbar leaves its
tile partials and Update_W folds them itself) against the default mode.

The variable is read once per process, so each mode runs in a fresh child
Python process (this file run as a script) under its own time limit:

* farmer crops_multiplier=10, S = 60: N = 30 nonants, one node, the unfused
  device loop -- the size at which Update_W would take k_update_w_seg2, which
  does not fold the tiles (from-tiles mode keeps k_update_w_seg there);
* farmer S = 2000 with iterk_fused=0: N = 3, k_update_w_seg in both modes.

Same tile partials, same fold order (xbar_fold_all in k_xbar's last block or
in Update_W's blocks): x-bar and W are expected bit for bit.  At N = 30 the
convergence sums come from another kernel (k_update_w_seg sums a tile's 30
slots per thread, k_update_w_seg2 per chunk of 8), so conv is held to 1e-12
relative there (measured on the MI355X: bit-equal as well) and bit for bit at
N = 3.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 4
RUNS = {
    # name: (S, scenario creator kwargs, iterk solver options)
    "cm10-S60-N30": (60, {"crops_multiplier": 10}, {"native_loop": 1}),
    "S2000-N3-unfused": (2000, {}, {"native_loop": 1, "iterk_fused": 0}),
}


def _child(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mpisppy_amd  # noqa: F401
    from mpisppy_amd import _native
    from mpisppy_amd.examples import farmer
    from helpers import run_engine
    res = {}
    for name, (S, kw, iterk) in RUNS.items():
        ph, conv, Eobj, tb = run_engine(farmer.scenario_creator, farmer.scenario_names_creator(S),
                                        dict(kw, num_scens=S), ITERS, lib=_native.load(), device="cuda:0",
                                        options={"convthresh": 1e-10, "iterk_solver_options": iterk})
        st = ph.iterk_stats
        assert not st["fused"] and st["not_optimal"] == 0, st
        res[name + "/W"] = ph.W_array()
        res[name + "/xbar"] = ph.xbar_by_node()["ROOT"][0]
        res[name + "/xsqbar"] = ph.xbar_by_node()["ROOT"][1]
        res[name + "/conv"] = np.array([conv])
        res[name + "/iters"] = np.array([ph._PHIter])
        res[name + "/N"] = np.array([ph.batch.nonant.N])
    np.savez(out_path, **res)


def _run_child(out_path, from_tiles):
    env = dict(os.environ)
    env.pop("PHX_XBAR_FROM_TILES", None)
    if from_tiles:
        env["PHX_XBAR_FROM_TILES"] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out_path]
    subprocess.run(cmd, env=env, check=True, timeout=240)
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_xbar_from_tiles_matches_default_gpu(gpu_lib, tmp_path):
    base = _run_child(str(tmp_path / "default.npz"), False)
    tiles = _run_child(str(tmp_path / "from_tiles.npz"), True)
    assert int(base["cm10-S60-N30/N"][0]) == 30 and int(base["S2000-N3-unfused/N"][0]) == 3
    for name in RUNS:
        d = {k: _rel(tiles["%s/%s" % (name, k)], base["%s/%s" % (name, k)]) for k in ("W", "xbar", "xsqbar", "conv")}
        print("[from-tiles %s] iterations %d / %d, max rel diff vs default: %s" % (
            name, tiles[name + "/iters"][0], base[name + "/iters"][0], d))
        assert tiles[name + "/iters"][0] == base[name + "/iters"][0] == ITERS
        for k in ("W", "xbar", "xsqbar"):
            assert np.array_equal(tiles["%s/%s" % (name, k)], base["%s/%s" % (name, k)]), (name, k, d)
        if int(base[name + "/N"][0]) < 16:
            assert np.array_equal(tiles[name + "/conv"], base[name + "/conv"]), (name, d)
        assert d["conv"] <= 1e-12, (name, d)


if __name__ == "__main__":
    _child(sys.argv[1])
