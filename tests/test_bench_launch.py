"""bench.py's own N-rank launch (the driver's `python bench.py --gpus N` shape): with
no WORLD_SIZE in the environment it starts N ranks itself (torch.distributed.run,
127.0.0.1) before any GPU call.  Run here through the --device cpu test hook (gloo +
the host emulation library): the 2-rank line reports n_gpus = 2 and the same x-bar
and trivial bound as the 1-rank run (scenarios sharded contiguously, one fused
all-reduce per PH iteration)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(n, extra=("--no-conv", "--no-cpu-baseline", "--configs", "none"), tmp=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--device", "cpu", "--scens", "600",
           "--steps", "3", "--warmup", "1", "--ar-probe", "0"] + list(extra)
    if tmp is not None:
        cmd += ["--detail", str(tmp)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # rank 0 prints the one JSON line
    last = r.stdout.rstrip("\n").splitlines()[-1]
    assert last == lines[0]                            # ... as stdout's LAST line
    assert len(last.encode()) <= 8192, len(last.encode())
    return json.loads(last)


def test_bench_line_compact_cpu(tmp_path):
    """The driver parses stdout's last line (<= 8 KB): the contract keys, the roofline,
    the CPU baseline, conv_time and a per-config summary; the full record goes to
    the --detail file."""
    detail = tmp_path / "detail.json"
    d = _bench(1, extra=("--full", "--configs", "C1,C4", "--config-steps", "2", "--cpu-scens", "60", "--cpu-iters", "1",
                         "--cpu-procs", "2", "--conv-max-iters", "50"), tmp=detail)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline",
              "cpu_baseline", "conv_time", "iter0_s", "steady", "configs"):
        assert k in d, k
    assert d["roofline"]["kernel"] and "frac" in d["roofline"] and "traffic_ratio" in d["roofline"]
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 2
    sp = d["cpu_baseline"]["spread"]                 # median of three samples, with their range
    assert sp["samples"] == 3 and sp["min"] <= d["cpu_baseline"]["value"] <= sp["max"]
    for nm in ("C1", "C4"):
        c = d["configs"][nm]
        assert "error" not in c, c
        for k in ("value", "ms_per_step", "frac", "traffic_ratio", "cpu", "avg_launch_us"):
            assert k in c, (nm, k)
    full = json.loads(detail.read_text())
    assert full["configs"]["C4"]["workload"].startswith("aircond")
    assert full["value"] == d["value"] or abs(full["value"] - d["value"]) <= 1e-5 * full["value"]


DUMPED = ["W", "conv", "nonants", "obj", "scenario_index", "status", "trivial_bound", "x", "xbar", "xsqbar"]


def test_bench_plain_run_is_lean_and_dumps_cpu(tmp_path):
    """Without --full the run times its K steps and reports the headline alone: no
    roofline run, conv_time, all-reduce probe, CPU baseline, other configs or detail
    file.  --dump-outputs writes the timed run's final state as float64 .npy files,
    the same from run to run."""
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench(1, extra=("--dump-outputs", str(a)))
    _bench(1, extra=("--dump-outputs", str(b)))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup",
              "steady", "final"):
        assert k in d, k
    for k in ("cpu_baseline", "conv_time", "configs", "allreduce_hook", "detail"):
        assert k not in d, k
    assert d["roofline"] is None
    assert d["steps"] == 3 and d["iterk"]["iters"] == 3
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(600 * 1e3 / d["ms_per_step"], rel=1e-4)
    assert sorted(os.listdir(a)) == [n + ".npy" for n in DUMPED] == sorted(os.listdir(b))
    got = {n: np.load(a / (n + ".npy")) for n in DUMPED}
    for n, x in got.items():
        assert x.dtype == np.float64, n
        assert np.array_equal(x, np.load(b / (n + ".npy")), equal_nan=True), n
    assert sum(x.nbytes for x in got.values()) <= 64e6
    assert np.array_equal(got["scenario_index"], np.arange(600))
    assert got["W"].shape == got["nonants"].shape == (600, 3) and got["x"].shape[0] == 600
    assert got["obj"].shape == got["status"].shape == (600,)
    assert np.allclose(got["xbar"], d["final"]["xbar"]["ROOT"], rtol=1e-12, atol=0)
    assert got["conv"][0] == pytest.approx(d["final"]["conv"], rel=1e-12)
    # W sums to zero over the (equally likely) scenarios; x-bar is the nonants' mean
    assert np.abs(got["W"].sum(axis=0)).max() < 1e-6 * max(1.0, np.abs(got["W"]).max())


def test_dump_outputs_samples_above_cap(tmp_path, monkeypatch):
    """Per-scenario arrays that would not fit the cap keep a fixed sorted sample of
    the scenarios (the same one every time), listed in scenario_index."""
    import bench

    class FakePH:
        conv, trivial_bound, S = 0.5, None, 1000
        x = np.arange(S * 7, dtype=np.float64).reshape(7, S)

        def xbar_by_node(self):
            return {"ROOT": (np.ones(3), 2 * np.ones(3))}

        def W_array(self):
            return -self.x[:3].T

        def nonant_values(self):
            return self.x[:3].T.copy()

        def _host(self, key):
            return {"x": self.x, "obj": self.x[6], "status": np.zeros(self.S, dtype=np.int32)}[key]

    monkeypatch.setattr(bench, "DUMP_CAP", 20000)
    out = bench.dump_outputs(FakePH(), str(tmp_path / "d"))
    idx = out["scenario_index"].astype(int)
    assert 100 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(out["x"], FakePH.x.T[idx]) and np.array_equal(out["W"], -FakePH.x[:3].T[idx])
    assert np.isnan(out["trivial_bound"][0]) and out["conv"][0] == 0.5
    files = os.listdir(tmp_path / "d")
    assert sum(os.path.getsize(tmp_path / "d" / f) for f in files) <= 20000
    again = bench.dump_outputs(FakePH(), None, write=False)
    assert np.array_equal(again["scenario_index"], out["scenario_index"])


def test_bench_launches_ranks_cpu():
    one, two = _bench(1), _bench(2)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["config"]["scenarios"] == 600 and two["config"]["scenarios_per_gpu"] == 300
    assert two["steps"] == 3 and two["value"] > 0
    a, b = one["final"], two["final"]
    assert np.allclose(a["xbar"]["ROOT"], b["xbar"]["ROOT"], rtol=1e-12, atol=1e-12)
    assert abs(a["trivial_bound"] - b["trivial_bound"]) <= 1e-12 * abs(a["trivial_bound"])


def test_compact_line_cap_cpu():
    """whatever the record holds (long error strings, long CPU sample
    text, many configs), the compact line fits LINE_CAP and keeps the contract keys."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    big = "x" * 20000
    res = {"metric": "m", "value": 1.0, "unit": "u", "n_gpus": 1, "steps": 2, "warmup": 1, "ms_per_step": 1.0,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": big,
           "config": {"workload": big}, "roofline": {"kernel": "k", "frac": 0.1, "traffic_ratio": 1.0},
           "cpu_baseline": {"value": 1.0, "unit": "u", "cores": 1, "kind": "port", "sample": big,
                            "whole_host": {"value": 2.0, "how": big, "cap": big},
                            "spread": {"samples": 3, "min": 0.9, "max": 1.1}},
           "configs": {"C%d" % i: {"error": big} for i in range(200)}}
    out = bm.compact_line(res, "detail.json")
    line = json.dumps(out)
    assert len(line.encode()) <= bm.LINE_CAP
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "roofline", "cpu_baseline"):
        assert k in out, k
