"""bench.py's command line on a small code (hgp_34_n225, 2048 shots per step).

* A plain run times exactly ``--steps`` launches, prints one JSON line with the headline keys and
  nothing that takes runs of its own; ``--dump-outputs`` writes the counters the timed launches
  returned, equal word for word to the same shot blocks run through ``DeviceMC.run``.
* ``--full`` adds the fp32 line and the CPU baseline (the PMC passes are switched off here: they
  start rocprofv3 three times).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE, S, K, W = "hgp_34_n225", 2048, 3, 1


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--code", CODE, "--shots", str(S), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == W and d["n_gpus"] == 1
    assert d["unit"] == "shots/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(S / (d["ms_per_step"] * 1e-3), rel=1e-9)
    return d


def test_plain_run_is_lean_and_dumps_the_timed_counters(gpu, tmp_path):
    import bench
    from qldpc_fault_tolerance_amd import codes
    from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceMC

    out = tmp_path / "o"
    d = _bench("--dump-outputs", str(out))
    assert "cpu_baseline" not in d and "fp32_fast_mode" not in d
    assert d["roofline"]["traffic"] is None and d["roofline"]["hbm"]["pmc"] is None
    assert sorted(os.listdir(out)) == ["counters.npy", "counters_last_step.npy"]
    cnt, last = np.load(out / "counters.npy"), np.load(out / "counters_last_step.npy")
    assert cnt.dtype == np.float64 and last.dtype == np.float64

    # the same global shot blocks (steps W .. W+K-1 of S shots, bench.SEED) through DeviceMC.run
    code = codes.get_code(CODE)
    n, p = code.N, bench.DEFAULT_P
    dx = DeviceBP(code.hz, p * np.ones(n), max_iter=int(n / 10), ms_scaling_factor=0.625, precision=64)
    dz = DeviceBP(code.hx, p * np.ones(n), max_iter=int(n / 10), ms_scaling_factor=0.625, precision=64,
                  vars_per_thread=dx.geometry()["vars_per_thread"])
    mc = DeviceMC(code, dx, dz)
    words = [bench.result_words(mc.run(*bench.pauli_probs(p), bench.SEED, (W + i) * S, S, "Total")) for i in range(K)]
    assert last[0] == S and cnt[0] == S * K
    assert np.array_equal(last, words[-1])
    assert np.array_equal(cnt, np.sum(words, axis=0))


def test_full_run_adds_the_fp32_line_and_the_cpu_baseline(gpu):
    d = _bench("--full", "--pmc-traffic", "0", "--cpu-seconds", "0.2")
    assert d["fp32_fast_mode"]["value"] > 0 and d["fp32_fast_mode"]["unit"] == "shots/s"
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "shots/s"
