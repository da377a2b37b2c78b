"""bench.py's plain run, --full and --dump-outputs on the GPU (a small config-3 workload).

A plain run times the steps and reports the headline figure alone: the fields of the extra
measurements are null, --steps is the number of timed steps and ms_per_step their mean time.
--full measures the rest after the timed steps, so it changes nothing the timed path computed:
both runs dump the same arrays, and a dump is what the engine returns for that batch — the
statuses of a stream are bit-exact against the oracle elsewhere (tests/test_gpu_bench_regime.py).
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
D, STEPS, WARMUP = 50_000, 4, 2
SMALL = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--desc", str(D), "--log2-slots", "20",
         "--batches-per-second", "4", "--prefill", "6"]


def _bench(extra):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py")] + SMALL + extra, capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--full", "--cpu-seconds", "0.2", "--dump-outputs", str(tmp_path / "full")])
    for line in (plain, full):
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["engine"]["batches"] >= 6 + WARMUP + STEPS
        assert line["unit"] == "descriptor decisions/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
        assert line["ms_per_step"] > 0
        # value = descriptors of the timed steps / their time; ms_per_step = that time / steps (rounded to 1e-4 ms)
        assert line["value"] == pytest.approx(D / (line["ms_per_step"] * 1e-3), rel=1e-4 / line["ms_per_step"] + 1e-6)
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["host_path"] is None
    assert plain["table"]["region_live_fraction"] is None
    # the timed steps alone: prefill + warmup + steps batches went through the engine
    assert plain["engine"]["batches"] == 6 + WARMUP + STEPS
    assert full["roofline"]["kernels_us_per_batch"] and full["roofline"]["random_access"]
    assert full["cpu_baseline"]["value"] > 0 and full["host_path"]["value"] > 0
    assert len(full["table"]["region_live_fraction"]) == 8
    a = {f.name: np.load(f) for f in sorted((tmp_path / "plain").iterdir())}
    b = {f.name: np.load(f) for f in sorted((tmp_path / "full").iterdir())}
    assert sorted(a) == sorted(b) == ["status.npy", "throttle_ms.npy"]
    assert a["status.npy"].dtype == np.float64 and a["status.npy"].shape == (D, 5)
    assert a["throttle_ms.npy"].dtype == np.float64 and a["throttle_ms.npy"].shape == (D,)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # every descriptor was decided: code OK (1) or OVER_LIMIT (2) in the low byte of code_flags
    code = a["status.npy"][:, 0].astype(np.uint32) & 0xFF
    assert set(np.unique(code)) <= {1, 2} and (code == 1).any()
