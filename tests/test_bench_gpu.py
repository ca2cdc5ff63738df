"""bench.py end to end on the GPU: a plain run prints the headline line alone, and --dump-outputs writes the same outputs run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC = json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"].split(";")[0]  # the headline's metric, verbatim


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args)
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    runs = []
    for k in range(2):
        d = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"run{k}"))
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["metric"] == METRIC and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        # what --full adds is absent from a plain line
        assert "cpu_baseline" not in d and "same_loop_over_200_steps" not in d["config"] and "lpv_gather_copy_rebuilt_every_step" not in d["config"]
        lit = np.load(tmp_path / f"run{k}" / "lit.npy")
        assert lit.dtype == np.float32 and lit.shape == (2 ** 21, 4) and (lit[:, :3] > 0).any()
        runs.append(lit)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


@pytest.mark.gpu
def test_chain_workload_dumps_its_final_image(tmp_path):
    d = _bench("--workload", "4k_probe_gi_chain", "--steps", "2", "--warmup", "1", "--ramp-ms", "0", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and "final-image" in d["metric"]
    img = np.load(tmp_path / "final_image.npy")
    assert img.dtype == np.float32 and img.shape == (2 ** 21, 4)
    assert img.min() >= 0 and img.max() <= 255 and np.array_equal(img, np.round(img)) and img[:, :3].max() > 0
