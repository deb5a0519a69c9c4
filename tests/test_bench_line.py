"""What a plain ``bench.py`` run prints: the headline and its configuration, nothing measured beside it (that is ``--full``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
# fields that only ``--full`` measures (N = 1)
FULL_ONLY = ("latency_ms_p50", "latency_ms_p95", "value_one_frame_at_a_time", "roofline", "roofline_stages", "fp32_hip_path",
             "multi_agent_one_gpu", "pyramid_model", "second_encoder", "encode_modes", "points_to_boxes", "codebook_seg2_dict256",
             "rehearsal", "sharded_world1", "cpu_baseline", "parity", "cpu_baseline_torch")


@pytest.mark.parametrize("flag", ["--no-extras", "--no-cpu-baseline"])
def test_full_line_trims_need_full(flag):
    """``--no-extras`` / ``--no-cpu-baseline`` only trim the ``--full`` line: without ``--full`` they are refused, not ignored."""
    r = subprocess.run([sys.executable, BENCH, "--steps", "2", flag], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    """A plain run: set-up, warm-up, the timed steps, ``--dump-outputs``, one line whose ``value`` is the frames of the timed steps over
    their time (``ms_per_step``), and none of the fields ``--full`` measures."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "frames/sec/node (N-agent int8 BEV fusion)" and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "i8" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    frames = line["config"]["frames_per_step"]
    assert frames == 32 and line["value"] == pytest.approx(frames * 1e3 / line["ms_per_step"], rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    preds = np.load(out / "preds_tensor.npy")
    assert preds.size > 0 and np.isfinite(preds).all()
