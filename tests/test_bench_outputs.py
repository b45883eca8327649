"""bench.py --dump-outputs and the plain / --full split.  A plain run sets up, warms up, times --steps steps, writes
the last step's results when asked and prints the headline line; everything measured beside the headline (roofline,
encoder / log-mel / VAD replays, streaming latencies, CPU baseline) is behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "decode_mode", "encoder", "logmel", "vad", "stream_latency", "stream_load", "cpu_baseline")
NAMES = ["avg_logprob", "jump_times", "language", "language_prob", "n_tokens", "no_speech_prob", "seek_frames",
         "sum_logprob", "text_token_probs", "tokens"]


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_every_field_as_float32(tmp_path):
    from wmx.engine import WindowResult
    res = [WindowResult([50258, 50259, 7, 9], 50259, 0.75, -3.5, -0.875, 0.125, 3000,
                        np.array([0.0, 0.5, 1.25], np.float32), np.array([0.5, 0.25], np.float32)),
           WindowResult([50258], 50260, 0.5, -1.0, -1.0, 0.9, 1500, None, None)]
    d = str(tmp_path / "o")
    assert _bench().dump_outputs(d, res, 6) == NAMES
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["tokens"].tolist() == [[50258, 50259, 7, 9, -1, -1], [50258, -1, -1, -1, -1, -1]]
    assert got["n_tokens"].tolist() == [4, 1] and got["language"].tolist() == [50259, 50260]
    assert got["jump_times"].shape == (2, 7) and got["jump_times"][0, :4].tolist() == [0.0, 0.5, 1.25, -1.0]
    assert np.all(got["jump_times"][1] == -1) and np.all(got["text_token_probs"][1] == -1)
    assert got["text_token_probs"][0, :3].tolist() == [0.5, 0.25, -1.0]
    assert got["sum_logprob"].tolist() == [-3.5, -1.0] and got["seek_frames"].tolist() == [3000, 1500]
    # ranks above 0 write beside rank 0's files, never over them
    _bench().dump_outputs(d, res[:1], 6, world=2, rank=1)
    assert np.load(os.path.join(d, "tokens.rank1.npy")).shape == (1, 6)
    assert np.load(os.path.join(d, "tokens.npy")).shape == (2, 6)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout.strip() == "", (r.returncode, r.stdout)


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only_and_dumps_the_last_step(tmp_path):
    """One plain run at micro dims: the line carries the headline fields and none of the --full figures, --steps is
    the number of timed steps, and the dumped arrays are the B windows' results."""
    d = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if not k.startswith("WMX_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--model", "micro", "--dtype", "f16", "--batch", "2", "--max-new-tokens", "8",
                        "--dump-outputs", d], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE) and not any(k in out for k in FULL_ONLY), sorted(out)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False and out["dtype"] == "f16"
    assert out["ms_per_step"] > 0 and out["higher_is_better"] is True
    # value = audio seconds of the timed steps / their wall time, and ms_per_step is that wall time per step
    assert out["value"] == pytest.approx(30.0 * 2 / (out["ms_per_step"] * 1e-3), rel=1e-2)
    assert out["dumped_outputs"] == NAMES and sorted(os.listdir(d)) == [n + ".npy" for n in NAMES]
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 and a.shape[0] == 2 for a in got.values())
    for k in ("language_prob", "no_speech_prob"):
        assert np.all((got[k] >= 0) & (got[k] <= 1)), (k, got[k])
    n = got["n_tokens"].astype(int)
    assert np.all(n >= 0) and np.all(n <= 8)
    for b in range(2):
        assert np.all(got["tokens"][b, :n[b]] >= 0) and np.all(got["tokens"][b, n[b]:] == -1)
