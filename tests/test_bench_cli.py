"""bench.py's command line: a plain run is the headline alone, ``--full`` adds the extra points, ``--dump-outputs``
writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY_KEYS = {"ttft_ms", "decode_ms_per_token", "latency_points", "ttft", "sampled", "tp_rank_proxy", "mp1_point",
                  "calibration", "tp_points"}


def test_dump_outputs_float32_named_by_rank(tmp_path):
    seq = torch.arange(6 * 5, dtype=torch.int32).reshape(6, 5) * 20000  # token-id sized values
    bench._dump_outputs(str(tmp_path / "d"), {"sequences": seq}, rank=0, world=1)
    bench._dump_outputs(str(tmp_path / "d"), {"sequences": seq + 1}, rank=1, world=2)
    got = np.load(tmp_path / "d" / "sequences.npy")
    assert got.dtype == np.float32 and got.shape == (6, 5)
    assert np.array_equal(got, seq.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "sequences_rank1.npy"), (seq + 1).numpy().astype(np.float32))


def test_dump_outputs_samples_rows_beyond_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 8 * 10)  # room for 10 rows of 8 float32
    seq = torch.arange(64 * 8, dtype=torch.int32).reshape(64, 8)
    bench._dump_outputs(str(tmp_path / "a"), {"sequences": seq}, rank=0, world=1)
    bench._dump_outputs(str(tmp_path / "b"), {"sequences": seq}, rank=0, world=1)
    a, b = np.load(tmp_path / "a" / "sequences.npy"), np.load(tmp_path / "b" / "sequences.npy")
    assert a.shape == (10, 8) and a.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(a, b)  # the same rows every time
    rows = (a[:, 0] // 8).astype(int)
    assert len(set(rows)) == 10 and np.array_equal(a, seq.numpy()[rows].astype(np.float32))  # whole rows of the input


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_tokens(tmp_path):
    """One layer at the Llama-3-8B shapes, 8 rows: --steps sets the timed steps, the result line carries ms_per_step and
    none of the --full keys, and the dump is the [batch, prompt + generated] token matrix starting with the seeded
    prompts."""
    env = dict(os.environ, JLA_TUNE_FILE=str(tmp_path / "tune.json"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--layers", "1", "--batch", "8", "--prompt-len", "16", "--gen-len", "8",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert HEADLINE_KEYS <= set(res) and not (FULL_ONLY_KEYS & set(res))
    assert res["metric"] == "output_tokens_per_sec" and res["unit"] == "tokens/s" and res["higher_is_better"] is True
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(8 * 8 * 1000.0 / res["ms_per_step"], rel=1e-3)
    assert r.stderr.count("timed step") == 2 and "side point" not in r.stderr
    seq = np.load(tmp_path / "out" / "sequences.npy")
    assert seq.dtype == np.float32 and seq.shape == (8, 24)
    prompts = torch.randint(3, 128256, (8, 16), generator=torch.Generator().manual_seed(100), dtype=torch.int32)
    assert np.array_equal(seq[:, :16], prompts.numpy().astype(np.float32))
    assert (seq >= 0).all() and (seq < 128256).all() and np.array_equal(seq, np.round(seq))
