"""bench.py without --full: the headline only (set-up, pre-warm, W warm-up steps, exactly K timed steps, the line), and
--dump-outputs, which writes what the K timed steps computed.  No GPU here: --dry-run-device replaces the arena by a
counter whose state is a function of its step count, so the structure of the line and of the dump is what is checked."""
import json
import os

import numpy as np

from test_bench_multirank import one_json_line, run_bench

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype")
FULL_ONLY = ("default_form", "cpu_baseline", "ensemble")


def test_plain_line_is_the_headline_only(tmp_path):
    d = one_json_line(run_bench("--gpus", "1", "--steps", "37", "--warmup", "5", "--dry-run-device", "--detail",
                                str(tmp_path / "d.json")))
    for k in CONTRACT:
        assert k in d, k
    assert d["steps"] == 37 and d["warmup"] == 5 and d["roofline"]["launches"] == 37
    assert d["unit"] == "particle-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - d["config"]["bots_per_gpu"] * 37 / (d["ms_per_step"] * 37 * 1e-3)) / d["value"] < 1e-9
    for k in FULL_ONLY:
        assert k not in d, k
    assert "long" not in d["roofline"]     # (the dry-run region is 3 ms: --full would add the >= 100 ms one)
    long = json.loads((tmp_path / "d.json").read_text())
    assert set(long["phases_end_s"]) == {"headline"} and long["outputs"] is None


def test_full_line_carries_every_leg():
    d = one_json_line(run_bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--dry-run-device", "--full",
                                "--bots", "20000", "--cpu-seconds", "0.2", "--e2e-steps", "20", "--detail", ""))
    for k in CONTRACT + FULL_ONLY:
        assert k in d, k
    assert d["steps"] == 20 and d["roofline"]["launches"] == 20 and d["roofline"]["long"]["steps"] > 0


def test_dump_outputs_are_the_timed_steps_and_repeat(tmp_path):
    """The dump is the state after the W + K steps, float32, and the same arguments give the same files."""
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        d = one_json_line(run_bench("--steps", "20", "--warmup", "5", "--bots", "3000", "--dry-run-device",
                                    "--dump-outputs", str(out), "--detail", ""))
        assert d["steps"] == 20
        runs.append({f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = runs
    assert set(a) == {"pos", "vel", "rad", "phase", "dead", "absForce_a", "absForce_r"}
    for k in a:
        assert a[k].dtype == np.float32 and len(a[k]) == 3000, k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # the dry-run arena's radius is its clock: 25 steps of 0.01
    assert np.all(a["rad"] == np.float32(0.01 * 25))


def test_dump_of_a_large_state_is_a_fixed_sample_under_64_mb(tmp_path):
    import bench
    n = 3_000_000
    rng = np.random.default_rng(7)
    st = {"pos": rng.random((n, 2), np.float32), "vel": rng.random((n, 2), np.float32), "rad": rng.random(n, np.float32),
          "phase": rng.random(n, np.float32), "dead": np.zeros(n, np.int32), "absForce_a": None,
          "absForce_r": rng.random(n, np.float32)}
    w1 = bench.dump_outputs(st, str(tmp_path / "a"))
    w2 = bench.dump_outputs(st, str(tmp_path / "b"))
    assert w1 == w2 and "absForce_a" not in w1 and "bot_index" in w1
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert 32e6 < total <= 64e6
    idx = np.load(tmp_path / "a" / "bot_index.npy").astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(idx, np.load(tmp_path / "b" / "bot_index.npy").astype(np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "pos.npy"), st["pos"][idx])
    assert np.array_equal(np.load(tmp_path / "a" / "dead.npy"), np.zeros(len(idx), np.float32))
