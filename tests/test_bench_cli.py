"""bench.py's launcher contract on the CPU (no GPU is touched on these paths):
* under a launcher, WORLD_SIZE must equal --gpus (else a non-zero exit before any work);
* --gpus N without a launcher spawns N child ranks with RANK / LOCAL_RANK / WORLD_SIZE set and
  exits non-zero when a rank fails (here cfg5, a single-GPU workload, refuses WORLD_SIZE=2 in
  each child before importing torch)."""
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=120)


def test_world_size_mismatch_exits_nonzero():
    r = _run(["--gpus", "4", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "does not match WORLD_SIZE=2" in r.stderr
    assert r.stdout == ""


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: float32 stays float32, ids and fp64 scores go out as float64, and an array
    above its share of the budget is cut to the same seeded, sorted row sample on every run."""
    import numpy as np

    import bench  # (the repository root is on sys.path: tests/conftest.py)

    D = np.arange(12, dtype=np.float32).reshape(4, 3)
    I = np.array([[2 ** 40 + 1, 5, 7]] * 4, dtype=np.int64)
    bench._dump_outputs(str(tmp_path / "a"), {"D": D, "I": I, "S": D.astype(np.float64)})
    d, i, s = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("D", "I", "S"))
    assert d.dtype == np.float32 and np.array_equal(d, D)
    assert i.dtype == np.float64 and np.array_equal(i.astype(np.int64), I)
    assert s.dtype == np.float64 and np.array_equal(s, D)

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 40 * 8)  # two arrays: 40 fp64 values each
    big = np.arange(1000, dtype=np.float64).reshape(100, 10)
    for sub in ("b", "c"):
        bench._dump_outputs(str(tmp_path / sub), {"S": big, "D": D})
    sb, sc = np.load(tmp_path / "b" / "S.npy"), np.load(tmp_path / "c" / "S.npy")
    assert sb.shape == (4, 10) and np.array_equal(sb, sc)
    assert np.all(np.diff(sb[:, 0]) > 0) and all(np.array_equal(r, big[int(r[0]) // 10]) for r in sb)
    assert np.array_equal(np.load(tmp_path / "b" / "D.npy"), D)


def test_plain_and_full_options_parse(monkeypatch):
    import bench  # (the repository root is on sys.path: tests/conftest.py)

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x"


def test_spawned_ranks_see_the_world_and_failures_propagate():
    r = _run(["--gpus", "2", "--workload", "cfg5"])
    assert r.returncode != 0
    # the children ran with WORLD_SIZE=2 and refused it (the parent stops the other rank once one
    # has failed, so it may not get to print)
    assert r.stderr.count("cfg5 is a single-GPU workload") >= 1, r.stderr
    assert r.stdout == ""
