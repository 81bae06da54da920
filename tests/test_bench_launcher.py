"""bench.py's multi-rank launcher and timing protocol on the CPU (gloo, --dry-run): `--gpus 2`
without a torch.distributed environment starts two ranks as child processes and rank 0 prints one
JSON line with n_gpus = 2 (the driver's N>1 runs use the same path under torch.distributed.run)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_launcher_two_ranks():
    line = _run("--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1")
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["scaling"] == "strong"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # BASELINE config 3: ONE 3M-impression set sharded over the ranks, contiguous and complete
    assert line["config"]["global_batch"] == 3_000_000
    assert [tuple(s) for s in line["config"]["shards"]] == [(0, 1_500_000), (1_500_000, 1_500_000)]


def test_single_rank_default():
    line = _run("--dry-run", "--steps", "2", "--warmup", "0")
    assert line["n_gpus"] == 1
    assert line["config"]["global_batch"] == 3_000_000


def test_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last step's output as float .npy, identical from run to run;
    --steps sets the timed steps (also as --steps=N) and --full is accepted."""
    import numpy as np
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    la = _run("--gpus", "1", "--dry-run", "--steps=4", "--warmup", "1", "--dump-outputs", a)
    lb = _run("--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "0", "--full", "--dump-outputs", b)
    assert la["steps"] == 4 and la["warmup"] == 1 and lb["steps"] == 2 and lb["warmup"] == 0
    assert la["ms_per_step"] > 0 and lb["ms_per_step"] > 0
    assert os.listdir(a) == ["product.npy"] == os.listdir(b)
    xa, xb = np.load(os.path.join(a, "product.npy")), np.load(os.path.join(b, "product.npy"))
    assert xa.dtype == np.float32 and xa.shape == (64, 64) and np.isfinite(xa).all()
    assert np.array_equal(xa, xb)


def test_dump_outputs_samples_large_arrays(tmp_path):
    """An array past its share of the 64 MB cap is written as the same seeded rows, in row order."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(3_000_000, dtype=torch.float32)[:, None].expand(-1, 40)      # 480 MB if written whole
    idx = torch.arange(1000, dtype=torch.int64).reshape(10, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"scores": big, "index": idx})
    sa, sb = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "b" / "scores.npy")
    assert sa.dtype == np.float32 and sa.shape[1] == 40 and 100_000 < sa.shape[0] < 3_000_000
    assert np.array_equal(sa, sb) and (np.diff(sa[:, 0]) > 0).all() and (sa == sa[:, :1]).all()
    ia = np.load(tmp_path / "a" / "index.npy")
    assert ia.dtype == np.float64 and np.array_equal(ia, idx.numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000
