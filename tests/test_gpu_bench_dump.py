"""GPU: a plain `bench.py` run and `--dump-outputs`.  A plain run times the
steps and leaves out what `--full` adds; `--dump-outputs DIR` writes what the
last timed step left in the output ring as float32 rows of 4 KiB blocks: the
whole ring when it is small, a fixed choice of blocks when it is large (here a
5 GiB ring, so kept blocks lie past byte 2^32).  Both are checked byte for
byte against the C oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _run(args, out_dir, timeout=240):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)] + args
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_dumps_whole_small_ring(tmp_path, oracle):
    n, size = 64, 64 << 10
    j = _run(["--config", "8", "--objects", str(n), "--steps", "3", "--warmup", "1"], tmp_path)
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "GiB/s" and j["dtype"] == "u8" and j["higher_is_better"] is True
    # what --full adds is not run
    assert j["verified_vs_oracle"] is None and j["cpu_baseline"] is None and j["d2h_inclusive"] is None
    assert "store_only_best_GBps" not in j["roofline"]
    assert os.listdir(tmp_path) == ["ring.npy"]
    got = np.load(tmp_path / "ring.npy")
    assert got.dtype == np.float32 and got.shape == (n * size // 4096, 4096)
    exp = oracle.fill_stream(size, n, 1, 0, 1, bench.SEED_BASE, 0, oracle.base_block(bench.BASE_SEED))
    assert np.array_equal(got.astype(np.uint8).ravel(), exp)


def test_dump_samples_large_ring(tmp_path, oracle):
    n, size = 640, 8 << 20
    j = _run(["--config", "2", "--objects", str(n), "--steps", "1", "--warmup", "0"], tmp_path)
    nb = n * size // bench.DUMP_BLOCK
    idx = bench.dump_blocks(nb, bench.DUMP_BUDGET)
    assert j["dumped_outputs"]["files"] == {"ring.npy": {"blocks": len(idx), "of": nb}}
    got = np.load(tmp_path / "ring.npy")
    assert got.dtype == np.float32 and got.shape == (len(idx), 4096) and got.nbytes <= 64 * 10**6
    assert idx[-1] * bench.DUMP_BLOCK > 1 << 32
    base = oracle.base_block(bench.BASE_SEED)
    per = size // bench.DUMP_BLOCK
    # the first and the last kept block, and a few between, each against its whole object
    for row in (0, 1, len(idx) // 2, len(idx) - 2, len(idx) - 1):
        obj, blk = divmod(idx[row], per)
        exp = oracle.fill_controlled(size, 1, 0, 1, bench.object_entropy_py(bench.SEED_BASE, obj), base)
        assert np.array_equal(got[row].astype(np.uint8), exp[blk * 4096:(blk + 1) * 4096]), (row, obj, blk)
