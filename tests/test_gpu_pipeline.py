"""The pipelined resnet play loop (two half-pools on two streams) plays the same games as the one-stream
loop: bench.py --dump-outputs of the headline under AZX_PIPELINE=0 and =1, each in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SUMS = [i for i, k in enumerate(bench.DUMP_COUNTERS) if k.startswith("sum_") and k not in
        ("sum_depth", "sum_k_interior", "sum_k_leaf")]


def _dump(tmp_path, pipeline, *args):
    out = tmp_path / ("pipe%d" % pipeline)
    env = dict(os.environ, AZX_PIPELINE=str(pipeline))
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1",
           "--dump-outputs", str(out), *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=660)
    assert r.returncode == 0, (pipeline, r.returncode, r.stderr.decode()[-2000:])
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    return out, lines[0]


def _same_games(tmp_path, *args):
    a, line_a = _dump(tmp_path, 0, *args)
    b, line_b = _dump(tmp_path, 1, *args)
    assert "one stream" in line_a and "AZX_PIPELINE=0" in line_a
    assert "two half-pools on two streams" in line_b and "AZX_PIPELINE=1" in line_b
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert "game_slots.npy" in names and "play_counters.npy" in names and any(n.startswith("root_") for n in names)
    assert names == sorted(f for f in os.listdir(b) if f.endswith(".npy"))
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.shape == y.shape, n
        if n == "play_counters.npy":
            ints = [i for i in range(len(x)) if i not in SUMS]
            assert np.array_equal(x[ints], y[ints]), (n, x, y)
            # per-game accumulators summed on the host in slot order: exact in practice, 1e-12 allowed
            np.testing.assert_allclose(y[SUMS], x[SUMS], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), n
    c = np.load(os.path.join(a, "play_counters.npy"))
    assert c[bench.DUMP_COUNTERS.index("plies")] > 0 and c[bench.DUMP_COUNTERS.index("evals")] > 0


def test_pipelined_headline_plays_the_same_games(tmp_path):
    """Default sizes (4096 games, 11x11, 400 simulations, 6x64 tower)."""
    _same_games(tmp_path)


def test_pipelined_small_pool_plays_the_same_games(tmp_path):
    """The smallest pool the pipelined loop takes (1024 games)."""
    _same_games(tmp_path, "--games", "1024")
