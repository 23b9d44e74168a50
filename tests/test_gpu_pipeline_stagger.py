"""The stagger of the pipelined play loop (in every move half B's first full evaluation waits until half of
half A's is done, half A's being issued as two sub-launches) changes when launches run, not what they compute: every
game is bit for bit what AZX_PIPELINE_STAGGER=0 and the one-stream loop (AZX_PIPELINE=0) play.  Every run is a fresh
child process (the switches are read once, by azx_create); every comparison is byte for byte."""
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

# (AZX_PIPELINE, AZX_PIPELINE_STAGGER): staggered, today's start, one stream
MODES = {"staggered": ("1", "1"), "together": ("1", "0"), "one_stream": ("0", "1")}
STAGGERED_PLAY = "two half-pools on two streams half an evaluation apart"


def _env(mode):
    pipeline, stagger = MODES[mode]
    return dict(os.environ, AZX_PIPELINE=pipeline, AZX_PIPELINE_STAGGER=stagger)


def _bench_dump(tmp_path, mode, *args):
    out = tmp_path / mode
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out), *args]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(mode), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=660)
    assert r.returncode == 0, (mode, r.returncode, r.stderr.decode()[-2000:])
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    return out, json.loads(lines[0])


def _same_dumps(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert "game_slots.npy" in names and "play_counters.npy" in names and any(n.startswith("root_") for n in names)
    assert names == sorted(f for f in os.listdir(b) if f.endswith(".npy"))
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.shape == y.shape and x.dtype == y.dtype, n
        assert x.tobytes() == y.tobytes(), n


def _same_games(tmp_path, *args):
    dumps = {mode: _bench_dump(tmp_path, mode, *args) for mode in MODES}
    kernels = {mode: line["kernels"] for mode, (_, line) in dumps.items()}
    assert STAGGERED_PLAY in kernels["staggered"] and "AZX_PIPELINE=1 AZX_PIPELINE_STAGGER=1" in kernels["staggered"]
    assert "two half-pools on two streams;" in kernels["together"] and "AZX_PIPELINE=1 AZX_PIPELINE_STAGGER=0" in kernels["together"]
    assert "one stream" in kernels["one_stream"] and "AZX_PIPELINE=0" in kernels["one_stream"]
    c = np.load(os.path.join(dumps["staggered"][0], "play_counters.npy"))
    assert c[bench.DUMP_COUNTERS.index("plies")] > 0 and c[bench.DUMP_COUNTERS.index("evals")] > 0
    _same_dumps(dumps["staggered"][0], dumps["together"][0])
    _same_dumps(dumps["staggered"][0], dumps["one_stream"][0])
    # the bench line's launch statistics keep their meaning: one booked network launch per phase of the whole pool
    # (the cut evaluation's two sub-launches count as one), network time within the step
    roof = {mode: line["roofline"] for mode, (_, line) in dumps.items()}
    print({mode: (r["launches"], r["avg_launch_ms"], r["net_share_of_step"]) for mode, r in roof.items()})
    assert roof["staggered"]["launches"] == roof["together"]["launches"] == roof["one_stream"]["launches"] > 0
    for mode, r in roof.items():
        assert 0.0 < r["net_share_of_step"] <= 1.0, (mode, r["net_share_of_step"])


def test_staggered_headline_plays_the_same_games(tmp_path):
    """Default sizes (4096 games, 11x11, 400 simulations, 6x64 tower)."""
    _same_games(tmp_path)


def test_staggered_small_pool_plays_the_same_games(tmp_path):
    """The smallest pool the pipelined loop takes (1024 games)."""
    _same_games(tmp_path, "--games", "1024")


# ---- engine-level cases, each mode in a child process of its own --------------------------------------------------
CHILD = r'''
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from azalea_amd import engine as eng
from azalea_amd.network import HexNetwork

case, out = sys.argv[2], sys.argv[3]
G = 1024


def engine(n, sims, blocks, chans=64):
    torch.manual_seed(0)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    E = eng.Engine(board_size=n, n_games=G, simulations=sims, search_batch_size=10, exploration_coef=0.5,
                   exploration_depth=4, evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans, seed=1234)
    E.set_weights({k: v.detach().numpy() for k, v in net.state_dict().items()})
    return E


res = {}
if case == "late":
    # 3x3 games one stone short of a win: at most five empty cells, one of them a winning move at least, so a game's
    # first ten selections end in at most five distinct leaves -- at most half of the 10 rows per game, which is `split`
    n = 3
    perms = np.stack([np.random.RandomState(100 + g).permutation(n * n) + 1 for g in range(G)]).astype(np.int32)
    won = eng.hex_replay(n, perms, np.full(G, n * n, np.int32))[0] != 0
    assert won.any(1).all()
    first_win = won.argmax(1)
    assert first_win.min() >= 4
    E = engine(n, 20, 1)
    E.reset(moves=[perms[g, :first_win[g]].tolist() for g in range(G)])
    stats = [E.play_steps(1)]
    res["stagger_first"] = E.debug_stagger()
    stats += [E.play_steps(1) for _ in range(3)]
    res["stagger"] = E.debug_stagger()
    keys = ("positions", "games", "game_errors", "plies", "selects", "evals", "sum_depth", "sum_k_interior", "sum_k_leaf")
    arrays = {"stats": np.array([[st[k] for k in keys] for st in stats], np.int64)}
    res["net_launches"] = [st["net_launches"] for st in stats]
    res["net_within_wall"] = all(st["net_seconds"] <= st["seconds"] * 1.0001 + 1e-6 for st in stats)
elif case == "generic":
    # 16 channels: the VALU fallback tower, whose kernels stride over the rows of their own sub-launch only
    E = engine(5, 40, 1, chans=16)
    stats = [E.play_steps(1) for _ in range(3)]
    res["stagger"] = E.debug_stagger()
    arrays = {"stats": np.array([[st[k] for k in ("positions", "games", "game_errors", "plies", "selects", "evals")] for st in stats], np.int64)}
else:
    # play_until (one enqueue_plies_pipelined call per ply) through play_device: the harvested rows
    E = engine(5, 40, 1)
    rows, st = E.play_device(6000)
    rec = torch.empty((rows, E.record_bytes), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    E.rows_pack(0, rows, rec.data_ptr())
    torch.cuda.synchronize()
    arrays = {"records": rec.cpu().numpy(), "metrics": E.play_row_metrics(rows),
              "stats": np.array([st[k] for k in ("positions", "games", "game_errors", "plies", "selects", "evals")], np.int64)}
    res["stagger"] = E.debug_stagger()
    res["plies_per_slot"] = st["plies"] / G
for k, v in E.get_root().items():
    arrays["root_" + k] = v
for k, v in E.get_games().items():
    arrays["game_" + k] = v
res["kernels"] = E.kernel_info()
E.close()
np.savez(out, **arrays)
print(json.dumps(res))
'''


def _child(tmp_path, case, mode):
    out = str(tmp_path / ("%s_%s.npz" % (case, mode)))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, case, out]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(mode), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=360)
    assert r.returncode == 0, (case, mode, r.returncode, r.stderr.decode()[-2000:])
    res = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    print(case, mode, res)
    return np.load(out), res


def _same_arrays(a, b, rows_as_set=()):
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        if k in rows_as_set:    # whole rows, byte for byte, in any order
            x, y = (np.sort(np.ascontiguousarray(v).view([("b", np.void, v.strides[0])]).ravel()) for v in (x, y))
        assert x.tobytes() == y.tobytes(), k


def test_second_sub_launch_with_no_live_row(tmp_path):
    """Fewer live rows than `split`: the second sub-launch finds a count of 0 and does nothing (the counters say that it
    happened), and the games are the ones the other two schedules play."""
    got = {mode: _child(tmp_path, "late", mode) for mode in MODES}
    st = got["staggered"][1]
    assert st["stagger_first"]["starts"] == 1 and st["stagger_first"]["empty"] == 1, st
    assert st["stagger_first"]["rows_behind"] == 0 and 0 < st["stagger_first"]["rows_queued"] <= 512 * 5, st
    assert st["stagger"]["starts"] == 4, st                      # once per move
    assert STAGGERED_PLAY in st["kernels"]
    for mode in ("together", "one_stream"):
        assert got[mode][1]["stagger"]["starts"] == 0, got[mode][1]
    for mode in MODES:      # one booked network launch per phase: BEGIN + num_batches (20 // 10 + 1) per move
        assert got[mode][1]["net_launches"] == [4] * 4 and got[mode][1]["net_within_wall"], (mode, got[mode][1])
    assert got["staggered"][0]["stats"][:, 3].sum() > 0 and got["staggered"][0]["stats"][:, 5].sum() > 0
    _same_arrays(got["staggered"][0], got["together"][0])
    _same_arrays(got["staggered"][0], got["one_stream"][0])


def test_play_device_harvests_the_same_rows(tmp_path):
    """play_until is one pipelined call per ply, each with its cut evaluation.  A game's rows are contiguous in the
    harvest queue; the order in which games of the two half-pools reserve their room there is the order their streams
    get to it, so the rows are compared as a set of whole records (each byte for byte), the trees and game states in
    place."""
    got = {mode: _child(tmp_path, "device", mode) for mode in MODES}
    st = got["staggered"][1]
    assert st["stagger"]["starts"] >= 2 and st["stagger"]["empty"] < st["stagger"]["starts"], st
    assert st["stagger"]["starts"] == round(st["plies_per_slot"]), st
    assert len(got["staggered"][0]["records"]) >= 6000
    for other in ("together", "one_stream"):
        _same_arrays(got["staggered"][0], got[other][0], rows_as_set=("records", "metrics"))


def test_generic_tower_plays_the_same_games(tmp_path):
    """The cut evaluation on the generic fallback tower (k_stem_generic + k_conv_generic): same games, cut in every move."""
    got = {mode: _child(tmp_path, "generic", mode) for mode in MODES}
    st = got["staggered"][1]
    assert "k_stem_generic" in st["kernels"] and STAGGERED_PLAY in st["kernels"], st
    assert st["stagger"]["starts"] == 3 and st["stagger"]["empty"] < 3, st
    assert got["staggered"][0]["stats"][:, 5].sum() > 0
    _same_arrays(got["staggered"][0], got["together"][0])
    _same_arrays(got["staggered"][0], got["one_stream"][0])


def test_kernel_info_names_the_switch():
    """azx_kernel_info reports AZX_PIPELINE_STAGGER next to AZX_PIPELINE, for an engine the pipeline does not take too."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from azalea_amd import engine as eng\n"
            "E = eng.Engine(board_size=5, n_games=8, simulations=10, evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64)\n"
            "print(E.kernel_info()); E.close()\n" % ROOT)
    for mode, want in (("staggered", "AZX_PIPELINE=1 AZX_PIPELINE_STAGGER=1"), ("together", "AZX_PIPELINE=1 AZX_PIPELINE_STAGGER=0")):
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], cwd=ROOT, env=_env(mode),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=150)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        text = r.stdout.decode()
        assert want in text and "one stream" in text and "src=" in text, text
