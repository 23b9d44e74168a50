"""Device-resident replay ring (azx_replay_*, azalea_amd/device_replay.py) against the reference's
recorded ReplayBuffer states and shuffled DataLoader epoch (golden G7), and against the host
mirror on rows the engine itself played."""
import numpy as np
import pytest
import torch

from replay_golden import KEYS, assert_batch_equal, load_g7, source_frame

pytestmark = pytest.mark.gpu


def make_engine(n=11, games=8, sims=20):
    from azalea_amd import engine as eng
    return eng.Engine(board_size=n, n_games=games, simulations=sims, search_batch_size=10,
                      evaluator=eng.EVAL_UNIFORM, noise_scale=0.25, temperature=1.0,
                      exploration_depth=15, seed=99)


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def flat(batch):
    out = dict(batch)
    out["board"] = np.asarray(batch["board"])
    return out


def test_put_append_wrap_and_overflow_match_reference():
    from azalea_amd.device_replay import DeviceReplayBuffer
    z = load_g7()
    frame = source_frame(z)
    cap = int(z["cap"])
    E = make_engine()
    buf = DeviceReplayBuffer(E, cap, frame[:cap])
    assert len(buf) == cap and buf.write_idx == 0 and buf.fresh_counter == 0
    for j, (a, b) in enumerate(z["cuts"]):
        buf.put(frame[int(a):int(b)])
        assert buf.write_idx == int(z["put%d_write_idx" % j])
        assert buf.fresh_counter == float(z["put%d_fresh" % j])
        assert_batch_equal(host(buf.sample(np.arange(cap))), z, "put%d_" % j)
    E.close()


def test_shuffled_epoch_matches_reference_dataloader():
    from azalea_amd.device_replay import DeviceReplayBuffer
    z = load_g7()
    frame = source_frame(z)
    cap = int(z["cap"])
    E = make_engine()
    buf = DeviceReplayBuffer(E, cap, frame[:cap])
    for a, b in z["cuts"]:
        buf.put(frame[int(a):int(b)])
    torch.manual_seed(1234)
    n = 0
    for j, batch in enumerate(buf.loader(5)):
        assert list(batch.keys()) == list(KEYS)
        assert all(v.is_cuda for v in batch.values())
        assert_batch_equal(host(batch), z, "epoch_b%d_" % j, exact_width=int(z["epoch_widths"][j]))
        n += 1
    assert n == len(z["epoch_widths"])
    E.close()


def test_state_dict_round_trip():
    from azalea_amd.device_replay import DeviceReplayBuffer
    z = load_g7()
    frame = source_frame(z)
    E = make_engine()
    buf = DeviceReplayBuffer(E, 12, frame[:12])
    buf.put(frame[12:19])
    sd = buf.state_dict()
    before = host(buf.sample(np.arange(12)))
    E2 = make_engine()
    buf2 = DeviceReplayBuffer(E2, 12)
    buf2.load_state_dict(sd)
    assert buf2.write_idx == buf.write_idx and buf2.fresh_counter == buf.fresh_counter and len(buf2) == 12
    after = host(buf2.sample(np.arange(12)))
    for k in KEYS:
        assert np.array_equal(before[k], after[k]), k
    E.close(); E2.close()


def test_consume_refills_on_device_with_whole_valid_games():
    """ReplayBuffer.consume accounting (replay_buffer.py:121-132) with the refill played and stored
    on the GPU; the stored rows are legal Hex positions with normalised visit distributions and
    collate exactly like the same rows taken through the host path."""
    from azalea_amd.device_replay import DeviceReplayBuffer
    from azalea_amd.parallel_player import rows_to_frame
    from azalea_amd.prep import torch_batch_replays
    E = make_engine(n=7, games=16, sims=20)
    cap = 4096
    buf = DeviceReplayBuffer(E, cap)
    assert len(buf) == 0
    m = buf.consume(100)                       # nothing fresh: refill = 100 - (-100) = 200 rows at least
    rows = len(buf)
    assert rows >= 200 and buf.fresh_counter == rows - 100 and m["games"] >= 1
    assert buf.consume(50) == {} or buf.fresh_counter >= 50
    got = host(buf.sample(np.arange(rows)))
    board = got["board"].reshape(rows, 49)
    k = (got["legal_moves"] > 0).sum(1)
    assert np.array_equal(k, (board == 0).sum(1))
    for i in range(rows):
        assert np.array_equal(got["legal_moves"][i, :k[i]], np.flatnonzero(board[i] == 0) + 1)
        assert abs(got["moves_prob"][i, :k[i]].sum() - 1.0) < 1e-5 and np.all(got["moves_prob"][i, k[i]:] == 0)
    assert set(np.unique(got["reward"])) <= {-1.0, 1.0} and np.all(got["result"] == 0)
    # stones alternate: X (colour 0) moves on even plies
    assert np.array_equal(got["color"], ((board > 0).sum(1) & 1))
    # the same rows through the host mirror collate to the same tensors
    frame = rows_to_frame(dict(board=board.reshape(rows, 7, 7), color=got["color"], nlegal=k,
                               moves_prob=np.pad(got["moves_prob"], ((0, 0), (0, 49 - got["moves_prob"].shape[1]))),
                               reward=got["reward"]))
    idx = np.array([3, 0, rows - 1, rows // 2, 7])
    want = {kk: v.numpy() for kk, v in torch_batch_replays([frame[int(i)] for i in idx]).items()}
    have = host(buf.sample(idx))
    for kk in KEYS:
        assert have[kk].dtype == want[kk].dtype and np.array_equal(have[kk], want[kk]), kk
    E.close()


def test_mover_view_collate_is_the_search_side_flip():
    """azx_replay_set_mover_view (config["train_mover_view"]; not the reference's batch): the second player's rows come
    out as hex.py's flip_player_board_moves makes them for the search (mcts.py:178-181), the first player's rows and
    every moves_prob / reward / color untouched; the ring, its checkpoint and the default view are unaffected."""
    from azalea_amd.device_replay import DeviceReplayBuffer
    from azalea_amd.game.hex import HexGame
    from azalea_amd.policy_trainer import to_mover_view
    for n in (7, 11, 13):
        E = make_engine(n=n, games=16, sims=20)
        buf = DeviceReplayBuffer(E, 4096)
        buf.consume(150)
        rows = len(buf)
        idx = np.random.RandomState(n).permutation(rows)[:97]
        plain = host(buf.sample(idx))
        buf.mover_view = True
        assert buf.mover_view
        seen = host(buf.sample(idx))
        kept = buf.state_dict()["rows"]                     # checkpoints hold absolute colours whatever the view
        assert buf.mover_view
        buf.mover_view = False
        again = host(buf.sample(idx))
        second = plain["color"] == 1
        assert second.any() and (~second).any()
        want_b, want_m = HexGame.flip_player_board_moves(plain["board"][second], plain["legal_moves"][second])
        assert np.array_equal(seen["board"][second], want_b) and np.array_equal(seen["legal_moves"][second], want_m)
        assert np.array_equal(seen["board"][~second], plain["board"][~second])
        assert np.array_equal(seen["legal_moves"][~second], plain["legal_moves"][~second])
        for k in ("color", "moves_prob", "reward", "result"):
            assert np.array_equal(seen[k], plain[k]), k
        for k in KEYS:
            assert np.array_equal(again[k], plain[k]), k
            assert np.array_equal(np.asarray(kept[k])[idx].reshape(plain[k].shape[0], -1)[:, :plain[k].reshape(len(idx), -1).shape[1]],
                                  plain[k].reshape(len(idx), -1)) or k in ("legal_moves", "moves_prob"), k
        # the host twin used for DataLoader batches does the same
        tb = to_mover_view({k: torch.as_tensor(v).clone() for k, v in plain.items()}, HexGame)
        for k in KEYS:
            assert np.array_equal(tb[k].numpy(), seen[k]), k
        # flipped twice is the identity, and a flipped row is a position with the same stones for the mover
        back_b, back_m = HexGame.flip_player_board_moves(seen["board"][second], seen["legal_moves"][second])
        assert np.array_equal(back_b, plain["board"][second]) and np.array_equal(back_m, plain["legal_moves"][second])
        E.close()


@pytest.mark.parametrize("mode", ["overflow", "wrap"])
def test_record_put_wraps_and_overflows_like_the_row_put(mode):
    """k_records_put's wrap ((write_idx + i) % cap) and overflow (skip = n - cap) paths, which no ring larger than its
    rows reaches: the same harvested 7x7 rows enter engine A's ring as records (replay_put_records) and engine B's as
    host rows (replay_put, whose wrap and overflow golden G7 pins) -- once as a single put into a ring five rows too
    small, once as two puts of which the second wraps -- and the two rings hold the same state and collate the same
    batches at every index."""
    from azalea_amd import distributed as azd
    A, B = make_engine(n=7, games=16, sims=20), make_engine(n=7, games=16, sims=20)
    rows, _ = A.play_device(40)
    assert rows >= 40
    rec = torch.empty((rows, A.record_bytes), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    A.rows_pack(0, rows, rec.data_ptr())
    turned = rec.flip(0).contiguous()                           # the second put: the same rows, last first
    torch.cuda.synchronize()
    puts = [rec] if mode == "overflow" else [rec, turned]
    cap = rows - 5 if mode == "overflow" else rows + rows // 2
    from azalea_amd.device_replay import DeviceReplayBuffer
    bufs = [DeviceReplayBuffer(E, cap) for E in (A, B)]
    for part in puts:
        h = azd.unpack_rows(part.cpu().numpy(), 7)
        A.replay_put_records(rows, part.data_ptr())
        B.replay_put(h["board"], h["color"], h["nlegal"], h["moves_prob"], h["reward"])
        assert A.replay_state() == B.replay_state()
    want = dict(capacity=cap, size=cap, write_idx=(len(puts) * rows) % cap)
    assert A.replay_state() == want and want["write_idx"] != 0
    a, b = (host(buf.sample(np.arange(cap))) for buf in bufs)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    # and the ring is what a sequential put leaves: slot (first + i) % cap holds row i of the last cap rows put
    h = azd.unpack_rows(torch.cat(puts).cpu().numpy(), 7)
    total = len(puts) * rows
    slot = np.arange(total - cap, total) % cap
    assert np.array_equal(a["board"].reshape(cap, 49)[slot], h["board"].reshape(total, 49)[total - cap:])
    assert np.array_equal(a["reward"][slot], h["reward"][total - cap:])
    A.close(); B.close()


@pytest.mark.parametrize("n", [2, 3, 8, 12, 13])
def test_record_exchange_round_trip_on_other_board_sizes(n):
    """The multi-GPU exchange unit (AZX_RECORD_BYTES, k_rows_pack -> k_records_put) on the smallest and largest boards:
    rows harvested on the device, packed into records, unpacked by the host twin (distributed.unpack_rows) and -- put
    into a ring from the records -- collated: the same boards, move lists, distributions, rewards, colours."""
    from azalea_amd import distributed as azd
    from azalea_amd.device_replay import DeviceReplayBuffer
    E = make_engine(n=n, games=16, sims=20)
    rows, st = E.play_device(40)
    assert rows >= 40
    rec = torch.empty((rows, E.record_bytes), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    E.rows_pack(0, rows, rec.data_ptr())
    assert E.record_bytes == azd.record_bytes(n * n) and E.record_bytes % 16 == 0
    host_rows = azd.unpack_rows(rec.cpu().numpy(), n)
    buf = DeviceReplayBuffer(E, rows + 3)
    E.replay_put_records(rows, rec.data_ptr())
    assert len(buf) == rows
    got = host(buf.sample(np.arange(rows)))
    cells = n * n
    board = got["board"].reshape(rows, cells)
    assert np.array_equal(board, host_rows["board"].reshape(rows, cells))
    assert np.array_equal(got["color"], host_rows["color"]) and np.array_equal(got["reward"], host_rows["reward"])
    k = host_rows["nlegal"]
    assert np.array_equal(k, (board == 0).sum(1)) and np.array_equal(got["color"], (board > 0).sum(1) & 1)
    K = got["moves_prob"].shape[1]
    assert K == k.max() and np.array_equal(got["moves_prob"], host_rows["moves_prob"][:, :K])
    for i in range(rows):
        assert np.array_equal(got["legal_moves"][i, :k[i]], np.flatnonzero(board[i] == 0) + 1)
        assert abs(got["moves_prob"][i].sum() - 1.0) < 1e-5
    assert len(np.unique(host_rows["game_uid"])) >= 1 and set(np.unique(got["reward"])) <= {-1.0, 1.0}
    # the host twin packs what it unpacked
    assert np.array_equal(azd.pack_rows(host_rows, cells), rec.cpu().numpy())
    E.close()
