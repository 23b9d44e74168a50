"""Searches and self-play calls still enqueue what they did before the host code that issues a search's launches was
folded into one phase sequence: azx_search per evaluator, from a reset and on a kept root, with host noise
and with the shortest schedule; the phase API with every n_pending it returns; azx_play_steps by persistent launches,
per-move launches and the two half-pools; azx_play with and without a queue that parks its slots -- held to
tests/golden/search_host_digests.json.  The fixture was written by tests/golden/make_search_host_digests.py on the
commit before that change; this file runs the script's cases and never writes the fixture.  The state errors of the
phase API and what a failed hand-over leaves behind are asserted here directly."""
import ctypes as C
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_search_host_digests",
                                                  os.path.join(GOLDEN, "make_search_host_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mk = _load_maker()

with open(mk.FIXTURE) as _f:
    WANT = json.load(_f)

IN_PROCESS = [name for name in mk.CASES if name not in mk.IN_CHILD_ONLY]


def test_the_fixture_holds_the_cases_of_the_script():
    assert set(WANT) == set(IN_PROCESS) | set(mk.CHILDREN) and len(WANT) == 24
    # not vacuous: no two cases have the same value but the stub's search and the inline evaluator's, which build the
    # same trees; and the three pipeline modes played the same games
    assert WANT[mk.SAME_TREES[0]] == WANT[mk.SAME_TREES[1]]
    assert len(set(WANT.values())) == len(WANT) - 1
    assert len({mk.games_of(WANT[name]) for name in mk.SAME_GAMES}) == 1


@pytest.mark.parametrize("name", IN_PROCESS)
def test_a_case_leaves_what_the_fixture_says(name):
    got = mk.run_case(name)
    print(name, got)
    assert got == WANT[name]


@pytest.mark.parametrize("name", list(mk.CHILDREN))
def test_a_case_under_its_switch_leaves_what_the_fixture_says(name):
    """AZX_NO_PERSISTENT, AZX_PIPELINE and AZX_PIPELINE_STAGGER are read at azx_create from the environment: these
    cases run in a child."""
    got = mk.child_case(name)
    print(name, got)
    assert got == WANT[name]


def test_the_pipeline_modes_differ_in_their_launches_only():
    games = {name: mk.games_of(WANT[name]) for name in mk.SAME_GAMES}
    assert len(set(games.values())) == 1, games
    launches = {name: [int(x) for x in WANT[name].split("|")[1].split(";")[0].split(",")] for name in mk.SAME_GAMES}
    print(launches)
    nb, plies = 5, 3
    # one stream and the half-pools alike book nb + 2 tree launches and nb + 1 evaluations per move: a phase's two
    # half-pool launches, and the staggered phase's two sub-launches, count as one
    for name in mk.SAME_GAMES:
        assert launches[name] == [plies * (nb + 2), plies * (nb + 2), plies * (nb + 1)], name
    how = [WANT[name].split("|")[2] for name in mk.SAME_GAMES]
    assert "half an evaluation apart" in how[0] and how[1].endswith("two half-pools on two streams")
    assert how[2].endswith("one stream")


@pytest.mark.parametrize("kind", ["uniform", "net"])
def test_a_queue_that_some_games_fit_parks_the_slots_and_returns_whole_games(kind):
    """Under a 16-row queue which games get in depends on the order they finish in (make_search_host_digests.PARK_CAP),
    so no digest: play(40) must end at the all-parked check, below its 40 rows, with whole games only, twice."""
    import numpy as np
    from azalea_amd import engine as eng
    E = mk.engine(eng, kind)
    try:
        E.debug_set_queue_cap(16)
        for _ in range(2):
            rows, st = E.play(40)
            n = st["positions"]
            assert 0 <= n <= 16 and len(rows["game_uid"]) == n and st["game_errors"] == 0
            for uid in np.unique(rows["game_uid"]):
                mine = rows["game_uid"] == uid
                assert mine.sum() >= 2 * mk.N - 1                        # a whole game: no shorter one exists
                assert (np.diff(rows["nlegal"][mine]) == -1).all()       # ... its plies in order, none missing
    finally:
        E.close()


def test_the_phase_api_refuses_a_step_too_many_and_fpu_in_flight():
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    E = mk.engine(eng, "net")
    try:
        E.reset()
        E.search_begin()
        for step in range(E.num_batches + 1):
            with pytest.raises(AzxError, match=r"azx error -4.*fpu: a phase-API search is in flight \(finish it with "
                                               r"azx_search_step first\)"):
                E.set_fpu("reduction", 0.0, 0.25, 0.0)
            n, done = E.search_step()
            assert done == (step == E.num_batches)
        with pytest.raises(AzxError, match="azx error -4.*azx_search_step without azx_search_begin"):
            E.search_step()
        E.set_fpu("reduction", 0.0, 0.25, 0.0)               # the search is over: accepted again
    finally:
        E.close()


def _returns_3_at_hand_over(E, at):
    """Registers on E the stub with its `at`-th hand-over from now replaced by a return of 3 (Engine's own trampoline
    returns 0 or 1 only); the ctypes callback is returned to be kept alive."""
    from azalea_amd import _lib
    E.set_external_evaluator(mk.stub())
    good, calls = E._ext_cb, [0]

    def fn(*args):
        calls[0] += 1
        return 3 if calls[0] == at else good(*args)
    cb = _lib.EVAL_FN(fn)
    _lib.check(E.L.azx_set_external_evaluator(E.h, C.cast(cb, C.c_void_p), None))
    return cb, good


@pytest.mark.parametrize("call", ["search", "play_steps"])
def test_a_failed_hand_over_stops_the_call_and_leaves_no_booked_launches(call):
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    E = mk.engine(eng, "external")
    try:
        E.reset()
        keep = _returns_3_at_hand_over(E, 3)
        with pytest.raises(AzxError, match=r"azx error -7.*external evaluator returned 3 on a batch of \d+ rows"):
            E.search() if call == "search" else E.play_steps(6)
        with pytest.raises(AzxError, match="azx error -4.*an external evaluation failed and left searches half done: "
                                           "azx_reset every slot first"):
            E.search() if call == "search" else E.play_steps(6)
        E.set_external_evaluator(mk.stub())
        del keep
        # after a reset of every slot the engine searches what a fresh one with the stub registered does ...
        import hashlib
        h = hashlib.sha256()
        mk.two_searches(E, h, E.search)
        assert h.hexdigest() == WANT["search_ext"]
        # ... and the next self-play call books its own launches only: the failed call's timed pairs were dropped
        E.reset()
        st = E.play_steps(2)
        nb = E.num_batches
        assert (st["mcts_launches"], st["mcts_kernel_launches"], st["net_launches"]) == (2 * (nb + 2), 2 * (nb + 2), 2 * (nb + 1))
    finally:
        E.close()
