"""The self-play options still hand the kernels the values they did before their host plumbing was folded into tables
(DESIGN 7.17): one small network-free engine under no option, each option alone, every option the library takes
together and the Gumbel root search with the options it goes with, held to tests/golden/selfplay_option_digests.json --
the stats as exact integers, the option fields of azx_kernel_info and a SHA-256 over the harvested rows, games ordered by
game_uid.  The fixture was written by tests/golden/make_selfplay_option_digests.py on the commit before that change;
this file runs the script's cases and never writes the fixture."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_selfplay_option_digests",
                                                  os.path.join(GOLDEN, "make_selfplay_option_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mk = _load_maker()

with open(mk.FIXTURE) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_the_cases_of_the_script():
    assert set(WANT["cases"]) == set(mk.CASES) and len(mk.CASES) == 10
    assert WANT["engine"] == dict(board_size=mk.N, n_games=mk.G, seed=mk.SEED, plies=mk.PLIES)
    # every option alone, all the library takes together, gumbel with the four it goes with
    assert all(mk.CASES[name] == (name,) for name in mk.ORDER)
    assert set(mk.CASES["all_but_gumbel"]) == set(mk.ORDER) - {"gumbel"}
    assert set(mk.CASES["gumbel_with"]) == {"gumbel", "playout_cap", "resign", "train_targets", "selfplay_openings"}
    # the fixture is not vacuous: every case played whole games, and every option left its mark in its own stats
    played = {name: c for name, c in WANT["cases"].items() if "refused" not in c}
    assert "none" in played and all(c["games"] >= mk.G and c["rows"] > 0 for c in played.values())
    assert len({c["digest"] for c in played.values()}) == len(played)
    for name in mk.ORDER:
        if name in played:
            assert any(sum(v) if isinstance(v, list) else v for v in played[name]["stats"][name].values()), name


@pytest.mark.parametrize("name", list(mk.CASES))
def test_a_case_gives_the_stats_the_info_fields_and_the_rows_of_the_fixture(name):
    got, want = mk.run_case(mk.CASES[name]), WANT["cases"][name]
    print(name, got)
    if "refused" in want:
        assert got == want                      # the refusal's text, character for character
        return
    assert got["info"] == want["info"]
    assert got["stats"] == want["stats"]
    assert (got["games"], got["rows"]) == (want["games"], want["rows"])
    assert got["digest"] == want["digest"]


def test_an_engine_with_every_option_cleared_plays_the_games_of_one_that_never_had_them():
    got, want = mk.run_cleared(), WANT["cleared"]
    print(got)
    assert got == want
    assert got["cleared"]["digest"] == got["fresh"]["digest"] and got["cleared"]["info"] == got["fresh"]["info"]
    assert set(got["fresh"]["info"].values()) == {"off"}


def test_search_after_a_play_under_every_option_is_the_search_of_a_fresh_engine():
    """The options are still set: the scope of the play calls left the engine's device state off."""
    got, want = mk.run_search_after_options(), WANT["search"]
    print(got)
    assert got == want
    assert got["after_all_options"] == got["fresh"]
