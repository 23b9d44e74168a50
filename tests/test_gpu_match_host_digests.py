"""Matches and tournaments still play the games they did before their host code was folded into one ply loop
(DESIGN 7.19): small matches -- plain, collecting under a fixed first mover, from a book without and with refills, with an
external engine under either ply schedule, with a small network -- and tournaments of three engines and of one pair,
held to tests/golden/match_host_digests.json: a SHA-256 per case over the records, the stats' integers and the harvested
rows.  The fixture was written by tests/golden/make_match_host_digests.py on the commit before that change; this file
runs the script's cases and never writes the fixture."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_match_host_digests",
                                                  os.path.join(GOLDEN, "make_match_host_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mk = _load_maker()

with open(mk.FIXTURE) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_the_cases_of_the_script():
    assert set(WANT) == set(mk.CASES) | {mk.PLAIN_ORDER} and len(mk.CASES) == 8
    # not vacuous: the cases that play different games have different digests, those that play the same games one
    same = {mk.PLAIN_ORDER, mk.SAME_GAMES[0]}
    assert len({WANT[name] for name in WANT if name not in same}) == len(WANT) - len(same)
    assert WANT[mk.PLAIN_ORDER] == WANT[mk.PLAIN_ORDER_OF]
    assert WANT[mk.SAME_GAMES[0]] == WANT[mk.SAME_GAMES[1]]


@pytest.mark.parametrize("name", list(mk.CASES))
def test_a_case_plays_the_games_of_the_fixture(name):
    got = mk.run_case(name)
    print(name, got)
    assert got == WANT[name]


def test_the_one_pair_tournament_plays_the_games_of_its_match():
    assert mk.run_case(mk.SAME_GAMES[0]) == mk.run_case(mk.SAME_GAMES[1])


def test_the_plain_ply_order_plays_the_games_of_the_interleaved_one():
    """AZX_MATCH_INTERLEAVE is read at azx_match_create from the environment: the plain order runs in a child."""
    got = mk.plain_order_digest()
    print(got)
    assert got == WANT[mk.PLAIN_ORDER]
    assert got == mk.run_case(mk.PLAIN_ORDER_OF)
