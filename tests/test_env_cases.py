"""CPU: every constructed case of tests/env_cases.py shows the property it is named for, through the restatements
alone (oracle/breakout_synth.py, oracle/pong_synth.py), for each value of the serve draw; the converters to the 16
device words round-trip; and the two scripted lockstep runs of tests/test_gpu_env_edges.py reach what they are
there for (a 21-point finish in Pong, upper-row bricks and ball losses in Breakout). No GPU is needed.
"""
import numpy as np
import pytest

from oracle import breakout_synth, pong_synth
from tests import env_cases as ec

_IDS = {g: [c.name for c in ec.CASES[g]] for g in ec.CASES}


def test_case_names_are_unique():
    for g, names in _IDS.items():
        assert len(set(names)) == len(names), g


@pytest.mark.parametrize("case", ec.CASES["breakout"], ids=_IDS["breakout"])
def test_breakout_case(case):
    assert case.prop, case.name
    for d in ec.draws("breakout"):
        ec.check_case("breakout", case, d)


@pytest.mark.parametrize("case", ec.CASES["pong"], ids=_IDS["pong"])
def test_pong_case(case):
    assert case.prop, case.name
    for d in ec.draws("pong"):
        ec.check_case("pong", case, d)


@pytest.mark.parametrize("game", ["breakout", "pong"])
def test_serving_cases_depend_on_the_draw_and_no_other(game):
    """a case draws the serve exactly when its step's result differs between the draws"""
    for c in ec.CASES[game]:
        outs = {repr(ec.synth(game).step(c.state, c.action, d)) for d in ec.draws(game)}
        assert len(outs) == (len(ec.draws(game)) if ec.serves(game, c.state, c.action) else 1), c.name


def test_words_round_trip_and_brick_words_are_signed():
    for g in ec.CASES:
        for c in ec.CASES[g]:
            w = ec.words(g, c.state, c.score)
            assert len(w) == 16 and all(-2 ** 31 <= x < 2 ** 31 for x in w)
            assert ec.state_of(g, w) == (c.state, c.score), c.name
            assert np.array_equal(np.array(w, dtype=np.int32), np.array(w, dtype=np.int64))
    full = ec.breakout_words(breakout_synth.new_state(10))
    assert full[6:9] == [-1, -1, (1 << 26) - 1] and full[9] == 1 and full[0] == 10
    by_name = {c.name: c for c in ec.CASES["breakout"]}
    # (the rows above the brick stand, the rows below are empty: index 0 leaves 14 bits of row 0, 32 12 bits of row 2)
    want = {0: (6, 0x7ffe), 31: (6, 0x7fffffff), 32: (7, 0x1ffe), 63: (7, 0x7fffffff), 64: (8, (1 << 11) - 2),
            89: (8, (1 << 25) - 1)}
    for b, (word, value) in want.items():
        c = by_name[f"brick_index_{b}"]
        s1, _, _ = breakout_synth.step(c.state, c.action, 1)
        w1 = ec.breakout_words(s1)
        assert w1[word] == value, (b, w1[6:9])
        w0 = ec.breakout_words(c.state)
        assert [w1[k] for k in (6, 7, 8) if k != word] == [w0[k] for k in (6, 7, 8) if k != word]
        assert word == 6 or w1[6] == -1  # (bit 31 of a full word 0: the signed word stays -1)
    pw = ec.pong_words(pong_synth.new_state(9, 40))
    assert pw[0] == 9 and pw[6] == 40 and sum(map(abs, pw)) == 49


def test_case_table_covers_the_issue_list():
    """the quantities the issue's list names each occur: every brick row and point value, both sub-steps of every
    wall, the four bounce classes of each paddle, both points, the score finishes, done by loss and by truncation"""
    bk_out = [(c, breakout_synth.step(c.state, c.action, 1)) for c in ec.CASES["breakout"]]
    assert {p for _, (_, p, _) in bk_out} >= {0.0, 1.0, 4.0, 7.0, 14.0, 11.0, 8.0, 5.0, 2.0}
    assert sum(t for _, (_, _, t) in bk_out) >= 3
    refills = [c.name for c, (s1, p, _) in bk_out if p > 0 and s1["bricks"] == ec.FULL and c.state["bricks"] != ec.FULL
               and bin(c.state["bricks"]).count("1") == 1]
    assert len(refills) >= 3, refills  # the last brick in each of the three words
    pg_out = [(c, pong_synth.step(c.state, c.action, 0)) for c in ec.CASES["pong"]]
    assert {p for _, (_, p, _) in pg_out} == {0.0, 1.0, -1.0}
    assert {(s1["me"], s1["them"]) for _, (s1, _, t) in pg_out if t} >= {(21, 3), (5, 21), (21, 20), (20, 21)}
    for g, outs in (("breakout", bk_out), ("pong", pg_out)):
        dn = [ec.done(c, t) for c, (_, _, t) in outs]
        assert any(d and not t for d, (_, (_, _, t)) in zip(dn, outs)) and not all(dn)
        assert {c.ep_count for c, _ in outs} >= {0, 1} and {c.steps for c, _ in outs} >= {0, ec.MAX_STEPS - 1}


def test_lockstep_scripts_reach_what_they_are_for():
    from tests.env_cases import BreakoutTracker, pong_actions, run_restated
    n, steps = 8, 1400
    acts = pong_actions(n, steps)
    ends = run_restated("pong", n, steps, lambda t, states: acts[t], seed=5, max_steps=10 ** 6)["score_ends"]
    assert ends >= 1, "no Pong episode of the lockstep run ends by score"
    out = run_restated("breakout", n, 300, BreakoutTracker(n, seed=7), seed=5, max_steps=10 ** 6)
    assert out["terminated"] >= n and out["points"] >= 20 * n, out
