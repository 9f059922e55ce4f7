"""GPU: the resident search kernel's mode-5 hand-off word and tail (lzm_search_res.h: hand_pack,
expand_wave_r, backup_wave_r, the closed-form tie pick).

After the register walk every wave takes the walk's outcome (status, len, x, action) from one LDS
word; a leaf tie's candidates, its pick, the leaf and the backup's length are arithmetic on that
word's fields instead of reads of the path and the separate scalars. Every case is the fused
search's record — each simulation's x, action and search_len — and the final distributions, values
and trajectories, bit-equal to OracleTree fed the recorded network outputs
(tests/test_gpu_fused.py's fused_search / check_tree_exact, tests/test_gpu_walk_regs.py's
oracle_mismatch), over what the word's readers distinguish: a tie at the root (candidates from the
root's legal list) and below it ({0, 1}), one and two players (the tail's to_play flips), the late
pick and the pick before the dynamics (LZM_RES_LATE=0), Philox (no tie status), zero-init heads
(status 2 / 3: the resumed walk rewrites the word), one root (no look-back), and modes 1 and 4,
which keep the separate scalars.
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import test_gpu_fused as tf  # noqa: E402
from tests.test_gpu_fused import check_tree_exact, fused_search  # noqa: E402
from tests.test_gpu_walk_regs import assert_both_endings, oracle_mismatch  # noqa: E402

A, H = 2, 128
RAGGED = [[0], [1], [0, 1]]


@contextlib.contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def exact(case, **env):
    """check_tree_exact(case) under the environment env, computed once per (case, env) and shared."""
    key = (case, tuple(sorted(env.items())))
    if key not in _RUNS:
        with environ(**env):
            _RUNS[key] = check_tree_exact(case)
    return _RUNS[key]


def assert_same_search(a, b):
    for f in ("x", "action", "search_len"):
        assert np.array_equal(a["rec"][f], b["rec"][f]), f
    for f in ("dist", "values", "traj"):
        assert np.array_equal(a[f], b[f]), f


def ragged_roots(monkeypatch, legal):
    from lightzero_amd.mcts_ctree import MuZeroMCTSCtree
    roots = MuZeroMCTSCtree.roots
    monkeypatch.setattr(MuZeroMCTSCtree, "roots", classmethod(lambda cls, n, _l: roots(n, legal)))


class _AlternatingPlayers:
    """fused_search's generator with its to_play draw replaced by 1, 2, 1, 2, ..."""

    def __init__(self, rng):
        self._rng = rng

    def __getattr__(self, name):
        return getattr(self._rng, name)

    def integers(self, lo, hi, size):
        assert (lo, hi) == (1, 3)
        return np.array([1 + (q & 1) for q in range(size)])


class _Random:
    def __getattr__(self, name):
        return getattr(np.random, name)

    @staticmethod
    def default_rng(seed):
        return _AlternatingPlayers(np.random.default_rng(seed))


class _Numpy:
    """numpy as tests.test_gpu_fused sees it, with the alternating to_play draw"""
    random = _Random()

    def __getattr__(self, name):
        return getattr(np, name)


@pytest.mark.parametrize("S", [1, 2])
def test_root_level_ties_through_rleg(S, monkeypatch):
    B = 3
    ragged_roots(monkeypatch, RAGGED)
    r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A)
    assert r["diag"][0] == 0 and r["diag"][3] == 0
    assert oracle_mismatch(r, B, S, legal=RAGGED) is None
    # simulation 0 ends at a child of the root (a tie at level 0 where the root has two legal actions)
    assert np.array_equal(r["rec"]["x"][0], np.zeros(B, np.int32))
    assert np.array_equal(r["rec"]["search_len"][0], np.ones(B, np.int32))
    assert r["rec"]["action"][0][0] == 0 and r["rec"]["action"][0][1] == 1 and r["rec"]["action"][0][2] in (0, 1)
    d = r["dist"]
    assert (d[0] >= 0).sum() == 1 and (d[1] >= 0).sum() == 1 and (d[2] >= 0).sum() == 2


def test_ragged_legal_sets_two_players(monkeypatch):
    B, S = 6, 25
    legal = RAGGED * 2
    ragged_roots(monkeypatch, legal)
    monkeypatch.setattr(tf, "np", _Numpy())
    r = fused_search(B, S, A, H, False, 2, False, seed=B + S + A)
    assert r["to_play"].tolist() == [1, 2, 1, 2, 1, 2]
    assert r["diag"][0] == 0 and r["diag"][3] == 0
    assert oracle_mismatch(r, B, S, legal=legal) is None
    d = r["dist"]
    for i, l in enumerate(legal):
        assert (d[i] >= 0).sum() == len(l)


@pytest.mark.parametrize("players", [1, 2])
def test_late_pick_against_pick_before_the_dynamics(players):
    case = (8, 25, A, H, False, players, False)
    late = exact(case)  # (each equals the oracle: check_tree_exact)
    early = exact(case, LZM_RES_LATE="0")
    assert_same_search(late, early)
    assert_both_endings(late["rec"])
    assert_both_endings(early["rec"])


def test_modes_1_4_5_agree():
    case = (8, 25, A, H, False, 2, False)
    out = {m: exact(case, LZM_RES_SELECT=m) for m in ("1", "4", "5")}
    assert_same_search(out["1"], out["4"])
    assert_same_search(out["4"], out["5"])
    assert_same_search(out["1"], out["5"])
    assert_same_search(out["5"], exact(case))  # (the default is mode 5)


def test_philox_two_players():
    exact((8, 25, A, H, False, 2, True))


def test_zero_heads_resume_rewrites_the_word():
    r = exact((8, 25, A, H, True, 1, False))
    assert r["diag"][2] > 0, "no tie between visited children was resolved through depth speculation"


def test_one_root():
    exact((1, 10, A, H, False, 1, False))
