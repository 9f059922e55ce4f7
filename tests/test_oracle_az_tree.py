"""CPU: az_oracle.search(return_tree=True), the restatement's whole tree flattened in the device's layout
(lightzero_amd/csrc/lzm_az.h: node 0 the root, every expansion appends its children contiguously in action
order), and the breadth-first state walk behind the table-driven policy of tests/test_gpu_az_oracle.py."""
import numpy as np
import pytest

from helpers import az_encode_states, az_reachable_states
from oracle import az_oracle
from oracle.tictactoe import SimTicTacToe, done_winner, random_boards, scripted_policy_value


def _blocks(first, n):
    """{node: (first child, one past the last)}: the blocks lie in the order their nodes were expanded, so a
    block ends where the next one starts"""
    starts = sorted(int(f) for f in first if f >= 0)
    ends = dict(zip(starts, starts[1:] + [n]))
    return {i: (int(f), ends[int(f)]) for i, f in enumerate(first) if f >= 0}


@pytest.mark.parametrize("max_moves,sims,sample", [(4, 60, False), (4, 60, True), (8, 150, True)])
def test_return_tree_is_consistent_with_return_values(max_moves, sims, sample):
    boards, starts = random_boards(12, 40 + max_moves, max_moves=max_moves)
    table = az_oracle.noise_table(0.3)
    for b, s in zip(boards, starts):
        ref = az_oracle.search(b, int(s), sims, scripted_policy_value, sample, table=table, return_values=True)
        visits, vsums, (rv, rvs), tree = az_oracle.search(b, int(s), sims, scripted_policy_value, sample, table=table,
                                                          return_values=True, return_tree=True)
        only = az_oracle.search(b, int(s), sims, scripted_policy_value, sample, table=table, return_tree=True)
        assert np.array_equal(visits, ref[0]) and np.array_equal(vsums.view(np.int32), ref[1].view(np.int32))
        assert (rv, rvs) == ref[2] and np.array_equal(only[0], visits)
        visit, vsum, first, n = tree
        assert all(np.array_equal(x, y) for x, y in zip(only[1][:3], tree[:3])) and only[1][3] == n
        assert visit.dtype == np.int32 and vsum.dtype == np.float32 and first.dtype == np.int32
        assert len(visit) == len(vsum) == len(first) == n
        # the root and its children: the existing return_values outputs
        legal = np.nonzero(b == 0)[0]
        assert first[0] == 1 and visit[0] == rv == sims
        assert vsum[0].view(np.int32) == np.float32(rvs).view(np.int32)
        assert np.array_equal(visit[1:1 + len(legal)], visits[legal])
        assert np.array_equal(vsum[1:1 + len(legal)].view(np.int32), vsums[legal].view(np.int32))
        # every node but the root is in exactly one block; an inner node was visited once when it was expanded
        # and once per visit of a child (the root is expanded before the first simulation)
        blocks = _blocks(first, n)
        covered = np.zeros(n, np.int32)
        for i, (f, e) in blocks.items():
            covered[f:e] += 1
            assert 1 <= e - f <= 9
            assert visit[i] == (0 if i == 0 else 1) + visit[f:e].sum(), (i, visit[i], visit[f:e])
        assert covered[0] == 0 and (covered[1:] == 1).all()
        assert (visit[first < 0] >= 0).all() and n == 1 + sum(e - f for f, e in blocks.values())
        # return_tree="priors": the same tree with the nodes' float32 priors; a fresh root has prior 1, and without
        # noise its children carry the policy's priors in action order
        withp = az_oracle.search(b, int(s), sims, scripted_policy_value, sample, table=table, return_tree="priors")[1]
        assert all(np.array_equal(x, y) for x, y in zip(withp[:3], tree[:3])) and withp[3] == n
        prior = withp[4]
        assert prior.dtype == np.float32 and len(prior) == n and prior[0] == 1.0 and (prior[1:] > 0).all()
        if not sample:
            want = scripted_policy_value(b, legal)[0]
            assert np.array_equal(prior[1:1 + len(legal)], np.array([want[a] for a in legal], np.float32))


def test_reachable_states_cover_the_game():
    """from the empty board, player 1 first: the game's 4,520 non-terminal positions, each once, none terminal,
    stone counts consistent with the player to move; other roots add the states only they reach; the encoding
    is current_state()'s scaled form"""
    empty = np.zeros(9, np.int32)
    st = az_reachable_states([(empty, 0)])
    assert len(st) == 4520 and len(set(st)) == 4520 and st[0] == ((0,) * 9, 1)
    for b, p in st:
        assert not done_winner(b)[0]
        assert b.count(1) - b.count(2) == (0 if p == 1 else 1)
    odd = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.int32)  # two stones of player 1, player 1 to move
    more = az_reachable_states([(empty, 0), (empty, 1), (odd, 0)])
    assert more[:2] == [((0,) * 9, 1), ((0,) * 9, 2)] and (tuple(odd.tolist()), 1) in more
    assert set(st) < set(more) and len(set(more)) == len(more)
    assert sum(1 for b, p in more if b.count(1) - b.count(2) == (0 if p == 2 else -1)) == 4520  # the mirrored game
    x = az_encode_states(more[:50] + [(tuple(odd.tolist()), 1)])
    env = SimTicTacToe(scale=True)
    env.reset(0, odd)
    assert x.shape == (51, 3, 3, 3) and x.dtype == np.float32 and np.array_equal(x[-1], env.current_state()[1])
    assert np.array_equal(x[1, 2], np.full((3, 3), 1.0, np.float32))  # player 2 to move: plane 2 = 2 / 2
