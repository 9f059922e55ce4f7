"""CPU: the Connect4 restatement's rules on hand-written boards, lzm_az_c4_net_prepare as a permutation, and
Connect4AZNet's shape checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import az_connect4_ref as ref


def _board(rows):
    return np.array([int(ch) for row in rows for ch in row], np.int32)


BOARDS = [  # (rows top to bottom, (done, winner), legal actions)
    (["0000000"] * 6, (False, -1), [0, 1, 2, 3, 4, 5, 6]),
    (["0000000"] * 5 + ["2221111"], (True, 1), [0, 1, 2, 3, 4, 5, 6]),                                 # horizontal, corner
    (["2000000", "2000000", "2000000", "2000000", "1000000", "1011000"], (True, 2), [1, 2, 3, 4, 5, 6]),  # vertical, top
    (["0000000", "0000000", "0001000", "0012000", "0122000", "1221000"], (True, 1), [0, 1, 2, 3, 4, 5, 6]),  # diagonal /
    (["0000000", "0000000", "2000000", "1200000", "1120000", "1212000"], (True, 2), [0, 1, 2, 3, 4, 5, 6]),  # diagonal \
    (["1122112", "2211221", "1122112", "2211221", "1122112", "2211221"], (True, -1), []),                  # full, no line
]


@pytest.mark.parametrize("rows, result, legal", BOARDS)
def test_restatement_rules_on_known_boards(rows, result, legal):
    env = ref.SimConnect4()
    env.reset(0, _board(rows))
    assert env.get_done_winner() == result and env.legal_actions == legal
    if legal:  # a move lands on the column's lowest empty cell
        a = legal[-1]
        height = sum(row[a] != "0" for row in rows)
        env.step(a)
        assert env.board[(5 - height) * 7 + a] == 1 and env.current_player == 2 and (env.board != 0).sum() == \
            (_board(rows) != 0).sum() + 1


@pytest.mark.parametrize("nres", [1, 2])
def test_net_prepare_is_a_permutation(nres):
    """arange weights: every raw weight appears exactly once in the packed buffer, everything else is zero"""
    from lightzero_amd import _lib
    L = _lib.load()
    nraw = 64 * 27 + 64 + 4 * nres * (64 * 576 + 64) + 32 * 64 + 32 + 2 * (32 * 672 + 96) + 32 + 1 + 7 * 32 + 7
    raw = np.arange(1, nraw + 1, dtype=np.float32)
    n = L.lzm_az_c4_net_floats(nres)
    assert n > nraw and L.lzm_az_c4_net_floats(3) == -1
    out = np.full(n, -1.0, np.float32)
    assert L.lzm_az_c4_net_prepare(nres, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == 0
    assert np.array_equal(np.sort(out[out != 0]), raw) and (out == 0).sum() == n - nraw
    assert L.lzm_az_c4_net_prepare(3, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == -1


def test_connect4_net_refuses_other_models():
    from lightzero_amd.alphazero import Connect4AZNet
    from lightzero_amd.model_az import AlphaZeroModel, connect4_alphazero_model, tictactoe_alphazero_model
    with pytest.raises(ValueError, match="Connect4 AlphaZeroModel config"):
        Connect4AZNet(AlphaZeroModel((3, 6, 7), 7, 1, 16, fc_value_layers=(32,), fc_policy_layers=(32,)).eval())
    with pytest.raises(ValueError, match="Connect4 AlphaZeroModel config"):
        Connect4AZNet(tictactoe_alphazero_model())
    with pytest.raises(ValueError, match="eval mode"):
        Connect4AZNet(connect4_alphazero_model().train())
