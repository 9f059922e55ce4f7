"""CPU: the Gomoku restatement's rules on hand-written boards, lzm_az_gmk_net_prepare as a permutation, and
GomokuAZNet's shape checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import az_gomoku_ref as ref


def _board(rows):
    return np.array([int(ch) for row in rows for ch in row], np.int32)


BOARDS = [  # (rows top to bottom, (done, winner))
    (["000000"] * 6, (False, -1)),
    (["000000"] * 5 + ["011111"], (True, 1)),                                          # (0, 1) into the corner
    (["200000", "200000", "200000", "200000", "200000", "000000"], (True, 2)),        # (1, 0) from the corner
    (["100000", "010000", "001000", "000100", "000010", "000000"], (True, 1)),        # (1, 1) from the corner
    (["000002", "000020", "000200", "002000", "020000", "000000"], (True, 2)),        # (1, -1) from the corner
    (["000000", "000020", "000200", "002000", "020000", "200000"], (True, 2)),        # (1, -1) into the corner
    (["111111"] + ["000000"] * 5, (True, 1)),                                          # six in a row
    (["020000", "020000", "020000", "020000", "020000", "011111"], (True, 2)),        # 2 starts at (0, 1), 1 at (5, 1)
    (["112211", "221122", "112211", "221122", "112211", "221122"], (True, -1)),        # full, no five
    (["011110", "000000", "000000", "000000", "000000", "000000"], (False, -1)),       # four is not five
]


@pytest.mark.parametrize("rows, result", BOARDS)
def test_restatement_rules_on_known_boards(rows, result):
    env = ref.SimGomoku()
    env.reset(1, _board(rows))
    legal = [i for i, ch in enumerate("".join(rows)) if ch == "0"]
    assert env.get_done_winner() == result and env.legal_actions == legal
    if legal:  # a move fills exactly its cell with the mover's stone
        env.step(legal[-1])
        assert env.board[legal[-1]] == 2 and env.current_player == 1 and (env.board != _board(rows)).sum() == 1


def test_lines_and_draw_board():
    assert len(ref.LINES) == 32 and len(set(ref.LINES)) == 32
    draw = np.array([1 + ((c // 2 + r) % 2) for r in range(6) for c in range(6)], np.int32)
    assert np.array_equal(draw, _board(BOARDS[8][0])) and ref.done_winner(draw) == (True, -1)
    obs = ref.encode(_board(BOARDS[7][0]), 2)
    assert obs.shape == (3, 6, 6) and obs[0, 0, 1] == 0.5 and obs[1, 5, 1] == 0.5 and (obs[2] == 1.0).all()


@pytest.mark.parametrize("nres", [1, 2])
def test_net_prepare_is_a_permutation(nres):
    """arange weights: every raw weight appears exactly once in the packed buffer, everything else is zero"""
    from lightzero_amd import _lib
    L = _lib.load()
    nraw = 32 * 27 + 32 + 4 * nres * (32 * 288 + 32) + 32 * 32 + 32 + 2 * (32 * 576 + 96) + 32 + 1 + 36 * 32 + 36
    raw = np.arange(1, nraw + 1, dtype=np.float32)
    n = L.lzm_az_gmk_net_floats(nres)
    assert n > nraw and L.lzm_az_gmk_net_floats(3) == -1
    out = np.full(n, -1.0, np.float32)
    assert L.lzm_az_gmk_net_prepare(nres, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == 0
    assert np.array_equal(np.sort(out[out != 0]), raw) and (out == 0).sum() == n - nraw
    assert L.lzm_az_gmk_net_prepare(3, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == -1


def test_gomoku_net_refuses_other_models():
    from lightzero_amd.alphazero import GomokuAZNet
    from lightzero_amd.model_az import (AlphaZeroModel, connect4_alphazero_model, gomoku_alphazero_model,
                                        tictactoe_alphazero_model)
    for other in (connect4_alphazero_model(), tictactoe_alphazero_model(),
                  AlphaZeroModel((3, 6, 6), 36, 1, 16, fc_value_layers=(32,), fc_policy_layers=(32,)).eval()):
        with pytest.raises(ValueError, match="Gomoku AlphaZeroModel config"):
            GomokuAZNet(other)
    with pytest.raises(ValueError, match="eval mode"):
        GomokuAZNet(gomoku_alphazero_model().train())
