"""CPU: lzm_az_gmkn_net_prepare as a permutation, the board-size checks of the lzm_az_gmkn_* entry points and
GomokuAZNet's shape checks at 9 x 9 / 15 x 15 (no GPU needed)."""
import ctypes

import numpy as np
import pytest


@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("n", [9, 15])
def test_net_prepare_is_a_permutation(n, nres):
    """arange weights: every raw weight appears exactly once in the packed buffer, everything else is zero"""
    from lightzero_amd import _lib
    L = _lib.load()
    c = n * n
    nraw = 32 * 27 + 32 + 4 * nres * (32 * 288 + 32) + 32 * 32 + 32 + 2 * (32 * 16 * c + 96) + 32 + 1 + c * 32 + c
    raw = np.arange(1, nraw + 1, dtype=np.float32)
    total = L.lzm_az_gmkn_net_floats(n, nres)
    assert total > nraw
    out = np.full(total, -1.0, np.float32)
    assert L.lzm_az_gmkn_net_prepare(n, nres, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == 0
    assert np.array_equal(np.sort(out[out != 0]), raw) and (out == 0).sum() == total - nraw


@pytest.mark.parametrize("n, nres", [(6, 1), (7, 1), (16, 1), (9, 3), (15, 3)])
def test_entry_points_refuse_other_sizes_on_the_host(n, nres):
    from lightzero_amd import _lib
    L = _lib.load()
    buf = np.zeros(16, np.float32)
    nbytes = ctypes.c_int64(-7)
    assert L.lzm_az_gmkn_net_floats(n, nres) == -1
    assert L.lzm_az_gmkn_net_prepare(n, nres, ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data)) == -1
    assert b"9 and 15" in L.lzm_last_error()
    if nres == 1:
        assert L.lzm_az_gmkn_workspace_bytes(n, 4, 50, ctypes.byref(nbytes)) == -1 and nbytes.value == -7
        assert b"9 and 15" in L.lzm_last_error()
    else:
        assert L.lzm_az_gmkn_workspace_bytes(n, 4, 50, ctypes.byref(nbytes)) == 0 and nbytes.value > 0


def test_gomoku_net_refuses_other_models_and_model_has_board_size():
    from lightzero_amd.alphazero import GomokuAZNet
    from lightzero_amd.model_az import AlphaZeroModel, gomoku_alphazero_model
    for other in (AlphaZeroModel((3, 12, 12), 144, 1, 32, fc_value_layers=(32,), fc_policy_layers=(32,)).eval(),
                  AlphaZeroModel((3, 15, 15), 225, 1, 64, fc_value_layers=(32,), fc_policy_layers=(32,)).eval()):
        with pytest.raises(ValueError, match="Gomoku AlphaZeroModel config"):
            GomokuAZNet(other)
    m = gomoku_alphazero_model(board_size=15)
    assert m.fc_policy_head[-1].out_features == 225 and not m.training
    assert gomoku_alphazero_model().fc_policy_head[-1].out_features == 36
