"""CPU: lzm_az_gmkn_net_split_prepare's fragments give back the 3x3 weights; argument checks; the precision keyword."""
import ctypes

import numpy as np
import pytest

from lightzero_amd import _lib

FRAG3 = 9 * 2 * 2 * 64 * 4  # floats per layer: [chunk = tap][N tile][term][lane][8 fp16]


@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("n", [9, 15])
def test_split_fragments_recover_f32_weights(n, nres):
    """every 32 -> 32 weight comes back as (h + l) 2^-e_c within 2^-22 of its row's largest |w|, at the place the
    16x16x32 B operand reads it (out 16 N tile + lane % 16, in 8 (lane / 16) + e, chunk = tap); rows of layer 0 span
    2^-30 .. 2^20 and one row is all zero; the scales and bounds follow the fragments"""
    L = _lib.load()
    nl, cells = 4 * nres, n * n
    nraw = (32 * 27 + 32 + nl * (32 * 288 + 32) + 32 * 32 + 32 + 2 * (32 * 16 * cells + 32 * 3) + 32 + 1
            + cells * 32 + cells)
    raw = (np.random.default_rng(10 * n + nres).standard_normal(nraw) * 0.05).astype(np.float32)
    first = raw[32 * 27 + 32:][:32 * 288].reshape(32, 288)
    first *= np.exp2(np.linspace(-30, 20, 32)).astype(np.float32)[:, None] / 0.05
    first[5] = 0
    nf = L.lzm_az_gmkn_net_split_floats(n, nres)
    assert nf > nl * FRAG3
    out = np.zeros(nf, np.float32)
    arg = ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert L.lzm_az_gmkn_net_split_prepare(n, nres, *arg) == 0
    conv = 2 * 9 * 64 + 32  # the fragments follow conv0's and its bias
    inv = out[conv + nl * FRAG3 + nl * 32:][:nl * 32].reshape(nl, 32).astype(np.float64)
    bd = out[conv + nl * FRAG3 + 2 * nl * 32:][:nl * 4].reshape(nl, 4)
    tap, t_, l_, e_ = np.meshgrid(np.arange(9), np.arange(2), np.arange(64), np.arange(8), indexing="ij")
    cout, cin = 16 * t_ + (l_ & 15), 8 * (l_ >> 4) + e_
    for l in range(nl):
        at = 32 * 27 + 32 + l * (32 * 288 + 32)
        W, b = raw[at:at + 32 * 288].astype(np.float64).reshape(32, 32, 9), raw[at + 32 * 288:at + 32 * 289]
        terms = out[conv + l * FRAG3:][:FRAG3].view(np.float16).astype(np.float64).reshape(9, 2, 2, 64, 8)
        rec = terms.sum(axis=2) * inv[l][cout]
        top = np.abs(W).max(axis=(1, 2))
        assert np.all(np.abs(rec - W[cout, cin, tap]) <= top[cout] * 2.0 ** -22), l
        assert np.all(np.abs(terms) < 2.0 ** 15) and np.all(np.log2(inv[l]) % 1 == 0)
        assert bd[l, 0] >= np.abs(W).sum(axis=(1, 2)).max() and np.abs(b).max() <= bd[l, 1] <= np.abs(b).max() * 1.00001


@pytest.mark.parametrize("n,nres", [(6, 1), (10, 1), (9, 0), (15, 3)])
def test_bad_board_size_or_blocks_give_minus_one(n, nres):
    L = _lib.load()
    buf = np.zeros(16, np.float32)
    arg = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data)
    assert L.lzm_az_gmkn_net_split_floats(n, nres) == -1
    assert L.lzm_az_gmkn_net_split_prepare(n, nres, *arg) == -1
    assert L.lzm_az_gmkn_net_split_eval(n, nres, *arg, 1, *arg, arg[0], None) == -1


def test_precision_keyword():
    from lightzero_amd.alphazero import GomokuAZNet
    from lightzero_amd.model_az import AlphaZeroModel
    with pytest.raises(ValueError, match="precision"):
        GomokuAZNet(None, precision="fp16")
    m = AlphaZeroModel((3, 6, 6), 36, 1, 32, fc_value_layers=(32,), fc_policy_layers=(32,)).eval()
    with pytest.raises(ValueError, match="9 and 15"):
        GomokuAZNet(m, device="cpu", precision="split")
