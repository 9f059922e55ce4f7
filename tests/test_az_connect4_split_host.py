"""CPU: lzm_az_c4_net_split_prepare's fragments give back the 3x3 weights, and the precision keyword."""
import ctypes

import numpy as np
import pytest

from lightzero_amd import _lib

FRAG3 = 4 * 18 * 2 * 64 * 4  # floats per layer: [wave][chunk][term][lane][8 fp16]


@pytest.mark.parametrize("nres", [1, 2])
def test_split_fragments_recover_f32_weights(nres):
    """every 64 -> 64 weight comes back as (h + l) 2^-e_c within 2^-22 of its row's largest |w|, at the place the
    16x16x32 B operand reads it (out 16 wave + lane % 16, in 32 j + 8 (lane / 16) + e, chunk 2 tap + j); rows of
    layer 0 span 2^-30 .. 2^20 and one row is all zero; the scales and bounds follow the fragments"""
    L = _lib.load()
    nl = 4 * nres
    nraw = 64 * 27 + 64 + nl * (64 * 576 + 64) + 32 * 64 + 32 + 2 * (32 * 672 + 32 * 3) + 32 + 1 + 7 * 32 + 7
    raw = (np.random.default_rng(nres).standard_normal(nraw) * 0.05).astype(np.float32)
    first = raw[64 * 27 + 64:][:64 * 576].reshape(64, 576)
    first *= np.exp2(np.linspace(-30, 20, 64)).astype(np.float32)[:, None] / 0.05
    first[5] = 0
    n = L.lzm_az_c4_net_split_floats(nres)
    assert n > nl * FRAG3 and L.lzm_az_c4_net_split_floats(3) == -1
    out = np.zeros(n, np.float32)
    arg = ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert L.lzm_az_c4_net_split_prepare(nres, *arg) == 0 and L.lzm_az_c4_net_split_prepare(3, *arg) == -1
    conv = 4 * 9 * 64 + 64  # the fragments follow conv0's and its bias
    inv = out[conv + nl * FRAG3 + nl * 64:][:nl * 64].reshape(nl, 64).astype(np.float64)
    bd = out[conv + nl * FRAG3 + 2 * nl * 64:][:nl * 4].reshape(nl, 4)
    w_, s_, l_, e_ = np.meshgrid(np.arange(4), np.arange(18), np.arange(64), np.arange(8), indexing="ij")
    cout, cin, tap = 16 * w_ + (l_ & 15), 32 * (s_ & 1) + 8 * (l_ >> 4) + e_, s_ >> 1
    for l in range(nl):
        at = 64 * 27 + 64 + l * (64 * 576 + 64)
        W, b = raw[at:at + 64 * 576].astype(np.float64).reshape(64, 64, 9), raw[at + 64 * 576:at + 64 * 577]
        terms = out[conv + l * FRAG3:][:FRAG3].view(np.float16).astype(np.float64).reshape(4, 18, 2, 64, 8)
        rec = terms.sum(axis=2) * inv[l][cout]
        top = np.abs(W).max(axis=(1, 2))
        assert np.all(np.abs(rec - W[cout, cin, tap]) <= top[cout] * 2.0 ** -22), l
        assert np.all(np.abs(terms) < 2.0 ** 15) and np.all(np.log2(inv[l]) % 1 == 0)
        assert bd[l, 0] >= np.abs(W).sum(axis=(1, 2)).max() and np.abs(b).max() <= bd[l, 1] <= np.abs(b).max() * 1.00001


def test_precision_keyword_rejects_unknown_values():
    from lightzero_amd.alphazero import Connect4AZNet
    with pytest.raises(ValueError, match="precision"):
        Connect4AZNet(None, precision="fp16")
