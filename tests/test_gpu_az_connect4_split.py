"""GPU: the Connect4 network on split-fp16 MFMA (lzm_az_c4_net_split.h, Connect4AZNet(precision="split")) against
the torch module in float64, and inside the search against the plain-Python restatement."""
import copy
import functools

import numpy as np
import pytest
import torch

import az_connect4_ref as ref
from test_gpu_az_connect4 import S, _bits, _compare, _mcts, _net, _playouts, _roots

pytestmark = pytest.mark.gpu


def _model(nres):
    return _net(nres)[0]


def _split(m):
    from lightzero_amd.alphazero import Connect4AZNet
    return Connect4AZNet(m, precision="split")


@functools.lru_cache(maxsize=None)
def _states():
    """301 playout positions: no multiple of 2 or 4 positions per workgroup, so the last workgroup is ragged"""
    po = _playouts()[::20][:301]
    return torch.from_numpy(np.stack([ref.encode(b, 1 + int((b != 0).sum()) % 2) for b in po]))


def _check(m, net, x32, note):
    """|got - ref| <= 2e-5 + 2e-4 |ref| against the module in float64 on the CPU; p99 / max absolute error at most
    2x / 4x the module's CPU float32 error (an error under 2e-5 passes that by itself); the first position alone"""
    with torch.no_grad():
        gp, gv = net.compute_policy_value(x32.cuda())
        ap, av = net.compute_policy_value(x32[:1].cuda())
        rp, rv = copy.deepcopy(m).double().compute_policy_value(x32.double())
        fp, fv = m.compute_policy_value(x32)
    for name, got, one, want, f32 in (("policy", gp, ap, rp, fp), ("value", gv, av, rv, fv)):
        got, f32 = got.cpu().double().reshape(want.shape), f32.double().reshape(want.shape)
        err, e32 = (got - want).abs(), (f32 - want).abs()
        q = [float(torch.quantile(err.reshape(-1), z)) for z in (0.99, 1.0)]
        q32 = [float(torch.quantile(e32.reshape(-1), z)) for z in (0.99, 1.0)]
        print(f"connect4 split net {note} {name}: |err| p99 / max = {q[0]:.3e} / {q[1]:.3e} "
              f"(torch CPU float32: {q32[0]:.3e} / {q32[1]:.3e}); max |ref| {float(want.abs().max()):.3e}")
        assert torch.isfinite(got).all()
        assert bool((err <= 2e-5 + 2e-4 * want.abs()).all()), (name, float((err - 2e-4 * want.abs()).max()))
        assert q[1] <= max(2e-5, 4 * q32[1]) and q[0] <= max(2e-5, 2 * q32[0]), (name, q, q32)
        e1 = (one.cpu().double().reshape(want[:1].shape) - want[:1]).abs()
        assert bool((e1 <= 2e-5 + 2e-4 * want[:1].abs()).all()), (name, "n = 1")
    assert net.range_errors() == 0


@pytest.mark.parametrize("nres", [1, 2])
def test_split_net_matches_torch_float64(nres):
    """Measured on an MI355X, absolute error p99 / max (the module on the CPU in float32 beside it):
      1 residual block: policy 4.597e-08 / 9.471e-08 (4.378e-08 / 5.692e-08), value 3.027e-07 / 3.848e-07
                        (2.227e-07 / 2.296e-07)
      2 residual blocks: policy 6.274e-08 / 1.021e-07 (5.822e-08 / 1.207e-07), value 4.828e-07 / 5.566e-07
                        (4.869e-07 / 5.104e-07)"""
    m = _model(nres)
    _check(m, _split(m), _states(), f"nres {nres}")


@pytest.mark.parametrize("k", [-20, 0, 20])
def test_split_net_is_magnitude_independent(k):
    """conv0's folded weight and bias times 2^k (BatchNorm's affine pair scales both): unscaled fp16 terms overflow
    at +20 and lose their low terms at -20"""
    m = copy.deepcopy(_model(1))
    with torch.no_grad():
        m.norm.weight.mul_(2.0 ** k)
        m.norm.bias.mul_(2.0 ** k)
    _check(m, _split(m), _states()[:101], f"2^{k}")


@pytest.mark.parametrize("nres", [1, 2])
def test_split_net_bits_do_not_depend_on_the_batch(nres):
    """100 positions with input planes alternately times 1 and 2^-24: each alone equals itself inside the batch"""
    net = _split(_model(nres))
    x = _states()[:100].clone()
    x[1::2] *= 2.0 ** -24
    batch = _bits(net, x)
    for i in range(100):
        assert np.array_equal(_bits(net, x[i:i + 1]), batch[i:i + 1]), i
    assert np.isfinite(batch.view(np.float32)).all() and net.range_errors() == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stepwise_trees_equal_reference_split_network(graph):
    """the 9-root x 50-simulation search with the split network in the loop against the Python search that
    evaluates each position alone through the same network: whole trees bit for bit (graph: capture and replay)"""
    net = _split(_model(1))
    boards, starts = _roots()
    cache = {}

    def pv(board, legal, player):
        key = (np.asarray(board, np.int8).tobytes(), player)
        if key not in cache:
            with torch.no_grad():
                p, v = net.compute_policy_value(torch.from_numpy(ref.encode(board, player))[None].cuda())
            cache[key] = ({a: p[0, a].item() for a in range(7)}, v.item())
        return cache[key]
    want = [ref.search(b, int(s), S, pv, False) for b, s in zip(boards, starts)]
    m = _mcts(graph)
    for run in range(2 if graph else 1):
        m.get_next_actions(boards, starts, net.compute_policy_value, 1.0, False)
        _compare(m, want, f"split network graph={graph} run={run}")
    assert net.range_errors() == 0


@pytest.mark.parametrize("bad", [1e38, float("nan")], ids=["1e38", "nan"])
def test_split_net_counts_range_errors(bad):
    m = copy.deepcopy(_model(1))
    with torch.no_grad():
        m.conv.weight.fill_(bad)
    net = _split(m)
    net.compute_policy_value(_states()[:5].cuda())
    assert net.range_errors() > 0
