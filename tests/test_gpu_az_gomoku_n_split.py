"""GPU: the Gomoku 9 x 9 / 15 x 15 network on split-fp16 MFMA (lzm_az_gomoku_n_net_split.h,
GomokuAZNet(precision="split")) against the torch module in float64, and inside the search against the plain-Python
restatement."""
import copy
import functools

import numpy as np
import pytest
import torch

import az_gomoku_ref as ref
from test_gpu_az_gomoku_n import S, _bits, _compare, _mcts, _net, _roots, _states

pytestmark = pytest.mark.gpu

SIZES = [9, 15]


@pytest.fixture(autouse=True)
def _board_size(request, monkeypatch):
    """the restatement's functions read ref.N when called: the size-n game, encoder and search"""
    monkeypatch.setattr(ref, "N", request.node.callspec.params["n"])


@functools.lru_cache(maxsize=None)
def _split(n, nres):
    from lightzero_amd.alphazero import GomokuAZNet
    return GomokuAZNet(_net(n, nres)[0], precision="split")


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
        print(f"gomoku split net {note} {name}: |err| p99 / max = {q[0]:.3e} / {q[1]:.3e} "
              f"(torch CPU float32: {q32[0]:.3e} / {q32[1]:.3e}); max |ref| {float(want.abs().max()):.3e}")
        assert torch.isfinite(got).all()
        assert bool((err <= 2e-5 + 2e-4 * want.abs()).all()), (name, float((err - 2e-4 * want.abs()).max()))
        assert q[1] <= max(2e-5, 4 * q32[1]) and q[0] <= max(2e-5, 2 * q32[0]), (name, q, q32)
        e1 = (one.cpu().double().reshape(want[:1].shape) - want[:1]).abs()
        assert bool((e1 <= 2e-5 + 2e-4 * want[:1].abs()).all()), (name, "n = 1")
    assert net.range_errors() == 0


@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_split_net_matches_torch_float64(n, nres):
    """300 playout positions. Measured on an MI355X, absolute error p99 / max (the module on the CPU in float32
    beside it):
      9 x 9,   1 block:  policy 5.624e-09 / 1.241e-08 (4.788e-09 / 1.091e-08), value 2.688e-07 / 3.535e-07
                         (2.462e-07 / 3.094e-07)
      9 x 9,   2 blocks: policy 5.921e-09 / 1.763e-08 (5.496e-09 / 1.339e-08), value 3.943e-07 / 4.695e-07
                         (2.891e-07 / 3.623e-07)
      15 x 15, 1 block:  policy 2.928e-09 / 7.606e-09 (2.087e-09 / 6.609e-09), value 3.765e-07 / 5.845e-07
                         (2.995e-07 / 3.584e-07)
      15 x 15, 2 blocks: policy 4.303e-09 / 1.244e-08 (2.473e-09 / 7.553e-09), value 3.856e-07 / 5.233e-07
                         (2.866e-07 / 3.468e-07)"""
    _check(_net(n, nres)[0], _split(n, nres), _states(n), f"{n}x{n} nres {nres}")


@pytest.mark.parametrize("k", [-20, 0, 20])
@pytest.mark.parametrize("n", SIZES)
def test_split_net_is_magnitude_independent(n, k):
    """conv0's folded weight and bias times 2^k (BatchNorm's affine pair scales both): unscaled fp16 terms overflow
    at +20 and lose their low terms at -20"""
    from lightzero_amd.alphazero import GomokuAZNet
    m = copy.deepcopy(_net(n, 1)[0])
    with torch.no_grad():
        m.norm.weight.mul_(2.0 ** k)
        m.norm.bias.mul_(2.0 ** k)
    _check(m, GomokuAZNet(m, precision="split"), _states(n)[:101], f"{n}x{n} 2^{k}")


@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_split_net_bits_do_not_depend_on_the_batch(n, nres):
    """7 positions, the input planes of every second one times 2^-24 (its neighbours' scales differ by 2^24), alone
    (n = 7) are the yardstick; the same 7 as rows of a 100-position call and one at a time"""
    net = _split(n, nres)
    x = _states(n)
    seven, rows = x[200:207].clone(), [0, 1, 2, 3, 4, 63, 99]
    seven[1::2] *= 2.0 ** -24
    alone = _bits(net, seven)
    # (the scaled positions' inputs are all but zero: their values may coincide, so only the unscaled ones must differ)
    assert len(np.unique(alone[::2, n * n])) == 4 and np.isfinite(alone.view(np.float32)).all()
    big = x[:100].clone()
    big[rows] = seven
    assert np.array_equal(_bits(net, big)[rows], alone)
    for i in range(7):
        assert np.array_equal(_bits(net, seven[i:i + 1]), alone[i:i + 1]), i
    assert net.range_errors() == 0


@pytest.mark.parametrize("graph,sample", [(False, False), (True, False), (False, True)],
                         ids=["eager", "graph", "eager-noise"])
@pytest.mark.parametrize("n", SIZES)
def test_stepwise_trees_equal_reference_split_network(n, graph, sample):
    """the 9-root x 50-simulation search with the split network in the loop against the Python search that
    evaluates each position alone through the same network: whole trees bit for bit (graph: capture and replay)"""
    net = _split(n, 1)
    boards, starts = _roots(n)
    cache = {}

    def pv(board, legal, player):
        key = (np.asarray(board, np.int8).tobytes(), player)
        if key not in cache:
            with torch.no_grad():
                p, v = net.compute_policy_value(torch.from_numpy(ref.encode(board, player))[None].cuda())
            cache[key] = (dict(enumerate(p[0].tolist())), v.item())
        return cache[key]
    want = [ref.search(b, int(s), S, pv, sample) for b, s in zip(boards, starts)]
    m = _mcts(n, graph)
    for run in range(2 if graph else 1):
        m.get_next_actions(boards, starts, net.compute_policy_value, 1.0, sample)
        _compare(m, want, f"split network n={n} graph={graph} sample={sample} run={run}")
    assert net.range_errors() == 0


@pytest.mark.parametrize("bad", [1e38, float("nan")], ids=["1e38", "nan"])
@pytest.mark.parametrize("n", SIZES)
def test_split_net_counts_range_errors(n, bad):
    from lightzero_amd.alphazero import GomokuAZNet
    m = copy.deepcopy(_net(n, 1)[0])
    with torch.no_grad():
        m.conv.weight.fill_(bad)
    net = GomokuAZNet(m, precision="split")
    net.compute_policy_value(_states(n)[:5].cuda())
    assert net.range_errors() > 0
