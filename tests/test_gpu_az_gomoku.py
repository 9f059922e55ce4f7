"""GPU: AlphaZero for Gomoku 6 x 6 (lzm_az_gomoku.h, lzm_az_gomoku_net.h) against the plain-Python game and search
(az_gomoku_ref.py over oracle.az_oracle) and the torch module in float64."""
import copy
import functools

import numpy as np
import pytest
import torch

import az_gomoku_ref as ref

pytestmark = pytest.mark.gpu

S = 50


# ---------------------------------------------------------------- positions
@functools.lru_cache(maxsize=None)
def _playouts():
    """every position of 200 seeded random games from the empty board, and 40 games played on to a full board,
    with the Python scan's answer for each"""
    rng, env, out, res = np.random.default_rng(0), ref.SimGomoku(), [], []
    for g in range(240):
        env.reset(0)
        while True:
            out.append(env.board.copy())
            res.append(env.get_done_winner())
            if not env.legal_actions or (g < 200 and res[-1][0]):
                break
            env.step(int(rng.choice(env.legal_actions)))
    return np.stack(out), res


def _draw_board():
    """a full board without a line of five: stones in runs of two along rows, alternating along columns"""
    return np.array([1 + ((c // 2 + r) % 2) for r in range(6) for c in range(6)], np.int32)


def _rows(rows):
    return np.array([int(ch) for row in rows for ch in row], np.int32)


def _roots():
    """B = 9: empty (either player first: 36 children, the full-width noise row); one empty cell whose fill is a
    draw; one move from a five for the mover; already won (a terminal root); six empty cells, two of them a five for
    player 1 and two a five for player 2 (the reference's walks reach depth 6 and terminal leaves of both signs);
    three playout positions with 29, 23 and 14 empty cells"""
    last = _draw_board()
    last[5] = 0  # (row 0, column 5) held a stone of player 1
    roots = [(np.zeros(36, np.int32), 0), (np.zeros(36, np.int32), 1), (last, 0),
             (_rows(["011110", "022200", "000000", "000000", "000000", "000000"]), 0),
             (_rows(["111110", "022220", "000000", "000000", "000000", "000000"]), 1),
             (_rows(["110011", "221122", "110211", "221022", "112211", "220022"]), 1)]
    po, res = _playouts()
    roots += [(po[i], int((po[i] != 0).sum()) % 2) for i in (7, 4321, 5000)]
    assert ref.done_winner(_draw_board()) == (True, -1) and ref.done_winner(roots[4][0]) == (True, 1)
    assert (roots[5][0] == 0).sum() == 6 and not any(ref.done_winner(b)[0] for b, _ in roots[:4] + roots[5:])
    return np.stack([b for b, _ in roots]), np.array([s for _, s in roots], np.int32)


# ---------------------------------------------------------------- 1. the game
def test_done_winner_equals_python_scan():
    from lightzero_amd._lib import call, ptr, stream_ptr
    hand = []
    for piece in (1, 2):  # each of the 32 lines alone: four directions, every edge and corner
        for r, c, dr, dc in ref.LINES:
            b = np.zeros((6, 6), np.int32)
            for k in range(5):
                b[r + k * dr, c + k * dc] = piece
            hand.append(b.reshape(36))
    both = _rows(["020000", "020000", "020000", "020000", "020000", "011111"])  # 2 owns the earlier start cell
    hand += [_rows(["111111"] + ["000000"] * 5), both, _draw_board()]
    po, res = _playouts()
    boards = np.concatenate([po, np.stack(hand)])
    want = np.array([[int(d), w] for d, w in res + [ref.done_winner(b) for b in hand]], np.int32)
    assert [tuple(w) for w in want[-3:]] == [(1, 1), (1, 2), (1, -1)]
    for row in ([1, 1], [1, 2], [1, -1], [0, -1]):
        assert (want == row).all(axis=1).any(), row
    d = torch.from_numpy(boards).cuda()
    out = torch.empty((len(boards), 2), dtype=torch.int32, device="cuda")
    call("lzm_az_gmk_done_winner", ptr(d), len(boards), ptr(out), stream_ptr())
    assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------- the scripted network
W = [(7 * i * i + 13 * i + 1) for i in range(36)]
_W_DEVICE = {}


def _script(cells, player, w):
    """integer hash of the position -> priors k / 1024, k in 1..61, and a value k / 1024, k in -1000..1000: exact in
    float32 on both sides. cells [n, 36] int64, player [n] int64, w: W in the caller's array type."""
    h = (cells * w).sum(-1) + player * 1000003
    pri = [1 + (h * (2 * a + 3) + a * 7919) % 61 for a in range(36)]
    return pri, (h * 31 + 17) % 2001 - 1000


def _script_torch(state):
    s = state.reshape(-1, 3, 36)
    player = (s[:, 2, 0] * 2).round().long()
    cells = (s[:, 0] > 0.25).long() * player[:, None] + (s[:, 1] > 0.25).long() * (3 - player)[:, None]
    if "w" not in _W_DEVICE:  # (first called outside a graph capture: the search's warm-up run)
        _W_DEVICE["w"] = torch.tensor(W, device=state.device)
    pri, val = _script(cells, player, _W_DEVICE["w"])
    return torch.stack(pri, 1).float() / 1024, val.float()[:, None] / 1024


def _script_ref(board, legal, player):
    pri, val = _script(np.asarray(board, np.int64)[None], np.array([player], np.int64), np.array(W, np.int64))
    return {a: np.float32(pri[a][0]) / np.float32(1024) for a in range(36)}, float(np.float32(val[0]) / np.float32(1024))


# ---------------------------------------------------------------- whole trees
def _mcts(graph=False):
    from lightzero_amd.alphazero import AlphaZeroMCTS
    return AlphaZeroMCTS(None, S, 19652, 1.25, 0.3, 0.25, device="cuda", graph=graph, game="gomoku")


def _compare(m, want, note):
    """every node of every board: node count, visit, value_sum bits, first, prior bits; the root's visit counts"""
    B = len(want)
    visit, vsum, first, nn = [t.cpu().numpy() for t in m.export_tree(B)]
    prior = m.export_priors(B).cpu().numpy()
    lv = m.last_visits(B).cpu().numpy()
    for i, (ov, _, (tv, ts, tf, n, tp)) in enumerate(want):
        assert nn[i] == n, (note, i, int(nn[i]), n)
        for name, got, exp in (("visit", visit[i, :n], tv), ("value_sum", vsum[i, :n].view(np.int32), ts.view(np.int32)),
                               ("first", first[i, :n], tf), ("prior", prior[i, :n].view(np.int32), tp.view(np.int32))):
            assert np.array_equal(got, exp), (note, i, name, int(np.nonzero(got != exp)[0][0]))
        assert np.array_equal(lv[i], ov), (note, i, lv[i], ov)


@functools.lru_cache(maxsize=None)
def _scripted_ref(sample):
    boards, starts = _roots()
    return [ref.search(b, int(s), S, _script_ref, sample) for b, s in zip(boards, starts)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sample", [False, True], ids=["nonoise", "noise"])
def test_stepwise_trees_equal_reference_scripted_network(sample, graph):
    boards, starts = _roots()
    m = _mcts(graph)
    act, probs = m.get_next_actions(boards.reshape(9, 6, 6), starts, _script_torch, 1.0, sample)
    _compare(m, _scripted_ref(sample), f"scripted sample={sample} graph={graph}")
    lv = m.last_visits(9).cpu().numpy()
    assert (lv.sum(1) > 0).all() and all(boards[i][a] == 0 for i, a in enumerate(act.cpu().numpy()))
    assert np.allclose(probs.cpu().numpy(), lv / lv.sum(1, keepdims=True), rtol=1e-15, atol=0)


# ---------------------------------------------------------------- the network
@functools.lru_cache(maxsize=None)
def _net(nres):
    from lightzero_amd.alphazero import GomokuAZNet
    from lightzero_amd.model_az import AlphaZeroModel
    torch.manual_seed(10 + nres)
    m = AlphaZeroModel((3, 6, 6), 36, nres, 32, fc_value_layers=(32,), fc_policy_layers=(32,),
                       last_linear_layer_init_zero=False)
    with torch.no_grad():  # non-trivial BatchNorm statistics so the folding is exercised
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
    m = m.eval()
    return m, GomokuAZNet(m)


@functools.lru_cache(maxsize=None)
def _states():
    po = _playouts()[0][::2][:2000]
    return torch.from_numpy(np.stack([ref.encode(b, 1 + int((b != 0).sum()) % 2) for b in po]))


def _bits(net, x):
    with torch.no_grad():
        p, v = net.compute_policy_value(x.cuda())
    return np.concatenate([p.cpu().numpy(), v.cpu().numpy()], axis=1).view(np.int32)


@pytest.mark.parametrize("nres", [1, 2])
def test_net_matches_torch_float64(nres):
    """GomokuAZNet (BatchNorm folded on the host, f32 MFMA convolutions, two K = 144 chains per element) on 2,000
    playout positions against the torch module itself on the CPU in float64 (eval mode, BatchNorm unfolded):
    |got - ref| <= 2e-5 + 2e-4 |ref|, and the maximum / 99th-percentile absolute error at most 4x / 2x those of the
    same module evaluated on the CPU in float32 (an error under 2e-5 passes this second check by itself).
    Measured on an MI355X, absolute error p99 / max (the module on the CPU in float32 beside it):
      1 residual block: policy 1.073e-08 / 2.226e-08 (1.195e-08 / 2.688e-08), value 1.057e-07 / 1.463e-07
                        (1.378e-07 / 2.187e-07)
      2 residual blocks: policy 1.243e-08 / 2.965e-08 (1.244e-08 / 3.361e-08), value 2.359e-07 / 3.244e-07
                        (2.404e-07 / 3.591e-07)"""
    m, net = _net(nres)
    x32 = _states()
    with torch.no_grad():
        gp, gv = net.compute_policy_value(x32.cuda())
        rp, rv = copy.deepcopy(m).double().compute_policy_value(x32.double())
        fp, fv = m.compute_policy_value(x32)
    for name, got, want, f32 in (("policy", gp, rp, fp), ("value", gv, rv, fv)):
        got, f32 = got.cpu().double().reshape(want.shape), f32.double().reshape(want.shape)
        err, e32 = (got - want).abs(), (f32 - want).abs()
        q = [float(torch.quantile(err.reshape(-1), z)) for z in (0.99, 1.0)]
        q32 = [float(torch.quantile(e32.reshape(-1), z)) for z in (0.99, 1.0)]
        print(f"gomoku net nres {nres} {name}: |err| p99 / max = {q[0]:.3e} / {q[1]:.3e} "
              f"(torch CPU float32: {q32[0]:.3e} / {q32[1]:.3e}); max |ref| {float(want.abs().max()):.3e}")
        assert torch.isfinite(got).all()
        assert bool((err <= 2e-5 + 2e-4 * want.abs()).all()), (name, float((err - 2e-4 * want.abs()).max()))
        assert q[1] <= max(2e-5, 4 * q32[1]) and q[0] <= max(2e-5, 2 * q32[0]), (name, q, q32)


@pytest.mark.parametrize("positions", [None, "1", "2"])
@pytest.mark.parametrize("nres", [1, 2])
def test_net_bits_do_not_depend_on_the_batch_or_instantiation(nres, positions, monkeypatch):
    """7 positions alone (n = 7) under the default rule are the yardstick; under every built instantiation
    (LZM_GMK_NET_POSITIONS) the same 7 alone, as rows of an n = 100 call on both sides of the workgroup boundaries
    of 1 and 2 positions per workgroup, and one at a time"""
    _, net = _net(nres)
    x = _states()
    seven, rows = x[1000:1007], [0, 1, 2, 3, 4, 63, 99]
    monkeypatch.delenv("LZM_GMK_NET_POSITIONS", raising=False)
    alone = _bits(net, seven)
    assert len(np.unique(alone[:, 36])) == 7 and np.isfinite(alone.view(np.float32)).all()
    if positions is not None:
        monkeypatch.setenv("LZM_GMK_NET_POSITIONS", positions)
        assert np.array_equal(_bits(net, seven), alone)
    big = x[:100].clone()
    big[rows] = seven
    assert np.array_equal(_bits(net, big)[rows], alone)
    for i in range(7):
        assert np.array_equal(_bits(net, seven[i:i + 1]), alone[i:i + 1]), i


@pytest.mark.parametrize("sample", [False, True], ids=["nonoise", "noise"])
def test_stepwise_trees_equal_reference_real_network(sample):
    """the search with GomokuAZNet in the loop against the Python search that evaluates each position alone
    through the same network (valid by test_net_bits_do_not_depend_on_the_batch_or_instantiation); then
    graph=True: the capture run and a replay give the eager visits"""
    _, net = _net(1)
    boards, starts = _roots()
    cache = {}

    def pv(board, legal, player):
        key = (np.asarray(board, np.int8).tobytes(), player)
        if key not in cache:
            with torch.no_grad():
                p, v = net.compute_policy_value(torch.from_numpy(ref.encode(board, player))[None].cuda())
            cache[key] = (dict(enumerate(p[0].tolist())), v.item())
        return cache[key]
    want = [ref.search(b, int(s), S, pv, sample) for b, s in zip(boards, starts)]
    m = _mcts()
    m.get_next_actions(boards, starts, net.compute_policy_value, 1.0, sample)
    _compare(m, want, f"real network sample={sample}")
    eager = m.last_visits(9).cpu().numpy().copy()
    g = _mcts(graph=True)
    for run in range(2):
        g.get_next_actions(boards, starts, net.compute_policy_value, 1.0, sample)
        assert np.array_equal(g.last_visits(9).cpu().numpy(), eager), run
