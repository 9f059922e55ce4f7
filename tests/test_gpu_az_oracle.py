"""GPU: both AlphaZero search paths against the CPU restatement (oracle/az_oracle.py) with a REAL-VALUED network.

The restatement is fed exactly what the kernels compute: a table of the fused network's outputs for every
state the searches can meet, built in one lzm_az_net_eval launch (helpers.AzTablePolicy; the premise, that a
state's outputs do not depend on where it sits in a batch, is test_net_eval_bits_do_not_depend_on_the_batch).
With identical inputs any difference in a tree is an arithmetic-order or indexing difference in the search
(the double pUCT pb_c * prior + value, the float32 value_sum accumulation, the root noise mix, near-ties
between children), so every comparison is np.array_equal on integers and float bit patterns, over every node
of every board. With a random network sibling scores never come within an ulp of each other, so the last
rounding of the score would stay unpinned: a near-tie network (_setup, kind "tie") covers it. Also here: the
sampled action restated on the host from the device's Philox block, the
launch plan of the fused search (lzm_az_fused_plan), and the fused network against the torch module in
float64."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import AzTablePolicy, az_encode_states, az_reachable_states
from oracle import az_oracle
from oracle.tictactoe import done_winner, random_boards
from test_gpu_alphazero import _mcts, _net

pytestmark = pytest.mark.gpu

EMPTY = np.zeros(9, np.int32)
# roots random_boards never makes: player 2 to move on the empty board, and boards whose player to move has the
# "wrong" parity for the stone count (reachable from no game that starts with player 1, some from no game at all)
EXTRA_ROOTS = [(EMPTY, 1),
               (np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.int32), 0),   # 2 - 0 stones, player 1 to move
               (np.array([1, 2, 0, 0, 2, 0, 0, 0, 0], np.int32), 1),   # 1 - 2 stones, player 2 to move
               (np.array([0, 1, 0, 2, 0, 0, 1, 0, 0], np.int32), 0),   # 2 - 1 stones, player 1 to move
               (np.array([2, 0, 0, 0, 0, 0, 0, 0, 0], np.int32), 0)]   # 0 - 1 stones, player 1 to move
NET_SEED = {1: 2, 2: 4}


@functools.lru_cache(maxsize=None)
def _setup(nres, kind="rand"):
    """(torch module, FusedAZNet, table policy over every state reachable from the empty board with either
    player first and from EXTRA_ROOTS): built once per network, shared by every test.
    kind "tie": the same random network with the policy head's last layer zeroed (every prior the same float32
    1/9) and the value head's last layer scaled by 1e-14, so that sibling scores differ by a few hundred ulps
    of the double score and which child wins depends on each rounding step of pb_c * prior + value_sum / visit:
    with the plain random network near-ties that tight do not occur (swapping the oracle's score for a fused
    multiply-add, a float32 one or a double mean changed none of 512 trees of 100 simulations)."""
    from lightzero_amd.alphazero import FusedAZNet
    m = _net(NET_SEED[nres], nres)
    if kind == "tie":
        with torch.no_grad():
            m.fc_policy_head[-1].weight.zero_()
            m.fc_policy_head[-1].bias.zero_()
            m.fc_value_head[-1].weight.mul_(1e-14)
            m.fc_value_head[-1].bias.mul_(1e-14)
    net = FusedAZNet(m)
    table = AzTablePolicy(net, [(EMPTY, 0)] + EXTRA_ROOTS)
    return m, net, table


@functools.lru_cache(maxsize=None)
def _noise():
    return az_oracle.noise_table(0.3)


def _roots37():
    boards, starts = random_boards(32, 9, max_moves=6)
    boards = np.concatenate([boards, np.stack([b for b, _ in EXTRA_ROOTS])])
    starts = np.concatenate([starts, np.array([s for _, s in EXTRA_ROOTS], np.int32)])
    assert len(boards) == 37 and not any(done_winner(b)[0] for b in boards)
    return boards, starts


@functools.lru_cache(maxsize=None)
def _roots(name):
    return {"b37": _roots37, "deep24": lambda: random_boards(24, 108, max_moves=8),
            "bench512": lambda: random_boards(512, 13)}[name]()


@functools.lru_cache(maxsize=None)
def _oracle(nres, name, sims, sample, kind="rand"):
    """[(root visit counts [9], (visit, value_sum, first, nnodes, prior))] per board: az_oracle.search with the
    table policy, the reference's noise table for alpha 0.3 and weight 0.25; computed once per case"""
    table = _setup(nres, kind)[2]
    boards, starts = _roots(name)
    return [az_oracle.search(b, int(s), sims, table.pv(b, s), sample, alpha=0.3, frac=0.25, table=_noise(),
                             return_tree="priors") for b, s in zip(boards, starts)]


def _seq_probs(visits, temperature):
    """visit_count_to_action_distribution: v / T summed in action order, then divided (double)"""
    x = visits.astype(np.float64) / temperature
    seq = np.zeros(len(x))
    for k in range(9):
        seq = seq + x[:, k]
    return x / seq[:, None]


def _compare(m, probs, ref, note=""):
    """every node of every board: nnodes, visit, value_sum bits, first, prior bits (the root's noise mix
    (float)(prior (1 - w) + noise w) and the network's float32 priors as stored); last_visits; action_probs (T = 1)"""
    B = len(ref)
    visit, vsum, first, nn = [t.cpu().numpy() for t in m.export_tree(B)]
    prior = m.export_priors(B).cpu().numpy()
    lv = m.last_visits(B).cpu().numpy()
    for i, (ov, (tv, ts, tf, n, tp)) in enumerate(ref):
        assert nn[i] == n, (note, i, int(nn[i]), n)
        for name, got, want in (("visit", visit[i, :n], tv), ("value_sum", vsum[i, :n].view(np.int32), ts.view(np.int32)),
                                ("first", first[i, :n], tf), ("prior", prior[i, :n].view(np.int32), tp.view(np.int32))):
            if not np.array_equal(got, want):
                k = int(np.nonzero(got != want)[0][0])
                raise AssertionError(f"{note} board {i}: {name} differs first at node {k} of {n}: "
                                     f"{got[k]} != {want[k]} ({int((got != want).sum())} nodes differ)")
        assert np.array_equal(lv[i], ov), (note, i, lv[i], ov)
    assert np.array_equal(probs.cpu().numpy(), _seq_probs(lv, 1.0)), note


def _fused(nres, name, sims, sample, note="", kind="rand"):
    _, net, _ = _setup(nres, kind)
    boards, starts = _roots(name)
    m = _mcts(sims)
    with torch.no_grad():
        _, probs = m.search_fused(boards, starts, net, 1.0, sample, export_tree=True)
    _compare(m, probs, _oracle(nres, name, sims, sample, kind), note)


# ---------------------------------------------------------------- a. every dispatch, ragged B
@pytest.mark.parametrize("rows", [0, 1, 2, 4, 8], ids=lambda r: f"R{r}")
@pytest.mark.parametrize("sample", [False, True], ids=["nonoise", "noise"])
def test_fused_search_whole_trees_equal_oracle(rows, sample, monkeypatch):
    """the one-launch search at B = 37 (ragged against every boards-per-workgroup value, five roots no game from
    player 1's first move reaches) against the restatement fed the same network outputs: whole trees bit for bit"""
    if rows:
        monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", str(rows))
    _fused(1, "b37", 30 if rows == 8 else 60, sample, f"R{rows}")  # R = 8 trees of 60 simulations do not fit in LDS


@pytest.mark.parametrize("rows", [0, 4], ids=lambda r: f"R{r}")
@pytest.mark.parametrize("sample", [False, True], ids=["nonoise", "noise"])
def test_fused_search_whole_trees_equal_oracle_two_res_blocks(rows, sample, monkeypatch):
    if rows:
        monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", str(rows))
    _fused(2, "b37", 60, sample, f"nres 2 R{rows}")


# ---------------------------------------------------------------- b. deep boards
def test_fused_search_deep_boards_equal_oracle():
    """boards up to 8 moves deep, 150 simulations, noise: most simulations end on terminal nodes (win, loss, draw
    from the leaf's side) and the trees saturate: the terminal value's sign and the repeated terminal leaf next
    to real-valued siblings"""
    _fused(1, "deep24", 150, True, "deep")


# ---------------------------------------------------------------- near-ties: every rounding step of the score
@pytest.mark.parametrize("path", ["fused-R0", "fused-R2", "stepwise"])
@pytest.mark.parametrize("sample", [False, True], ids=["nonoise", "noise"])
def test_near_tie_network_whole_trees_equal_oracle(path, sample, monkeypatch):
    """the "tie" network (_setup): equal priors and values of ~1e-14, so siblings' double scores lie a few hundred
    ulps apart and each rounding of pb_c * prior + value_sum / visit (no fused multiply-add, the float32 mean,
    the order of the products) decides the child: the cached decisions of one board per workgroup, the
    per-level decisions of two, and the per-simulation path's kernel, whole trees bit for bit"""
    _, net, table = _setup(1, "tie")
    assert len(np.unique(table.probs.view(np.int32))) == 1 and table.probs[0, 0] == np.float32(1.0) / np.float32(9.0)
    assert 0 < np.abs(table.value).max() < 1e-12 and len(np.unique(table.value)) > 1000
    if path == "stepwise":
        boards, starts = _roots("b37")
        m = _mcts(60)
        with torch.no_grad():
            _, probs = m.get_next_actions(boards, starts, net.compute_policy_value, 1.0, sample)
        _compare(m, probs, _oracle(1, "b37", 60, sample, "tie"), f"tie {path}")
    else:
        if path == "fused-R2":
            monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", "2")
        _fused(1, "b37", 60, sample, f"tie {path}", kind="tie")


# ---------------------------------------------------------------- c. the benched shape
@pytest.mark.parametrize("dispatch", ["auto", "other"])
def test_fused_search_batch_512_whole_trees_equal_oracle(dispatch, monkeypatch):
    """512 boards x 100 simulations with noise (a grid of several hundred workgroups, more than one per CU):
    all 512 trees bit for bit, with the boards per workgroup the library picks and with the other of {1, 2}"""
    _, net, _ = _setup(1)
    plan = _mcts(100).fused_plan(512, net)
    if dispatch == "other":
        monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", str(2 if plan["rows"] == 1 else 1))
        forced = _mcts(100).fused_plan(512, net)
        assert forced["rows"] != plan["rows"], (plan, forced)
        plan = forced
    _fused(1, "bench512", 100, True, f"{dispatch} plan {plan}")


# ---------------------------------------------------------------- d. the per-simulation path, same network
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stepwise_search_whole_trees_equal_oracle(graph):
    """get_next_actions with FusedAZNet.compute_policy_value in the loop (one lzm_az_net_eval of 37 states per
    simulation), eager and as a captured graph (capture run, then a replay): root, root children and every other
    node against the restatement"""
    _, net, _ = _setup(1)
    boards, starts = _roots("b37")
    ref = _oracle(1, "b37", 60, True)
    m = _mcts(60, graph)
    for run in range(2 if graph else 1):
        with torch.no_grad():
            _, probs = m.get_next_actions(boards, starts, net.compute_policy_value, 1.0, True)
        _compare(m, probs, ref, f"stepwise graph={graph} run {run}")


# ---------------------------------------------------------------- e. the sampled action
def _philox(ck):
    from lightzero_amd._lib import call, ptr, stream_ptr
    d = torch.from_numpy(np.ascontiguousarray(ck, np.uint32).view(np.int32)).cuda()
    out = torch.empty((len(ck), 4), dtype=torch.int32, device="cuda")
    call("lzm_debug_philox", ptr(d), ptr(out), len(ck), stream_ptr())
    return out.cpu().numpy().view(np.uint32)


def _expected_draws(probs, seed, counter):
    """az_finalize's draw (lzm_az.h): Philox counter (board, counter low, counter high, 0x415a), key (seed,
    0x414c5048); u = (53 bits of words 0, 1 + 0.5) / 2^53; the first action with a positive probability whose
    running sum (double, action order) exceeds u, else the last positive one"""
    B = len(probs)
    ck = np.zeros((B, 6), np.uint32)
    ck[:, 0] = np.arange(B)
    ck[:, 1], ck[:, 2], ck[:, 3] = counter & 0xffffffff, counter >> 32, 0x415a
    ck[:, 4], ck[:, 5] = seed, 0x414c5048
    r = _philox(ck).astype(np.uint64)
    u = (((r[:, 0] >> np.uint64(5)) << np.uint64(26) | (r[:, 1] >> np.uint64(6))).astype(np.float64) + 0.5) * 2.0 ** -53
    out = np.zeros(B, np.int32)
    for i in range(B):
        cum, best = 0.0, -1
        for k in range(9):
            cum = cum + float(probs[i, k])
            if best < 0 and probs[i, k] > 0.0 and u[i] < cum:
                best = k
        if best < 0:
            best = max(k for k in range(9) if probs[i, k] > 0.0)
        out[i] = best
    return out, u


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("path", ["fused", "stepwise"])
def test_sampled_action_equals_host_restatement(path, temperature):
    """the drawn action of every board, for two searches in a row: the second one's draws come from the
    advanced search counter"""
    _, net, _ = _setup(1)
    boards, starts = random_boards(64, 7)
    seed = 12345
    from lightzero_amd.alphazero import AlphaZeroMCTS
    m = AlphaZeroMCTS(9, 40, 19652, 1.25, 0.3, 0.25, device="cuda", seed=seed)
    draws = []
    for k in range(2):
        counter = int(m._count.item())
        assert counter == k
        with torch.no_grad():
            if path == "fused":
                act, probs = m.search_fused(boards, starts, net, temperature, True)
            else:
                act, probs = m.get_next_actions(boards, starts, net.compute_policy_value, temperature, True)
        act, probs = act.cpu().numpy(), probs.cpu().numpy()
        lv = m.last_visits(64).cpu().numpy()
        assert (lv.sum(axis=1) == 40).all()
        assert np.array_equal(probs, _seq_probs(lv, temperature))
        want, u = _expected_draws(probs, seed, counter)
        assert np.array_equal(act, want), (k, np.nonzero(act != want)[0], act, want)
        stale, u_stale = _expected_draws(probs, seed, counter + 1 - 2 * k)  # the other search's counter
        assert not np.array_equal(u, u_stale)
        draws.append((act, stale))
    # the searches are deterministic (same trees), so only the counter separates the two sets of draws: over 64
    # boards they differ, and each equals what the other search's counter would have drawn from its own tree
    assert not np.array_equal(draws[0][0], draws[1][0])
    assert np.array_equal(draws[0][0], draws[1][1]) and np.array_equal(draws[1][0], draws[0][1])


# ---------------------------------------------------------------- f. the table's premise
@pytest.mark.parametrize("nres", [1, 2])
def test_net_eval_bits_do_not_depend_on_the_batch(nres):
    """lzm_az_net_eval on the game's 4,520 non-terminal states: in order, in a fixed random permutation, as a
    prefix of odd length, and alone (n = 1): every state's 9 probabilities and value have the same bits"""
    _, net, table = _setup(nres)
    states = az_reachable_states([(EMPTY, 0)])
    assert len(states) == 4520
    x = torch.from_numpy(az_encode_states(states)).cuda()

    def run(t):
        with torch.no_grad():
            p, v = net.compute_policy_value(t)
        return np.concatenate([p.cpu().numpy(), v.cpu().numpy().reshape(-1, 1)], axis=1).view(np.int32)
    full = run(x)
    assert full.shape == (4520, 10)
    perm = np.random.default_rng(5).permutation(4520)
    assert np.array_equal(run(x[torch.from_numpy(perm).cuda()]), full[perm])
    assert np.array_equal(run(x[:4519]), full[:4519])
    for i in (0, 2261, 4519):
        assert np.array_equal(run(x[i:i + 1]), full[i:i + 1]), i
    # and the shared table (a larger batch, another order) holds the same bits for these states
    idx = np.array([table.index[(sum(c * 3 ** k for k, c in enumerate(b)), p)] for b, p in states])
    got = np.concatenate([table.probs[idx], table.value[idx, None]], axis=1).view(np.int32)
    assert np.array_equal(got, full)
    assert np.isfinite(full.view(np.float32)).all() and len(np.unique(full[:, 9])) > 1000  # real-valued outputs


# ---------------------------------------------------------------- g. the fused network against float64
@pytest.mark.parametrize("nres", [1, 2])
def test_fused_net_matches_torch_float64(nres):
    """the fused network (BatchNorm folded on the host, f32 MFMA convolutions) on the 4,520 states against the
    torch module itself on the CPU in float64 (eval mode, BatchNorm unfolded): |got - ref| <= 2e-5 + 2e-4 |ref|,
    and the maximum / 99th-percentile absolute error at most 4x / 2x those of the same module evaluated on the
    CPU in float32 (an error within the bound's absolute term 2e-5 passes this second check by itself).
    Measured on an MI355X, absolute error p99 / max (the module on the CPU in float32 beside it):
      1 residual block: policy 2.163e-08 / 3.949e-08 (2.790e-08 / 4.792e-08), value 1.235e-07 / 1.864e-07
                        (1.500e-07 / 2.353e-07)
      2 residual blocks: policy 2.924e-08 / 6.099e-08 (3.298e-08 / 6.539e-08), value 1.649e-07 / 3.093e-07
                        (1.815e-07 / 2.758e-07)"""
    m, net, _ = _setup(nres)
    states = az_reachable_states([(EMPTY, 0)])
    x32 = torch.from_numpy(az_encode_states(states))
    with torch.no_grad():
        gp, gv = net.compute_policy_value(x32.cuda())
        m64 = copy.deepcopy(m).cpu().double().eval()
        rp, rv = m64.compute_policy_value(x32.double())
        m32 = copy.deepcopy(m).cpu().float().eval()
        fp, fv = m32.compute_policy_value(x32)
    for name, got, ref, f32 in (("policy", gp, rp, fp), ("value", gv, rv, fv)):
        got, ref, f32 = got.cpu().double().reshape(ref.shape), ref.double(), f32.double().reshape(ref.shape)
        err, e32 = (got - ref).abs(), (f32 - ref).abs()
        q = [float(torch.quantile(err.reshape(-1), z)) for z in (0.99, 1.0)]
        q32 = [float(torch.quantile(e32.reshape(-1), z)) for z in (0.99, 1.0)]
        print(f"fused net nres {nres} {name}: |err| p99 / max = {q[0]:.3e} / {q[1]:.3e} "
              f"(torch CPU float32: {q32[0]:.3e} / {q32[1]:.3e}); max |ref| {float(ref.abs().max()):.3e}")
        assert torch.isfinite(got).all()
        assert bool((err <= 2e-5 + 2e-4 * ref.abs()).all()), (name, float((err - 2e-4 * ref.abs()).max()))
        assert q[1] <= max(2e-5, 4 * q32[1]) and q[0] <= max(2e-5, 2 * q32[0]), (name, q, q32)


# ---------------------------------------------------------------- the launch plan
@pytest.mark.parametrize("rows", [1, 2, 4, 8])
def test_fused_plan_follows_the_environment_override(rows, monkeypatch):
    _, net, _ = _setup(1)
    monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", str(rows))
    plan = _mcts(30).fused_plan(37, net)
    assert plan["rows"] == rows and plan["workgroups"] == (37 + rows - 1) // rows
    assert 0 < plan["lds_bytes"] <= 160 * 1024 and plan["per_cu"] >= 1, plan


@pytest.mark.parametrize("nres", [1, 2])
def test_fused_plan_at_the_benched_shape_fits_the_gpu(nres, monkeypatch):
    """B = 512, S = 100: the row count the library picks has a grid the GPU holds at once, by the occupancy the
    runtime reports (per_cu -1 would mean the query failed and 1 was assumed)"""
    monkeypatch.delenv("LZM_AZ_BOARDS_PER_WG", raising=False)
    _, net, _ = _setup(nres)
    plan = _mcts(100).fused_plan(512, net)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert plan["rows"] in (1, 2, 4, 8) and plan["workgroups"] == (512 + plan["rows"] - 1) // plan["rows"], plan
    assert plan["per_cu"] >= 1 and plan["workgroups"] <= plan["per_cu"] * cus, (plan, cus)
    assert 0 < plan["lds_bytes"] <= 160 * 1024 and plan["per_cu"] * plan["lds_bytes"] <= 160 * 1024, plan


def test_fused_plan_reports_trees_that_do_not_fit_and_the_search_refuses(monkeypatch):
    """8 boards per workgroup x 60 simulations: the plan reports more than 160 KiB of LDS and no workgroup per
    CU; search_fused raises the capacity error on the host, before any launch"""
    from lightzero_amd._lib import LzmError
    _, net, _ = _setup(1)
    monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", "8")
    m = _mcts(60)
    plan = m.fused_plan(37, net)
    assert plan["rows"] == 8 and plan["workgroups"] == 5 and plan["lds_bytes"] > 160 * 1024 and plan["per_cu"] == 0, plan
    boards, starts = _roots("b37")
    with pytest.raises(LzmError, match="LDS per workgroup"):
        m.search_fused(boards, starts, net, 1.0, True)
    out = (ctypes.c_int32 * 4)()
    monkeypatch.setenv("LZM_AZ_BOARDS_PER_WG", "3")
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        from lightzero_amd._lib import call
        call("lzm_az_fused_plan", 37, 60, 1, out)
