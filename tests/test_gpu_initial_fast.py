"""The shape-specialised initial-inference kernel (csrc/lzm_initial.h, initial_fast_kernel) against the generic one.

At the resident search kernel's widths (H 128, F 32, V 601, SimNorm 8, A <= 32, O <= 16) lzm_mlp_initial_inference
and lzm_mlp_initial_inference_prepare launch a kernel that holds its weights in registers, loaded ahead from a
second copy in [slot][thread] float4 order, and keeps ii_dense's arithmetic. It must give the generic kernel's
bits (LZM_II_FAST=0 forces that one, read at each call): without preparation across odd O (a short last R1 slice),
A = 3 (Q2: 85 slices, 32 of them with one k) and A = 32 (8 slices of 4); with preparation the same roots and the
same recorded search. Shapes one past each limit keep the generic kernel. CPU: the fast block is the permutation
the header states, and the Python shape rule is the library's.
"""
import numpy as np
import pytest
import torch

from lightzero_amd import _lib
from lightzero_amd.initial import FAST_MAX_ACTIONS, FAST_MAX_OBS, describe_initial, fast_block, fast_shape
from tests.test_gpu_initial_shapes import initial_model

FAST = dict(H=128, F=32, V=601, group=8)


def query(O, A, H=128, F=32, V=601, group=8):
    return _lib.load().lzm_mlp_initial_fast(O, H, F, V, A, group)


def cpu_model(O, A, seed=0):
    from lightzero_amd.model_mlp import MuZeroModelMLP
    torch.manual_seed(seed)
    return MuZeroModelMLP(observation_shape=O, action_space_size=A, latent_state_dim=128, fc_reward_layers=(32,),
                          fc_value_layers=(32,), fc_policy_layers=(32,), reward_support_size=601,
                          value_support_size=601, categorical_distribution=True, last_linear_layer_init_zero=False,
                          norm_type='BN', res_connection_in_dynamics=True).eval()


def test_fast_block_is_the_stated_permutation():
    """slot s of thread t: 4 consecutive k of the thread's column in ii_dense's map (include/lzmcts.h)"""
    layers, dims = describe_initial(cpu_model(5, 3))
    assert fast_shape(dims)
    blk = fast_block(layers).numpy()
    assert blk.size == 81920
    T, o = 256, 0
    for l in (1, 2, 3, 4, 6):
        W = layers[l][0].t().numpy()  # [K][N]
        K, N = W.shape
        Kc = K * N // T
        want = np.empty((Kc // 4, T, 4), np.float32)
        for t in range(T):
            n, ks = t % N, t // N
            want[:, t, :] = W[ks * Kc:(ks + 1) * Kc, n].reshape(Kc // 4, 4)
        assert np.array_equal(blk[o:o + want.size], want.reshape(-1)), l
        o += want.size
    W = layers[5][0].t().numpy()  # V2 [32][601]
    want = np.zeros((3, 8, T, 4), np.float32)
    for j in range(3):
        for t in range(T):
            if t + 256 * j < 601:
                want[j, :, t, :] = W[:, t + 256 * j].reshape(8, 4)
    assert np.array_equal(blk[o:], want.reshape(-1))


def test_selection_rule_host(monkeypatch):
    """the query: 1 at the fast shape up to both bounds, 0 one past each limit and with LZM_II_FAST=0; the Python
    rule that decides whether the block is packed is the same rule"""
    monkeypatch.delenv("LZM_II_FAST", raising=False)
    assert (FAST_MAX_OBS, FAST_MAX_ACTIONS) == (16, 32)
    cases = [dict(), dict(O=1, A=1), dict(O=16, A=32), dict(H=96), dict(F=48), dict(V=101), dict(group=4), dict(O=17),
             dict(A=33)]
    for c in cases:
        kw = dict(O=4, A=2, **FAST)
        kw.update(c)
        want = 1 if set(c) <= {"O", "A"} and kw["O"] <= 16 and kw["A"] <= 32 else 0
        assert query(**kw) == want, c
        dims = dict(obs=kw["O"], hidden=kw["H"], head_hidden=kw["F"], support=kw["V"], actions=kw["A"], group=kw["group"])
        assert fast_shape(dims) == bool(want), c
    monkeypatch.setenv("LZM_II_FAST", "0")
    assert query(4, 2) == 0
    monkeypatch.setenv("LZM_II_FAST", "1")
    assert query(4, 2) == 1


def run_initial(fi, obs):
    with torch.no_grad():
        out = fi.initial_inference(obs)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (out.latent_state, out.value, out.policy_logits)], out


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("O,A", [(4, 2), (1, 1), (5, 3), (FAST_MAX_OBS, 32)])
def test_fast_equals_generic_bitwise(O, A, B, monkeypatch):
    from lightzero_amd.initial import FusedInitialInference
    monkeypatch.delenv("LZM_II_FAST", raising=False)
    m = initial_model(O, 128, 32, 601, A, seed=O + A)
    fi = FusedInitialInference(m)
    assert fi.offsets.shape == (17,) and fi.offsets[16] > 0 and fi.offsets[16] % 4 == 0
    obs = torch.randn(B, O, generator=torch.Generator().manual_seed(B)).to("cuda:0")
    assert query(O, A) == 1
    fast, _ = run_initial(fi, obs)
    monkeypatch.setenv("LZM_II_FAST", "0")
    assert query(O, A) == 0
    generic, _ = run_initial(fi, obs)
    for name, a, b in zip(("latent", "value", "policy"), fast, generic):
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert np.isfinite(fast[1]).all() and np.abs(fast[1]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("players", [1, 2])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("A", [2, 3])
def test_fast_preparation_equals_generic(A, noise, players, monkeypatch):
    """the same legal table and counts, and the same recorded search afterwards, fast on and fast off"""
    from lightzero_amd.initial import FusedInitialInference
    from lightzero_amd.mcts_ctree import MuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    dev = torch.device("cuda", 0)
    B, S = 8, 6
    m = initial_model(4, 128, 32, 601, A, seed=A)
    fi = FusedInitialInference(m)
    rng = np.random.default_rng(A + players)
    legal = [sorted(rng.choice(A, size=1 + i % A, replace=False).tolist()) for i in range(B)]  # root 0: one action
    obs = torch.from_numpy(rng.normal(size=(B, 4)).astype(np.float32)).to(dev)
    noises = torch.from_numpy(rng.dirichlet([0.3] * A, size=B).astype(np.float32)).to(dev) if noise else None
    to_play = torch.from_numpy((np.full(B, -1) if players == 1 else rng.integers(1, 3, size=B)).astype(np.int32)).to(dev)
    rewards = torch.zeros(B, device=dev)
    seeds = torch.arange(100, 100 + S, dtype=torch.int32, device=dev)
    cfg = EasyDict(dict(num_simulations=S, discount_factor=0.997, device=dev,
                        model=dict(support_scale=300, categorical_distribution=True)))
    mcts = MuZeroMCTSCtree(cfg)
    mcts.record = True
    res = []
    for env, want in ((None, 1), ("0", 0)):
        if env is None:
            monkeypatch.delenv("LZM_II_FAST", raising=False)
        else:
            monkeypatch.setenv("LZM_II_FAST", env)
        assert query(4, A) == want
        roots = MuZeroMCTSCtree.roots(B, legal)
        with torch.no_grad():
            out = fi.initial_inference(obs, prepare=dict(roots=roots, noise_weight=0.25, noises=noises,
                                                         rewards=rewards, to_play=to_play))
        t = roots.tree
        d0 = t.distributions().cpu().numpy()
        for i, l in enumerate(legal):  # the legal table and counts: zero visits at the legal positions, -1 beyond
            assert (d0[i, :len(l)] == 0).all() and (d0[i, len(l):] == -1).all()
        mcts.search(roots, m, out.latent_state, to_play, seeds=seeds)
        assert mcts.last_path == "fused-mlp"
        res.append(dict(rec=mcts.last_record.numpy(), dist=t.distributions().cpu().numpy(),
                        values=t.values().cpu().numpy(), traj=t.trajectories(S + 2).cpu().numpy(), d0=d0,
                        out=[x.cpu().numpy() for x in (out.latent_state, out.value, out.policy_logits)]))
        t.check_errors()
        roots.clear()
    a, b = res
    assert np.array_equal(a["d0"], b["d0"])
    for x, y in zip(a["out"], b["out"]):
        assert np.array_equal(x, y)
    for f in ("x", "action", "search_len", "vtp", "decoded", "policy_logits"):
        assert np.array_equal(a["rec"][f], b["rec"][f]), f
    for f in ("dist", "values", "traj"):
        assert np.array_equal(a[f], b[f]), f
    assert (a["dist"][0] >= 0).sum() == 1 and a["dist"][0, 0] == S  # the one-action root


@pytest.mark.gpu
def test_one_past_the_bound_keeps_the_generic_kernel(monkeypatch):
    from lightzero_amd.initial import FusedInitialInference
    from tests.mlp_numerics import check_initial_network
    monkeypatch.delenv("LZM_II_FAST", raising=False)
    O, A, B = FAST_MAX_OBS + 1, 2, 37
    assert query(O, A) == 0
    m = initial_model(O, 128, 32, 601, A, seed=1)
    fi = FusedInitialInference(m)
    assert fi.offsets[16] == -1
    obs = torch.randn(B, O, generator=torch.Generator().manual_seed(B)).to("cuda:0")
    _, got = run_initial(fi, obs)
    check_initial_network(f"initial O{O} one past the fast bound B{B}", m, obs, got)


@pytest.mark.gpu
def test_fast_shape_matches_float64_and_repeats(monkeypatch):
    from lightzero_amd.initial import FusedInitialInference
    from tests.mlp_numerics import check_initial_network
    monkeypatch.delenv("LZM_II_FAST", raising=False)
    O, A, B = 4, 2, 37
    assert query(O, A) == 1
    m = initial_model(O, 128, 32, 601, A, seed=2)
    fi = FusedInitialInference(m)
    obs = torch.randn(B, O, generator=torch.Generator().manual_seed(B)).to("cuda:0")
    first, got = run_initial(fi, obs)
    check_initial_network(f"initial fast O{O} A{A} B{B}", m, obs, got)
    second, _ = run_initial(fi, obs)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
