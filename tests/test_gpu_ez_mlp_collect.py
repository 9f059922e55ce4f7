"""GPU: the CartPole EfficientZero model (cartpole_efficientzero_model, the zoo's quick-start config) on the
one-launch search through the collect step, the device collector and reanalyze.

1. DeviceSearchStep, eager and as one HIP graph: each step equals, bit for bit, the host-seeded
   EfficientZeroMCTSCtree.search on the same path (the collect step's glue as one launch before and one after
   the search kernel).
2. EfficientZeroCollectPolicy over DeviceCartPoleEnvManager through the MuZeroCollector drop-in takes the device
   path, and its segments equal the restatement's of the reference's collect loop fed the same episodes.
3. reanalyze_policy_targets takes the one-launch path; the same search, recorded, is reproduced by the oracle.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.collector_ref import EpisodeEnv, EpisodeForward, ref_collect  # noqa: E402
from oracle.oracle import OracleTree  # noqa: E402
from tests.helpers import PB_C_BASE, PB_C_INIT, VDM  # noqa: E402
from tests.test_gpu_muzero_collector import _compare, _played  # noqa: E402

DEV = torch.device("cuda", 0)


def _model(seed=0):
    from lightzero_amd.model_mlp import cartpole_efficientzero_model
    torch.manual_seed(seed)
    m = cartpole_efficientzero_model(random_heads=True)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
    return m.to(DEV).eval()


@pytest.mark.parametrize("graph", [False, True])
def test_device_search_step_matches_host_seeded_search(graph):
    from lightzero_amd.collect import DeviceSearchStep
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    B, S, seed = 8, 10, 7
    legal = [[0, 1]] * B
    model = _model()
    rng = np.random.default_rng(0)
    obs_list = [torch.from_numpy(rng.normal(size=(B, 4)).astype(np.float32)).to(DEV) for _ in range(3)]
    nz_list = [torch.from_numpy(rng.dirichlet([0.3, 0.3], size=B).astype(np.float32)).to(DEV) for _ in range(3)]
    step = DeviceSearchStep(model, B, S, legal, (4,), DEV, seed=seed, graph=graph)
    assert step.ez and step.mcts_cls is EfficientZeroMCTSCtree
    outs = []
    for k, (obs, nz) in enumerate(zip(obs_list, nz_list)):
        step.set_inputs(obs=obs, noises=nz)
        o = step.step()
        outs.append((o["distributions"].clone(), o["values"].clone()))
        assert int(step.step_counter.item()) == k + 1
        assert step.mcts.last_path == "fused-mlp"
        assert (outs[-1][0].sum(dim=1) == S).all()
    mcts = EfficientZeroMCTSCtree(EasyDict(dict(num_simulations=S, discount_factor=0.997, device=DEV,
                                                lstm_horizon_len=5,
                                                model=dict(support_scale=300, categorical_distribution=True))))
    base = (1000003 * seed) % 1000000
    to_play = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for n, (dist, vals) in enumerate(outs):
            out = (step.initial or model).initial_inference(obs_list[n])  # (the step's own initial inference)
            roots = EfficientZeroMCTSCtree.roots(B, legal)
            roots.prepare_device(0.25, nz_list[n], torch.zeros(B, device=DEV), out.policy_logits, to_play)
            seeds = torch.tensor([(base + n * S + k) % 1000000 for k in range(S)], dtype=torch.int32, device=DEV)
            mcts.search(roots, model, out.latent_state, out.reward_hidden_state, to_play, seeds=seeds)
            assert mcts.last_path == "fused-mlp"
            assert np.array_equal(roots.tree.distributions().cpu().numpy(), dist.cpu().numpy()), f"step {n}: visits"
            assert np.array_equal(roots.tree.values().cpu().numpy(), vals.cpu().numpy()), f"step {n}: root values"
            roots.clear()


def test_device_collector_cartpole_efficientzero_segments_match_restatement():
    """the zoo's CartPole EfficientZero config through the MuZeroCollector drop-in: the device collector with the
    one-launch EfficientZero MLP search in its captured step; segments identical to the restatement of the
    reference's loop fed the same episodes"""
    from lightzero_amd.envs import DeviceCartPoleEnvManager
    from lightzero_amd.policy import EfficientZeroCollectPolicy, policy_config
    from lightzero_amd.worker import MuZeroCollector
    n, n_ep, S = 8, 12, 10
    cfg = policy_config(num_simulations=S, game_segment_length=10, device=DEV, use_priority=True, n_episode=n,
                        lstm_horizon_len=5)
    col = MuZeroCollector(env=DeviceCartPoleEnvManager(n, seed=3), policy=EfficientZeroCollectPolicy(cfg, _model(2)),
                          policy_config=cfg)
    segs, meta = col.collect(n_episode=n_ep, policy_kwargs=dict(temperature=1.0, epsilon=0.0))
    assert col._device is not None and col._device.search.ez, "the EfficientZero policy did not take the device path"
    assert col._device.search.mcts.last_path == "fused-mlp"
    eps = _played(col.last_schedule)
    assert sum(len(e) for e in eps) == n_ep and all(len(e) >= 1 for e in eps)
    env = EpisodeEnv(eps)
    ref_segs, ref_meta, _ = ref_collect(cfg, env, EpisodeForward(env), n_ep)
    _compare(segs, meta, ref_segs, ref_meta)
    for e in sum(eps, []):
        assert (e["visits"].sum(axis=1) == S).all() and (e["reward"] == 1.0).all()


def test_reanalyze_takes_the_one_launch_path_and_equals_the_oracle():
    """24 roots (the smallest batch with several unroll positions: 4 x (5 + 1)), S 10, ragged legal sets"""
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree
    from lightzero_amd.reanalyze import reanalyze_policy_targets
    from lightzero_amd.utils import EasyDict
    N, A, S, horizon = 24, 2, 10, 5
    model = _model(4)
    rng = np.random.default_rng(1)
    obs = torch.from_numpy(rng.normal(size=(N, 4)).astype(np.float32)).to(DEV)
    mask = np.ones((N, A), np.int8)
    mask[::5, 1] = 0
    mask[::7, 0] = 0
    mask[0] = 1
    pmask = (rng.uniform(size=N) > 0.2).astype(np.int32)
    seeds = torch.arange(S, dtype=torch.int32, device=DEV) * 7919 + 1
    cfg = dict(num_simulations=S, discount_factor=0.997, lstm_horizon_len=horizon,
               model=dict(support_scale=300, categorical_distribution=True))
    info = {}
    target, values = reanalyze_policy_targets(model, obs, torch.from_numpy(mask).to(DEV),
                                              torch.from_numpy(pmask).to(DEV), cfg, seeds=seeds, info=info)
    assert info["last_path"] == "fused-mlp"
    # the same search through the drop-in API, recorded, and the oracle fed its network outputs
    legal = [list(np.nonzero(m)[0]) for m in mask]
    mcfg = EfficientZeroMCTSCtree.default_config()
    mcfg.update(cfg)
    mcfg.device = DEV
    mcts = EfficientZeroMCTSCtree(EasyDict(mcfg))
    mcts.record = True
    tp = np.full(N, -1, np.int32)
    with torch.no_grad():
        o = model.initial_inference(obs)
        roots = EfficientZeroMCTSCtree.roots(N, legal)
        roots.prepare_device(0.0, None, torch.zeros(N, device=DEV), o.policy_logits, torch.from_numpy(tp).to(DEV))
        mcts.search(roots, model, o.latent_state, o.reward_hidden_state, torch.from_numpy(tp).to(DEV), seeds=seeds)
    assert mcts.last_path == "fused-mlp"
    rec = mcts.last_record.numpy() | {"is_reset": mcts.last_record.is_reset.cpu().numpy()}
    disc = np.float32(0.997)
    ot = OracleTree(N, A, S, ez=True)
    la = np.full((N, A), -1, np.int32)
    for i, l in enumerate(legal):
        la[i, :len(l)] = l
    ot.set_legal(la, np.array([len(l) for l in legal], np.int32))
    ot.set_delta(VDM)
    ot.prepare(0.0, None, np.zeros(N, np.float32), o.policy_logits.float().cpu().numpy(), tp)
    for k in range(S):
        x, y, a, vtp, slen = ot.traverse(PB_C_BASE, PB_C_INIT, disc, int(rec["seeds"][k]), tp)
        assert np.array_equal(x, rec["x"][k]) and np.array_equal(a, rec["action"][k]), f"sim {k}"
        assert np.array_equal(slen, rec["search_len"][k]), f"sim {k}"
        is_reset = (slen % horizon == 0).astype(np.int32)
        assert np.array_equal(is_reset, rec["is_reset"][k]), f"sim {k}"
        ot.backprop(k + 1, disc, rec["decoded"][k][:, 0], rec["decoded"][k][:, 1], rec["policy_logits"][k], vtp,
                    is_reset)
    dist = ot.distributions()
    assert np.array_equal(roots.tree.distributions().cpu().numpy(), dist)
    roots.clear()
    tgt = target.cpu().numpy()
    for i in range(N):
        want = np.zeros(A, np.float32)
        if pmask[i]:
            d = np.asarray(dist[i][:len(legal[i])], np.float64)
            for j, a in enumerate(legal[i]):
                want[a] = d[j] / d.sum()
        np.testing.assert_allclose(tgt[i], want, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(values.cpu().numpy(), ot.values(), rtol=0, atol=1e-5)
