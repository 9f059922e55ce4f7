"""GPU: reanalyze_policy_targets for the conv models — the EfficientZero form (game_buffer_efficientzero.py:
322-391: (h, c) roots, value-prefix pool, EfficientZeroMCTSCtree.search) and the MuZero form — with the searches
on the one-launch kernels over root slices (cfg.sliced_search: reanalyze's own default for MuZero models, set by
the caller for EfficientZero; sliced_search_max_roots 64 makes three / two slices out of 130 / 70 positions). Ragged action masks, a policy_mask with zeros. The targets
and root values equal those computed from a direct search() on the generic path (fused_search off) from the same
roots and seeds: root values array-equal, targets within tests/test_gpu_reanalyze.py's rtol 1e-6 / atol 1e-7
(the float32 division against a float64 one)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_conv import DEV  # noqa: E402
from tests.test_gpu_conv_shapes import make_model  # noqa: E402


@pytest.mark.parametrize("kind,N,slices", [("ez", 130, 3), ("mz", 70, 2)])
def test_reanalyze_conv_targets_equal_generic_search(kind, N, slices):
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree, MuZeroMCTSCtree
    from lightzero_amd.reanalyze import reanalyze_policy_targets
    from lightzero_amd.utils import EasyDict
    S = 8
    ez = kind == "ez"
    model = make_model(kind, 51, **(dict(H=128) if ez else {}))
    A = model.action_space_size
    cls = EfficientZeroMCTSCtree if ez else MuZeroMCTSCtree
    rng = np.random.default_rng(2)
    obs = torch.from_numpy(rng.integers(0, 256, size=(N, 4, 64, 64)).astype(np.float32) / 255.0).to(DEV)
    mask = np.ones((N, A), np.int8)
    mask[::5, 1] = 0  # ragged legal sets
    mask[::7, 0] = 0
    mask[3, :A - 1] = 0  # one legal action
    pmask = (rng.uniform(size=N) > 0.2).astype(np.int32)
    assert (pmask == 0).any() and (pmask == 1).any()
    seeds = torch.arange(S, dtype=torch.int32, device=DEV) * 7919 + 3
    scale = 50 if ez else 300
    cfg = dict(num_simulations=S, discount_factor=0.997, lstm_horizon_len=5, sliced_search_max_roots=64,
               model=dict(support_scale=scale, categorical_distribution=True))
    if ez:  # (reanalyze turns the key on by itself for MuZero models only: EfficientZero's slices measured slower)
        cfg["sliced_search"] = True
    info = {}
    target, values = reanalyze_policy_targets(model, obs, torch.from_numpy(mask).to(DEV),
                                              torch.from_numpy(pmask).to(DEV), cfg, seeds=seeds, mini_infer_size=48,
                                              info=info)
    name = "fused" if ez else "fused-conv"
    assert info["last_path"] == f"{name} ({slices} slices)", info["last_path"]
    assert info["last_plan"]["slices"] == slices and info["last_plan"]["slice_roots"] == 64
    # the same search through the drop-in API on the generic path
    legal = [list(np.nonzero(m)[0]) for m in mask]
    mcfg = cls.default_config()
    mcfg.update(cfg)
    mcfg.update(dict(fused_search=False, device=DEV))
    mcts = cls(EasyDict(mcfg))
    with torch.no_grad():
        outs = [model.initial_inference(obs[i:i + 48]) for i in range(0, N, 48)]  # (the same inference slices)
        latent = torch.cat([o.latent_state for o in outs])
        logits = torch.cat([o.policy_logits for o in outs])
        roots = cls.roots(N, legal)
        tp = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        roots.prepare_device(0.0, None, torch.zeros(N, device=DEV), logits, tp)
        if ez:
            hidden = tuple(torch.cat([o.reward_hidden_state[j] for o in outs], dim=1) for j in range(2))
            mcts.search(roots, model, latent, hidden, tp, seeds=seeds)
        else:
            mcts.search(roots, model, latent, tp, seeds=seeds)
        assert mcts.last_path == "generic"
        dist = roots.get_distributions()
        vals = roots.get_values()
        roots.clear()
    tgt = target.cpu().numpy()
    for i in range(N):
        want = np.zeros(A, np.float32)
        if pmask[i]:
            d = np.asarray(dist[i], np.float64)
            assert d.sum() == S
            for j, a in enumerate(legal[i]):
                want[a] = d[j] / d.sum()
        np.testing.assert_allclose(tgt[i], want, rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(values.cpu().numpy(), np.asarray(vals, np.float32))
