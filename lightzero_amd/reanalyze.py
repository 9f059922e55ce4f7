"""Reanalyze: policy targets from a fresh search over replay positions.

Restates the search part of MuZeroGameBuffer._compute_target_policy_reanalyzed
(lzero/mcts/buffer/game_buffer_muzero.py:519-660) and of its EfficientZero form
(game_buffer_efficientzero.py:322-391) on device tensors: initial_inference over the
transition batch (batch_size x (num_unroll_steps + 1) positions, 1,536 at the reference's
defaults) in mini_infer_size slices, roots prepared with or without root noise (`reanalyze_noise`),
one MuZeroMCTSCtree.search — or, for an EfficientZero model, the (h, c) roots concatenated on the batch
axis, the roots prepared with the value-prefix pool and one EfficientZeroMCTSCtree.search(roots, model,
latent, (h, c), to_play) — then per position `visits / sum(visits)` scattered onto the
legal action indices, zeros where `policy_mask` is 0. The search takes the one-launch kernels where the model
has them (the fused kernel for MuZeroModelMLP; the conv kernels over root slices, cfg.sliced_search, which this
module turns on for MuZero models unless the caller's cfg says otherwise and leaves to the caller's cfg for
EfficientZero models, where it measured slower: the same results as the per-simulation path bit for
bit either way). The legal lists are built from the action mask
on the device (Roots.from_action_mask) and the scatter index is that device table, so the call
makes no host round trip. The list bookkeeping around it (game segment indices, child_visit
write-back) stays with the replay buffer (out of scope).
"""
import torch

from .mcts_ctree import EfficientZeroMCTSCtree, MuZeroMCTSCtree
from .utils import EasyDict


def _value_prefix_pool(outs, N, dev):
    """the initial inference's value prefixes as float32 [N] (the model restates the reference's list of zeros)"""
    rows = []
    for o in outs:
        v = o.value_prefix
        rows.append(v.to(dev, torch.float32).reshape(-1) if torch.is_tensor(v)
                    else torch.tensor([float(x) for x in v], dtype=torch.float32, device=dev))
    return torch.cat(rows).reshape(N)


def reanalyze_policy_targets(model, obs, action_mask, policy_mask, cfg, to_play=None, noises=None,
                             noise_weight=0.25, mini_infer_size=None, seeds=None, kind=None, info=None):
    """obs [N, ...] float, action_mask [N, A] {0,1}, policy_mask [N] {0,1} (device tensors).

    cfg: num_simulations, discount_factor, model.support_scale, pb_c_base / pb_c_init /
    value_delta_max (the MCTS classes' defaults otherwise; EfficientZero: lstm_horizon_len too). noises [N, A]
    (Dirichlet, legal order) or None for prepare_no_noise. kind: 'muzero' / 'efficientzero', or None to tell
    by the initial inference's output (an EfficientZero model's carries reward_hidden_state). info: optional
    dict that receives last_path and last_plan of the search. Returns (target_policies [N, A],
    root_values [N]) on the device.
    """
    dev = obs.device
    N = obs.shape[0]
    A = action_mask.shape[1]
    with torch.no_grad():
        step = mini_infer_size or N
        outs = [model.initial_inference(obs[i:i + step]) for i in range(0, N, step)]
        if kind is None:
            kind = 'efficientzero' if getattr(outs[0], 'reward_hidden_state', None) is not None else 'muzero'
        if kind not in ('muzero', 'efficientzero'):
            raise ValueError(f"reanalyze_policy_targets: kind {kind!r} (muzero / efficientzero)")
        ez = kind == 'efficientzero'
        cls = EfficientZeroMCTSCtree if ez else MuZeroMCTSCtree
        mcfg = cls.default_config()
        # Root slices of the one-launch conv search, unless cfg says otherwise: on for MuZero (measured at
        # 1,536 x 50: 10.0 ms against the per-simulation path's 10.4 ms), opt-in for EfficientZero, whose six
        # 256-root launches measured slower than the per-simulation path (15.3 against 12.9 ms)
        mcfg.sliced_search = not ez
        mcfg.update(cfg)
        mcfg.device = dev
        mcts = cls(EasyDict(mcfg))
        latent = torch.cat([o.latent_state for o in outs])
        logits = torch.cat([o.policy_logits for o in outs])
        # MuZero's initial reward is 0; EfficientZero prepares the roots with the value-prefix pool
        rewards = _value_prefix_pool(outs, N, dev) if ez else torch.zeros(N, dtype=torch.float32, device=dev)
        tp = (torch.full((N,), -1, dtype=torch.int32, device=dev) if to_play is None
              else to_play.to(device=dev, dtype=torch.int32))
        # legal lists from the mask on the device (the reference builds them on the host)
        roots = cls._tree.Roots.from_action_mask(action_mask.to(dev), fast_rng=(cls.rng_mode == 'philox'))
        legal_dev = roots._legal_dev[0]
        roots.prepare_device(noise_weight if noises is not None else 0.0,
                             noises if noises is not None else None, rewards, logits, tp)
        if ez:
            # the (h, c) roots of the slices concatenated on the batch axis ([1, n, H] each)
            hidden = tuple(torch.cat([o.reward_hidden_state[j] for o in outs], dim=1) for j in range(2))
            mcts.search(roots, model, latent, hidden, tp, seeds=seeds)
        else:
            mcts.search(roots, model, latent, tp, seeds=seeds)
        if info is not None:
            info.update(last_path=getattr(mcts, "last_path", None), last_plan=getattr(mcts, "last_plan", None))
        t = roots.tree
        dist = t.distributions().to(torch.float32)  # [N, A] in legal order, -1 padded
        values = t.values()
        roots.clear()
        valid = dist >= 0
        vis = torch.where(valid, dist, torch.zeros_like(dist))
        probs = vis / vis.sum(dim=1, keepdim=True).clamp_min(1.0)
        # scatter legal-order probabilities onto action indices (the device legal lists, -1 padded)
        idx = legal_dev.to(torch.int64)
        target = torch.zeros((N, A), dtype=torch.float32, device=dev)
        # padded slots add 0 at index 0 (scatter_add: no write conflicts)
        target.scatter_add_(1, idx.clamp_min(0), torch.where(idx >= 0, probs, torch.zeros_like(probs)))
        target = target * policy_mask.to(dev, torch.float32).unsqueeze(1)
    return target, values
