"""Times one fused CartPole-shape MuZero search (default 256 roots x 50 simulations, glibc mode) whose value,
reward and policy heads have their last layers scaled (default x30): the closest thing here to a trained
network's confident heads, where most walks score a node with one visited child and so evaluate the mean-q
chain (bench.py's random heads end 59% of their walks in a leaf tie instead). Device events on the search's
stream, the search call alone; one JSON line with each timed search's milliseconds, the median, and a
checksum of the visit counts and root values (equal between two libraries that search alike).

    LZM_LIB=lightzero_amd/liblzm_varP.so python tools/sharp_search_time.py [--scale 30] [--roots 256] [--sims 50]

The library is the one LZM_LIB names (tools/build_variant.sh), so parent and new alternate as processes.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=float, default=30.0)
    p.add_argument("--roots", type=int, default=256)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    import numpy as np
    import torch
    from lightzero_amd.mcts_ctree import MuZeroMCTSCtree
    from lightzero_amd.model_mlp import MuZeroModelMLP
    from lightzero_amd.utils import EasyDict

    if not torch.cuda.is_available():
        raise SystemExit("sharp_search_time: needs a GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    B, S, A = args.roots, args.sims, 2
    torch.manual_seed(0)
    model = MuZeroModelMLP(observation_shape=4, action_space_size=A, latent_state_dim=128, categorical_distribution=True,
                           reward_support_size=601, value_support_size=601, last_linear_layer_init_zero=False,
                           norm_type='BN', res_connection_in_dynamics=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
        for seq in (model.prediction_network.fc_value_head, model.dynamics_network.fc_reward_head,
                    model.prediction_network.fc_policy_head):
            lin = [m for m in seq.modules() if isinstance(m, torch.nn.Linear)][-1]
            lin.weight.mul_(args.scale)
            lin.bias.mul_(args.scale)
    model = model.to(dev).eval()
    cfg = MuZeroMCTSCtree.default_config()
    cfg.update(dict(num_simulations=S, discount_factor=0.997, device=dev,
                    model=dict(support_scale=300, categorical_distribution=True)))
    mcts = MuZeroMCTSCtree(EasyDict(cfg))
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.normal(size=(B, 4)).astype(np.float32)).to(dev)
    noises = torch.from_numpy(rng.dirichlet([0.3] * A, size=B).astype(np.float32)).to(dev)
    tp = torch.full((B,), -1, dtype=torch.int32, device=dev)
    seeds = torch.arange(S, dtype=torch.int32, device=dev) * 7919
    with torch.no_grad():
        out = model.initial_inference(obs)
    ms, visits = [], None
    for it in range(args.warmup + args.reps):
        roots = MuZeroMCTSCtree.roots(B, [list(range(A))] * B)
        roots.prepare_device(0.25, noises, torch.zeros(B, device=dev), out.policy_logits, tp)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mcts.search(roots, model, out.latent_state, tp, seeds=seeds)
        e1.record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
        roots.tree.check_errors()
        d = roots.tree.distributions().to(torch.int64)
        w = torch.arange(1, B * A + 1, device=dev, dtype=torch.int64).view(B, A)
        visits = [int((d * w).sum().item()), float(roots.tree.values().double().sum().item())]
        roots.clear()
    if mcts.last_path != "fused-mlp":
        raise SystemExit(f"sharp_search_time: the search took the {mcts.last_path} path, not the fused one")
    print(json.dumps(dict(lib=os.environ.get("LZM_LIB", "default"), scale=args.scale, roots=B, sims=S, path=mcts.last_path,
                          ms=[round(x, 4) for x in ms], median_ms=round(float(np.median(ms)), 4), visits=visits)),
          flush=True)


if __name__ == "__main__":
    main()
