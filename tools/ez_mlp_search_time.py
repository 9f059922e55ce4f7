"""Times one EfficientZero search over an EfficientZeroModelMLP (glibc mode) with device events on the search's
stream: the one-launch path (lzm_search_mlp_ez, cfg.fused_search on) or the per-simulation path (off), eager or
replayed as a HIP graph (cfg.use_hip_graph). One JSON line: the path taken, the milliseconds of each timed search
(roots prepared before the events; the search call alone is timed) and their median, and a checksum of the visit
counts and root values.

    python tools/ez_mlp_search_time.py [--repo DIR] [--roots N] [--sims S] [--hidden H] [--lstm HL]
                                       [--fused 0|1] [--graph 0|1] [--warmup W] [--reps R]

--repo: the tree whose lightzero_amd package is imported (default: this script's), so that one script times two
checkouts; a tree without EfficientZeroModelMLP gets this tree's model definition and runs its own search path.
A measurement session alternates the builds and settings, one process per line, each under its own time limit:

    for i in 1 2 3; do
      timeout -k 10 120 python tools/ez_mlp_search_time.py --fused 1 &&
      timeout -k 10 120 python tools/ez_mlp_search_time.py --fused 0 --graph 1 &&
      timeout -k 10 120 python tools/ez_mlp_search_time.py --fused 0 --graph 0 || break
    done
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_class(repo):
    from lightzero_amd import model_mlp
    if hasattr(model_mlp, "EfficientZeroModelMLP"):
        return model_mlp.EfficientZeroModelMLP
    # an older tree: this tree's model definition, inside that tree's package (its EZNetworkOutput, its mlp())
    spec = importlib.util.spec_from_file_location("lightzero_amd._ez_model_mlp",
                                                  os.path.join(HERE, "lightzero_amd", "model_mlp.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.EfficientZeroModelMLP


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repo", default=HERE)
    p.add_argument("--roots", type=int, default=256)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--hidden", type=int, default=128)
    p.add_argument("--lstm", type=int, default=128)
    p.add_argument("--actions", type=int, default=2)
    p.add_argument("--fused", type=int, default=1, help="cfg.fused_search")
    p.add_argument("--graph", type=int, default=0, help="cfg.use_hip_graph for the per-simulation path")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    import torch
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree
    from lightzero_amd.utils import EasyDict

    if not torch.cuda.is_available():
        raise SystemExit("ez_mlp_search_time: needs a GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    N, S, A = args.roots, args.sims, args.actions
    torch.manual_seed(0)
    model = model_class(args.repo)(observation_shape=4, action_space_size=A, lstm_hidden_size=args.lstm,
                                   latent_state_dim=args.hidden, last_linear_layer_init_zero=False,
                                   res_connection_in_dynamics=False).to(dev).eval()
    cls = EfficientZeroMCTSCtree
    cfg = cls.default_config()
    cfg.update(dict(num_simulations=S, discount_factor=0.997, device=dev, lstm_horizon_len=5,
                    use_hip_graph=bool(args.graph), fused_search=bool(args.fused),
                    model=dict(support_scale=300, categorical_distribution=True)))
    mcts = cls(EasyDict(cfg))
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.normal(size=(N, 4)).astype(np.float32)).to(dev)
    noises = torch.from_numpy(rng.dirichlet([0.3] * A, size=N).astype(np.float32)).to(dev)
    tp = torch.full((N,), -1, dtype=torch.int32, device=dev)
    seeds = torch.arange(S, dtype=torch.int32, device=dev) * 7919
    with torch.no_grad():
        out = model.initial_inference(obs)
    ms, visits = [], None
    for it in range(args.warmup + args.reps):
        roots = cls.roots(N, [list(range(A))] * N)
        roots.prepare_device(0.25, noises, torch.zeros(N, device=dev), out.policy_logits, tp)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mcts.search(roots, model, out.latent_state, out.reward_hidden_state, tp, seeds=seeds)
        e1.record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
        roots.tree.check_errors()
        d = roots.tree.distributions().to(torch.int64)
        w = torch.arange(1, N * A + 1, device=dev, dtype=torch.int64).view(N, A)
        visits = [int((d * w).sum().item()), float(roots.tree.values().double().sum().item())]
        roots.clear()
    print(json.dumps(dict(repo=os.path.abspath(args.repo), roots=N, sims=S, hidden=args.hidden, lstm=args.lstm,
                          fused=args.fused, graph=args.graph, path=mcts.last_path,
                          ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3),
                          spread_ms=round(float(max(ms) - min(ms)), 3), visits=visits)), flush=True)


if __name__ == "__main__":
    main()
