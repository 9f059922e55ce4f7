"""Times one reanalyze-sized search (default 1,536 roots x 50 simulations: batch_size 256 x (num_unroll_steps + 1)
of the Atari configs) for the Breakout MuZero and the Pong EfficientZero conv models, glibc mode, with device
events on the search's stream. One JSON line per model: the path the search took, the slices, and the
milliseconds of each timed search (roots prepared before the events; the search call alone is timed, the
EfficientZero hand-off guard's synchronise included).

    python tools/reanalyze_search_time.py [--repo DIR] [--sliced 0|1] [--graph 0|1] [--roots N] [--sims S]

--repo: the tree whose lightzero_amd package is imported (default: this script's), so that one script times two
checkouts in alternation; a tree without cfg.sliced_search ignores the key and takes its own path.
"""
import argparse
import json
import os
import sys


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p.add_argument("--sliced", type=int, default=1)
    p.add_argument("--graph", type=int, default=0, help="cfg.use_hip_graph for the per-simulation path")
    p.add_argument("--roots", type=int, default=1536)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--kinds", default="mz,ez")
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    import torch
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree, MuZeroMCTSCtree
    from lightzero_amd.model_conv import atari_efficientzero_model, atari_muzero_model
    from lightzero_amd.utils import EasyDict

    if not torch.cuda.is_available():
        raise SystemExit("reanalyze_search_time: needs a GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    N, S = args.roots, args.sims
    for kind in args.kinds.split(","):
        ez = kind == "ez"
        torch.manual_seed(0)
        model = (atari_efficientzero_model if ez else atari_muzero_model)(last_linear_layer_init_zero=False).to(dev).eval()
        A = model.action_space_size
        cls = EfficientZeroMCTSCtree if ez else MuZeroMCTSCtree
        cfg = cls.default_config()
        cfg.update(dict(num_simulations=S, discount_factor=0.997, device=dev, lstm_horizon_len=5,
                        use_hip_graph=bool(args.graph), sliced_search=bool(args.sliced),
                        model=dict(support_scale=50 if ez else 300, categorical_distribution=True)))
        mcts = cls(EasyDict(cfg))
        rng = np.random.default_rng(0)
        obs = torch.from_numpy(rng.integers(0, 256, size=(N, 4, 64, 64)).astype(np.float32) / 255.0).to(dev)
        noises = torch.from_numpy(rng.dirichlet([0.3] * A, size=N).astype(np.float32)).to(dev)
        tp = torch.full((N,), -1, dtype=torch.int32, device=dev)
        seeds = torch.arange(S, dtype=torch.int32, device=dev) * 7919
        with torch.no_grad():
            outs = [model.initial_inference(obs[i:i + 256]) for i in range(0, N, 256)]
            latent = torch.cat([o.latent_state for o in outs])
            logits = torch.cat([o.policy_logits for o in outs])
            hidden = tuple(torch.cat([o.reward_hidden_state[j] for o in outs], dim=1) for j in range(2)) if ez else None
        ms, visits = [], None
        for it in range(args.warmup + args.reps):
            roots = cls.roots(N, [list(range(A))] * N)
            roots.prepare_device(0.25, noises, torch.zeros(N, device=dev), logits, tp)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if ez:
                mcts.search(roots, model, latent, hidden, tp, seeds=seeds)
            else:
                mcts.search(roots, model, latent, tp, seeds=seeds)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                ms.append(e0.elapsed_time(e1))
            roots.tree.check_errors()
            # a checksum of the visit counts and root values: equal between two checkouts that search alike
            d = roots.tree.distributions().to(torch.int64)
            w = torch.arange(1, N * A + 1, device=dev, dtype=torch.int64).view(N, A)
            visits = [int((d * w).sum().item()), float(roots.tree.values().double().sum().item())]
            roots.clear()
        plan = getattr(mcts, "last_plan", None) or {}
        print(json.dumps(dict(kind=kind, repo=os.path.abspath(args.repo), roots=N, sims=S, graph=args.graph,
                              sliced=args.sliced, path=mcts.last_path, slices=plan.get("slices"),
                              ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3),
                              visits=visits)), flush=True)


if __name__ == "__main__":
    main()
