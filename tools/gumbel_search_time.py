"""Times one search over a MuZeroModelMLP (--model mlp, the default) or over the Breakout conv MuZeroModel of
bench.build_conv_model (--model conv: 64 x 8 x 8 latent, support 601, --actions actions; --hidden is unused) with
device events on the search's stream: GumbelMuZeroMCTSCtree
(--kind gumbel) or MuZeroMCTSCtree (--kind muzero), each on its generic per-simulation path replayed as one HIP
graph (--fused 0, the default: cfg.fused_search off, cfg.use_hip_graph on) or as its one-launch search
(--fused 1: cfg.fused_search on; LZM_FUSED_RES=0 in the environment keeps MuZero on the weight-streaming kernel the
Gumbel search shares). One JSON line: the path taken, the milliseconds of each timed search (roots prepared before
the events; the search call alone is timed), their median, and a checksum of the visit counts and root values.

    python tools/gumbel_search_time.py --kind gumbel|muzero [--model mlp|conv] [--fused 0|1] [--fused-conv]
                                       [--roots N] [--sims S] [--actions A] [--considered M] [--hidden H]
                                       [--graph 0|1] [--warmup W] [--reps R]

--fused-conv (--kind gumbel --model conv): cfg.fused_conv_search on, the one-launch conv Gumbel search
(lzm_search_conv_gumbel); without it the conv model's Gumbel search is the per-simulation loop replayed as one
graph. The conv pair of a session, at both shapes:

    for i in 1 2 3; do
      for s in "4 4" "18 16"; do set -- $s
        timeout -k 10 180 python tools/gumbel_search_time.py --model conv --actions $1 --considered $2 --fused-conv &&
        timeout -k 10 180 python tools/gumbel_search_time.py --model conv --actions $1 --considered $2 || break 2
      done
    done

--considered defaults to min(16, A). A measurement session alternates the variants, one process per line, each
under its own time limit:

    for i in 1 2 3; do
      for a in 2 18; do
        timeout -k 10 120 python tools/gumbel_search_time.py --kind gumbel --fused 1 --actions $a &&
        timeout -k 10 120 python tools/gumbel_search_time.py --kind gumbel --fused 0 --actions $a &&
        LZM_FUSED_RES=0 timeout -k 10 120 python tools/gumbel_search_time.py --kind muzero --fused 1 --actions $a \
          || break 2
      done
    done
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kind", choices=("gumbel", "muzero"), default="gumbel")
    p.add_argument("--model", choices=("mlp", "conv"), default="mlp")
    p.add_argument("--fused-conv", action="store_true", help="cfg.fused_conv_search: the one-launch conv Gumbel search")
    p.add_argument("--roots", type=int, default=256)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--actions", type=int, default=2)
    p.add_argument("--considered", type=int, default=0)
    p.add_argument("--hidden", type=int, default=128)
    p.add_argument("--fused", type=int, default=0, help="cfg.fused_search: the one-launch search where it applies")
    p.add_argument("--graph", type=int, default=1, help="cfg.use_hip_graph")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree, MuZeroMCTSCtree
    from lightzero_amd.model_mlp import MuZeroModelMLP
    from lightzero_amd.utils import EasyDict

    if not torch.cuda.is_available():
        raise SystemExit("gumbel_search_time: needs a GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    N, S, A = args.roots, args.sims, args.actions
    m = args.considered or min(16, A)
    torch.manual_seed(0)
    conv = args.model == "conv"
    if conv:  # bench.build_conv_model's network (atari_muzero_model, random BatchNorm statistics) with A actions
        import bench
        from lightzero_amd.model_conv import atari_muzero_model
        model = atari_muzero_model(action_space_size=A, last_linear_layer_init_zero=False)
        bench._random_bn(model, 1)
        model = model.to(dev).eval()
    else:
        model = MuZeroModelMLP(observation_shape=4, action_space_size=A, latent_state_dim=args.hidden,
                               last_linear_layer_init_zero=False, res_connection_in_dynamics=False).to(dev).eval()
    gumbel = args.kind == "gumbel"
    if args.fused_conv and not (gumbel and conv):
        raise SystemExit("gumbel_search_time: --fused-conv goes with --kind gumbel --model conv")
    cls = GumbelMuZeroMCTSCtree if gumbel else MuZeroMCTSCtree
    cfg = cls.default_config()
    cfg.update(dict(num_simulations=S, max_num_considered_actions=m, discount_factor=0.997, device=dev,
                    use_hip_graph=bool(args.graph), fused_search=bool(args.fused),
                    fused_conv_search=bool(args.fused_conv), env_type='not_board_games',
                    model=dict(support_scale=300, categorical_distribution=True)))
    mcts = cls(EasyDict(cfg))
    rng = np.random.default_rng(0)
    obs = torch.from_numpy((rng.random(size=(N, 4, 64, 64)) if conv else rng.normal(size=(N, 4))).astype(np.float32)).to(dev)
    noises = torch.from_numpy(rng.dirichlet([0.3] * A, size=N).astype(np.float32)).to(dev)
    values = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(dev)
    tp = torch.full((N,), -1, dtype=torch.int32, device=dev)
    seeds = torch.arange(S, dtype=torch.int32, device=dev) * 7919
    with torch.no_grad():
        out = model.initial_inference(obs)
    roots = cls.roots(N, [list(range(A))] * N)  # one Roots object: the same tree, so the graph is captured once
    ms = []
    for it in range(args.warmup + args.reps):
        if gumbel:
            roots.prepare_device(0.25, noises, torch.zeros(N, device=dev), values, out.policy_logits, tp)
        else:
            roots.prepare_device(0.25, noises, torch.zeros(N, device=dev), out.policy_logits, tp)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if gumbel:
            mcts.search(roots, model, out.latent_state, tp)
        else:
            mcts.search(roots, model, out.latent_state, tp, seeds=seeds)
        e1.record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    t = roots.tree
    check = float(t.distributions().clamp(min=0).double().sum().item() + t.values().double().sum().item())
    print(json.dumps(dict(kind=args.kind, model=args.model, fused=bool(args.fused), fused_conv=bool(args.fused_conv),
                          path=mcts.last_path, graph=bool(args.graph), roots=N, sims=S, actions=A,
                          considered=m if gumbel else None, hidden=None if conv else args.hidden,
                          ms=[round(v, 4) for v in ms],
                          median_ms=round(float(np.median(ms)), 4), checksum=check)))


if __name__ == "__main__":
    main()
