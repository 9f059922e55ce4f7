"""Times one CartPole (or, --env breakout, Breakout) collect step of a Gumbel MuZero policy with device events on the
step's stream.

    python tools/gumbel_collect_time.py --variant device|host|muzero [--env cartpole|breakout] [--fused-conv]
                                        [--envs N] [--sims S] [--considered M] [--warmup W] [--reps R]

--env breakout (--variant device or muzero): the Breakout device env with bench.build_conv_model's conv MuZeroModel;
  --fused-conv turns DeviceCollector(fused_conv=True) on: the one-launch conv Gumbel search in the step's graph
  instead of the per-simulation loop.

--variant device: DeviceCollector(algo="gumbel"), one graph replay per step (initial inference, root values, the
  6-argument prepare, the one-launch Gumbel search, lzm_gumbel_collect_outputs, the env kernel).
--variant host:   what a caller has without the device step, run eagerly on the same model and shape: initial
  inference -> InverseScalarTransform -> Roots.prepare_device -> GumbelMuZeroMCTSCtree.search with cfg.fused_search
  on -> the four getters -> the policy rows to the host and np.argmax there. No env step, no recording: it is a
  lower bound of such a caller's step. Only interfaces older than the device step are used.
--variant muzero: DeviceCollector for a MuZero policy at the same shape, for scale.

One JSON line: the milliseconds of each timed step between two events (the host variant also the wall clock, which
includes the copy and the host argmax after the last launch), the median and a checksum. A measurement session
alternates the variants, one process per line, each under its own time limit:

    for i in 1 2 3; do
      for v in device host muzero; do
        timeout -k 10 120 python tools/gumbel_collect_time.py --variant $v || break 2
      done
    done
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--variant", choices=("device", "host", "muzero"), default="device")
    p.add_argument("--env", choices=("cartpole", "breakout"), default="cartpole")
    p.add_argument("--fused-conv", action="store_true", help="DeviceCollector(fused_conv=True)")
    p.add_argument("--envs", type=int, default=256)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--considered", type=int, default=16)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from lightzero_amd.model_mlp import cartpole_muzero_model

    if not torch.cuda.is_available():
        raise SystemExit("gumbel_collect_time: needs a GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    N, S, m, A = args.envs, args.sims, args.considered, 2
    torch.manual_seed(0)
    breakout = args.env == "breakout"
    if breakout:
        if args.variant == "host" or (args.fused_conv and args.variant != "device"):
            raise SystemExit("gumbel_collect_time: --env breakout takes --variant device [--fused-conv] or muzero")
        import bench
        model = bench.build_conv_model(dev, seed=0)
    else:
        model = cartpole_muzero_model(random_heads=True).to(dev).eval()
    ms, wall = [], []

    def timed(fn, it):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
            wall.append((time.perf_counter() - t0) * 1e3)

    if args.variant in ("device", "muzero"):
        from lightzero_amd.collector import DeviceCollector
        kw = dict(algo="gumbel", max_num_considered_actions=m) if args.variant == "device" else {}
        if breakout:
            kw.update(env="breakout", episode_slots=2, max_episode_steps=64)
            if args.variant == "device":
                kw.update(fused_conv=bool(args.fused_conv))
        else:
            kw.update(episode_slots=8)
        col = DeviceCollector(model, N, S, device=dev, seed=0, graph=True, **kw)
        for it in range(args.warmup + args.reps):
            timed(col.step, it)
        path = col.search.mcts.last_path
        check = float(col.rec_visits.double().sum().item() + col.rec_value.double().sum().item())
    else:
        from lightzero_amd.initial import fused_initial_or_none
        from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
        from lightzero_amd.scaling_transform import InverseScalarTransform
        from lightzero_amd.utils import EasyDict
        cfg = GumbelMuZeroMCTSCtree.default_config()
        cfg.update(dict(num_simulations=S, max_num_considered_actions=m, discount_factor=0.997, device=dev,
                        fused_search=True, env_type='not_board_games',
                        model=dict(support_scale=300, categorical_distribution=True)))
        mcts = GumbelMuZeroMCTSCtree(EasyDict(cfg))
        initial = fused_initial_or_none(model) or model
        decode = InverseScalarTransform(300, dev, True)
        rng = np.random.default_rng(0)
        obs = torch.from_numpy(rng.uniform(-0.05, 0.05, size=(N, 4)).astype(np.float32)).to(dev)
        noises = torch.from_numpy(rng.dirichlet([0.3] * A, size=N).astype(np.float32)).to(dev)
        tp = torch.full((N,), -1, dtype=torch.int32, device=dev)
        zeros = torch.zeros(N, device=dev)
        roots = GumbelMuZeroMCTSCtree.roots(N, [list(range(A))] * N)
        disc = float(np.float32(0.997))
        last = {}

        def step():
            with torch.no_grad():
                out = initial.initial_inference(obs)
                roots.prepare_device(0.25, noises, zeros, decode(out.value).reshape(-1), out.policy_logits, tp)
                mcts.search(roots, model, out.latent_state, tp)
                t = roots.tree
                last.update(dist=t.distributions(), values=t.values(), cq=t.children_values(disc))
                last["action"] = np.argmax(t.policies(disc).cpu().numpy(), axis=1)

        for it in range(args.warmup + args.reps):
            timed(step, it)
        path = mcts.last_path
        check = float(last["dist"].double().sum().item() + last["values"].double().sum().item())
    out = dict(variant=args.variant, env=args.env, fused_conv=bool(args.fused_conv), path=path, envs=N, sims=S,
               considered=m if args.variant != "muzero" else None,
               ms=[round(v, 4) for v in ms], median_ms=round(float(np.median(ms)), 4), checksum=check)
    if args.variant == "host":
        out.update(wall_ms=[round(v, 4) for v in wall], median_wall_ms=round(float(np.median(wall)), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
