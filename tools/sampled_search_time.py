"""Times the Sampled EfficientZero search: 256 roots x 50 simulations with the tests' network
(tests/sampled_model.py; latent 16, support 21, LSTM 8), continuous (K, D) = (20, 3) or --discrete (A, K) = (18, 5),
as medians of repeated searches.

Three ways to run the same search:
  graph  SampledEfficientZeroMCTSCtree.search with cfg.use_hip_graph (the loop replayed as one HIP graph);
  eager  the same class, every launch enqueued from the host;
  host   the module-level ezs_tree API driven as the reference drives it (mcts_ctree_sampled.py:133-232): lists in
         and out of batch_traverse / batch_backpropagate, the state pools on the host.

The host loop runs first in a process of its own, then eager and graph in a second one (each child under its own
time limit; a failure ends the run). One JSON line.

With --latent the network is the package's continuous SampledEfficientZeroModelMLP (support 601, K = 20) at that
latent / --lstm width, --dim dimensions and --res residual dynamics, and a third way is timed beside eager and graph:
  one_launch  the same class with cfg.fused_search (lzm_search_mlp_sampled: the whole search in one kernel launch).
The host loop is skipped there.

    python tools/sampled_search_time.py [--discrete] [--roots 256] [--sims 50] [--reps 15]
    python tools/sampled_search_time.py --latent 256 --lstm 256 --dim 4 --res [--roots 8] [--sims 25]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
LATENT, SUPPORT, LSTM, HORIZON = 16, 21, 8, 5


def setup(B, dim, cont):
    import numpy as np
    import torch
    from sampled_model import SampledNet
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    pol = (np.concatenate([rng.normal(size=(B, dim)), rng.uniform(0.3, 1.0, size=(B, dim))], 1) if cont
           else rng.normal(size=(B, dim))).astype(np.float32)
    hidden = (np.zeros((1, B, LSTM), np.float32), np.zeros((1, B, LSTM), np.float32))
    return (SampledNet(LATENT, dim, cont, SUPPORT, lstm=LSTM).cuda().eval(),
            rng.normal(size=(B, LATENT)).astype(np.float32), pol.tolist(), hidden)


def setup_mlp(B, dim, latent, lstm, res):
    """setup()'s tuple with the package's continuous SampledEfficientZeroModelMLP (support 601, random heads)"""
    import numpy as np
    import torch
    from lightzero_amd.model_mlp import SampledEfficientZeroModelMLP
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    pol = np.concatenate([rng.normal(size=(B, dim)), rng.uniform(0.3, 1.0, size=(B, dim))], 1).astype(np.float32)
    hidden = (np.zeros((1, B, lstm), np.float32), np.zeros((1, B, lstm), np.float32))
    model = SampledEfficientZeroModelMLP(observation_shape=4, action_space_size=dim, lstm_hidden_size=lstm,
                                         latent_state_dim=latent, continuous_action_space=True,
                                         last_linear_layer_init_zero=False, res_connection_in_dynamics=res)
    return model.cuda().eval(), rng.normal(size=(B, latent)).astype(np.float32), pol.tolist(), hidden


def median_ms(fn, reps):
    import torch
    times = []
    for r in range(reps + 3):  # three warm-up searches (the graph run captures in its first)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def class_search(B, S, K, dim, cont, graph, inputs=None, record=False, fused=False, support=SUPPORT):
    """run(seeds=None, prepare_seed=None) -> (roots, mcts); inputs, seeds: as host_search's; fused: cfg.fused_search;
    support: the network's support size"""
    from lightzero_amd import SampledEfficientZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    model, lat, pol, hidden = inputs or setup(B, dim, cont)
    mcts = SampledEfficientZeroMCTSCtree(EasyDict(
        num_simulations=S, discount_factor=0.997, device="cuda", use_hip_graph=graph, lstm_horizon_len=HORIZON,
        fused_search=fused,
        model=EasyDict(support_scale=support // 2, categorical_distribution=True, continuous_action_space=cont)))
    roots, mcts.record = mcts.roots(B, [[-1]] * B, dim, K, cont), record

    def run(seeds=None, prepare_seed=None):
        roots.prepare_no_noise([0.0] * B, pol, [-1] * B, seed=prepare_seed)
        mcts.search(roots, model, lat, hidden, [-1] * B, seeds=seeds)
        return roots, mcts
    return run


def host_search(B, S, K, dim, cont, inputs=None):
    """run(seeds=None, prepare_seed=None) -> (roots, [(x, search_lens, last_actions) per simulation]); inputs:
    setup()'s tuple; seeds: per-simulation Philox keys instead of the host seed source (tests)"""
    import numpy as np
    import torch
    from lightzero_amd.ctree import ezs_tree
    from lightzero_amd.scaling_transform import InverseScalarTransform
    model, lat, pol, hidden = inputs or setup(B, dim, cont)
    inv = InverseScalarTransform(SUPPORT // 2, "cuda", True)
    roots = ezs_tree.Roots(B, [[-1]] * B, dim, K, cont)

    def run(seeds=None, prepare_seed=None):
        roots.prepare_no_noise([0.0] * B, pol, [-1] * B, seed=prepare_seed)
        mms = ezs_tree.MinMaxStatsList(B)
        mms.set_delta(0.01)
        pool, cs, hs, trace = [lat], [hidden[0]], [hidden[1]], []
        with torch.no_grad():
            for k in range(S):
                res = ezs_tree.ResultsWrapper(B)
                x, y, acts, vtp = ezs_tree.batch_traverse(roots, 19652, 1.25, 0.997, mms, res, [-1] * B, cont,
                                                          seed=None if seeds is None else int(seeds[k]))
                trace.append((x, res.get_search_len(), acts))
                pick = lambda p: torch.from_numpy(np.asarray([p[ix][iy] for ix, iy in zip(x, y)])).cuda()
                c, h = (torch.from_numpy(np.asarray([p[ix][0][iy] for ix, iy in zip(x, y)])).cuda().unsqueeze(0)
                        for p in (cs, hs))
                a = torch.from_numpy(np.asarray(acts, np.float32)).cuda()
                o = model.recurrent_inference(pick(pool), (c, h), a if cont else a.long().reshape(B))
                reset = np.array(res.get_search_len()) % HORIZON == 0
                state = [s.cpu().numpy() for s in o.reward_hidden_state]
                for s in state:
                    s[:, reset, :] = 0
                pool.append(o.latent_state.cpu().numpy()), cs.append(state[0]), hs.append(state[1])
                ezs_tree.batch_backpropagate(k + 1, 0.997, inv(o.value_prefix).reshape(-1).cpu().tolist(),
                                             inv(o.value).reshape(-1).cpu().tolist(), o.policy_logits.cpu().tolist(),
                                             mms, res, reset.astype(np.int32).tolist(), vtp)
        return roots, trace
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--discrete", action="store_true")
    ap.add_argument("--latent", type=int, default=0)
    ap.add_argument("--lstm", type=int, default=128)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--res", action="store_true")
    ap.add_argument("--child", choices=("host", "device"))
    a = ap.parse_args()
    K, dim, cont = (5, 18, False) if a.discrete else (20, 3, True)
    if a.latent:  # the package's MLP model: eager, graph and the one launch in this process
        inputs = setup_mlp(a.roots, a.dim, a.latent, a.lstm, a.res)
        out = {"roots": a.roots, "sims": a.sims, "K": 20, "dim": a.dim, "latent": a.latent, "lstm": a.lstm,
               "res": a.res, "reps": a.reps}
        for name, graph, fused in (("eager_ms", False, False), ("graph_ms", True, False), ("one_launch_ms", False, True)):
            run = class_search(a.roots, a.sims, 20, a.dim, True, graph, inputs, fused=fused, support=601)
            out[name] = median_ms(run, a.reps)
            out[name.replace("_ms", "_path")] = run()[1].last_path
        out["graph_vs_one_launch"] = out["graph_ms"] / out["one_launch_ms"]
        print(json.dumps(out))
        return
    if a.child == "host":
        print(json.dumps({"host_loop_ms": median_ms(host_search(a.roots, a.sims, K, dim, cont), a.reps)}))
        return
    if a.child == "device":
        print(json.dumps({"eager_ms": median_ms(class_search(a.roots, a.sims, K, dim, cont, False), a.reps),
                          "graph_ms": median_ms(class_search(a.roots, a.sims, K, dim, cont, True), a.reps)}))
        return
    out = {"roots": a.roots, "sims": a.sims, "K": K, "dim_or_actions": dim, "continuous": cont, "reps": a.reps}
    for child, limit in (("host", 240), ("device", 180)):  # each GPU step under its own time limit, chained
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child, "--roots", str(a.roots),
                            "--sims", str(a.sims), "--reps", str(a.reps)] + (["--discrete"] if a.discrete else []),
                           capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.exit(f"{child} run failed ({r.returncode}):\n{r.stderr[-2000:]}")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    out["graph_vs_host_loop"] = out["host_loop_ms"] / out["graph_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
