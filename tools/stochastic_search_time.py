"""Times the Stochastic MuZero search: 256 roots x 50 simulations at (A, C) = (4, 32) with the tests' two-branch
network (tests/stochastic_model.py; latent 16, support 21), as medians of repeated searches.

Three ways to run the same search:
  graph  StochasticMuZeroMCTSCtree.search with cfg.use_hip_graph (the loop replayed as one HIP graph);
  eager  the same class, every launch enqueued from the host;
  host   the module-level stochastic_mz_tree API driven as the reference drives it: split by leaf kind on the host,
         two sub-batch model calls and two batch_backpropagate calls with leaf_idx lists per simulation.

The host loop runs first in a process of its own, then eager and graph in a second one (each child under its own
time limit; a failure ends the run). One JSON line per process, then the graph-against-host-loop ratio.

    python tools/stochastic_search_time.py [--roots 256] [--sims 50] [--reps 15]
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
A, C, LATENT, SUPPORT = 4, 32, 16, 21


def setup(B):
    import numpy as np
    import torch
    from stochastic_model import TwoBranchNet
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    return (TwoBranchNet(LATENT, A, C, SUPPORT).cuda().eval(), rng.normal(size=(B, LATENT)).astype(np.float32),
            rng.normal(size=(B, A)).astype(np.float32).tolist())


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


def class_search(B, S, graph):
    from lightzero_amd import StochasticMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    model, lat, logits = setup(B)
    mcts = StochasticMuZeroMCTSCtree(EasyDict(
        num_simulations=S, discount_factor=0.997, device="cuda", use_hip_graph=graph,
        model=EasyDict(support_scale=SUPPORT // 2, categorical_distribution=True)))
    roots = mcts.roots(B, [list(range(A))] * B, C)

    def run():
        roots.prepare_no_noise([0.0] * B, logits, [-1] * B)
        mcts.search(roots, model, lat, [-1] * B)
    return run


def host_search(B, S):
    import numpy as np
    import torch
    from lightzero_amd.ctree import stochastic_mz_tree as st
    from lightzero_amd.scaling_transform import InverseScalarTransform
    model, lat, logits = setup(B)
    inv = InverseScalarTransform(SUPPORT // 2, "cuda", True)
    roots = st.Roots(B, [list(range(A))] * B, C)

    def run():
        roots.prepare_no_noise([0.0] * B, logits, [-1] * B)
        mms = st.MinMaxStatsList(B)
        mms.set_delta(0.01)
        pool = [lat]
        with torch.no_grad():
            for k in range(S):
                res = st.ResultsWrapper(B)
                ch, x, y, a, vtp = st.batch_traverse(roots, 19652, 1.25, 0.997, mms, res, [-1] * B)
                states = torch.from_numpy(np.asarray([pool[ix][iy] for ix, iy in zip(x, y)])).cuda()
                acts = torch.from_numpy(np.asarray(a)).cuda().long()
                nxt = np.zeros((B, LATENT), np.float32)
                for kind in (True, False):
                    idx = [i for i in range(B) if ch[i] == kind]
                    if not idx:
                        continue
                    o = model.recurrent_inference(states[idx], acts[idx], afterstate=not kind)
                    nxt[idx] = o.latent_state.cpu().numpy()
                    st.batch_backpropagate(k + 1, 0.997, inv(o.reward).reshape(-1).cpu().tolist(),
                                           inv(o.value).reshape(-1).cpu().tolist(), o.policy_logits.cpu().tolist(),
                                           mms, res, vtp, [kind] * B, idx)
                pool.append(nxt)
    return run


def one_launch_compare(out_path):
    """--one-launch: the one-launch search (cfg.fused_search, lzm_search_mlp_stoch) against the graph-replayed
    per-simulation path over a StochasticMuZeroModelMLP of the zoo widths (latent 128, support 601), at 256 roots x
    50 simulations and 8 x 25, (A, C) = (2, 2) and (4, 2). DESIGN.md 10's protocol: device events around the search
    call alone (roots prepared outside), medians of five after three warm-up searches, the two paths alternating
    three times in one session. Every run is kept in out_path."""
    import numpy as np
    import torch
    from lightzero_amd import StochasticMuZeroMCTSCtree
    from lightzero_amd.model_mlp import StochasticMuZeroModelMLP
    from lightzero_amd.utils import EasyDict
    runs = []
    for (B, S) in ((256, 50), (8, 25)):
        for (na, nc) in ((2, 2), (4, 2)):
            torch.manual_seed(0)
            rng = np.random.default_rng(1)
            model = StochasticMuZeroModelMLP(observation_shape=4, action_space_size=na, chance_space_size=nc,
                                             latent_state_dim=128, last_linear_layer_init_zero=False).cuda().eval()
            lat = torch.from_numpy(rng.normal(size=(B, 128)).astype(np.float32)).cuda()
            logits = rng.normal(size=(B, na)).astype(np.float32).tolist()
            paths = {}
            for name, extra in (("one_launch", dict(fused_search=True)), ("graph", dict(use_hip_graph=True))):
                mcts = StochasticMuZeroMCTSCtree(EasyDict(
                    num_simulations=S, discount_factor=0.997, device="cuda",
                    model=EasyDict(support_scale=300, categorical_distribution=True), **extra))
                paths[name] = (mcts, mcts.roots(B, [list(range(na))] * B, nc))
            for rnd in range(3):
                for name, (mcts, roots) in paths.items():
                    ms = []
                    for r in range(8):
                        roots.prepare_no_noise([0.0] * B, logits, [-1] * B)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        mcts.search(roots, model, lat, [-1] * B)
                        e1.record()
                        torch.cuda.synchronize()
                        if r >= 3:
                            ms.append(e0.elapsed_time(e1))
                    assert mcts.last_path == ("fused-mlp" if name == "one_launch" else "generic"), mcts.last_path
                    runs.append(dict(roots=B, sims=S, actions=na, chance=nc, path=name, round=rnd,
                                     median_ms=statistics.median(ms), ms=ms))
                    print(json.dumps(runs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(runs, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--child", choices=("host", "device"))
    ap.add_argument("--one-launch", metavar="OUT.json", help="time the one-launch search against the graph path")
    a = ap.parse_args()
    if a.one_launch:
        return one_launch_compare(a.one_launch)
    if a.child == "host":
        print(json.dumps({"host_loop_ms": median_ms(host_search(a.roots, a.sims), a.reps)}))
        return
    if a.child == "device":
        print(json.dumps({"eager_ms": median_ms(class_search(a.roots, a.sims, False), a.reps),
                          "graph_ms": median_ms(class_search(a.roots, a.sims, True), a.reps)}))
        return
    out = {"roots": a.roots, "sims": a.sims, "actions": A, "chance": C, "reps": a.reps}
    for child, limit in (("host", 240), ("device", 180)):  # each GPU step under its own time limit, chained
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child, "--roots", str(a.roots),
                            "--sims", str(a.sims), "--reps", str(a.reps)], capture_output=True, text=True,
                           timeout=limit)
        if r.returncode != 0:
            sys.exit(f"{child} run failed ({r.returncode}):\n{r.stderr[-2000:]}")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    out["graph_vs_host_loop"] = out["host_loop_ms"] / out["graph_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
