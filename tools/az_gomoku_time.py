"""Times one Gomoku AlphaZero search (graph=True, 50 simulations) at 32 boards (the config's collector batch) and 512
boards with the HIP network (GomokuAZNet.compute_policy_value) and with the torch module's compute_policy_value on
the GPU.

Per shape the two variants alternate three times; each turn times five searches with device events and keeps their
median. Raw runs go to --out as JSON, the summary to stdout. --instantiations also times the network alone (device
events around 200 launches) at --net-batches for every built positions-per-workgroup instantiation
(LZM_GMK_NET_POSITIONS), alternating three times. With --net-only N it only runs the HIP network N times at
--positions positions under the environment's instantiation (for a kernel trace: rocprofv3 --kernel-trace --stats
-- python ... --net-only 50). --board-size 9 / 15 times the lzm_az_gmkn_* family, which builds one position per
workgroup only. With --precision split (board sizes 9 and 15) the two search variants are the f32 and the split-fp16
HIP networks, alternating five times, and the network alone is timed at --net-batches for both, alternating three
times.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightzero_amd.alphazero import AlphaZeroMCTS, GomokuAZNet  # noqa: E402
from lightzero_amd.model_az import gomoku_alphazero_model  # noqa: E402

SIMS = 50


def flop_per_position(cells):
    """conv0 + 4 conv3x3 32->32 + 1x1 heads + the two FC1 per position, multiply-adds x 2"""
    return 2 * (cells * 27 * 32 + 4 * cells * 288 * 32 + cells * 32 * 32 + 2 * 16 * cells * 32)


def boards(B, seed=0, cells=36):
    """positions 0..15 random stones into a game"""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, cells), np.int32)
    for b in range(B):
        for k, c in enumerate(rng.permutation(cells)[:int(rng.integers(0, 16))]):
            out[b, c] = 1 + k % 2
    return out, np.zeros(B, np.int32)


def time_search(mcts, bd, st, pv, n=5):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        mcts.get_next_actions(bd, st, pv, 1.0, True)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def time_net(net, x, launches=200):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        net.compute_policy_value(x)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3  # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="az_gomoku_time.json")
    ap.add_argument("--net-only", type=int, default=0)
    ap.add_argument("--positions", type=int, default=512, help="batch of the --net-only calls")
    ap.add_argument("--instantiations", action="store_true")
    ap.add_argument("--net-batches", type=int, nargs="*", default=[32, 128, 256, 512, 1024, 2048, 4096])
    ap.add_argument("--board-size", type=int, default=6, choices=[6, 9, 15])
    ap.add_argument("--precision", choices=["f32", "split"], default="f32",
                    help="the HIP network's kernel; split: the searches alternate f32 and split instead of hip and torch")
    args = ap.parse_args()
    N = args.board_size
    split = args.precision == "split"
    env = "LZM_GMK_NET_POSITIONS"  # read by the 6 x 6 family only
    built = ("1", "2") if N == 6 else ("1",)
    torch.manual_seed(0)
    model = gomoku_alphazero_model(board_size=N).cuda()
    net = GomokuAZNet(model, precision=args.precision)
    if args.net_only:
        x = torch.rand(args.positions, 3, N, N, device="cuda")
        for _ in range(args.net_only):
            net.compute_policy_value(x)
        torch.cuda.synchronize()
        return
    result = {"sims": SIMS, "board_size": N, "flop_per_position": flop_per_position(N * N), "runs": [], "net_us": []}
    if args.instantiations:
        forced = os.environ.pop(env, None)
        for n in args.net_batches:
            x = torch.rand(n, 3, N, N, device="cuda")
            for turn in range(3):
                for p in built:
                    os.environ[env] = p
                    if turn == 0:
                        time_net(net, x, 20)
                    result["net_us"].append({"n": n, "positions": int(p), "turn": turn, "us": time_net(net, x)})
            os.environ.pop(env)
            for p in map(int, built):
                us = [r["us"] for r in result["net_us"] if r["n"] == n and r["positions"] == p]
                print(f"net n={n} positions/workgroup={p}: {['%.2f' % u for u in us]} us per launch")
        if forced is not None:
            os.environ[env] = forced
    variants = {"hip": net.compute_policy_value, "torch": model.compute_policy_value}
    if split:
        nets = {"f32": GomokuAZNet(model), "split": net}
        variants = {k: v.compute_policy_value for k, v in nets.items()}
        for n in args.net_batches:
            x = torch.rand(n, 3, N, N, device="cuda")
            for turn in range(3):
                for k, v in nets.items():
                    if turn == 0:
                        time_net(v, x, 20)
                    result["net_us"].append({"n": n, "variant": k, "turn": turn, "us": time_net(v, x)})
            for k in nets:
                us = [r["us"] for r in result["net_us"] if r["n"] == n and r.get("variant") == k]
                print(f"net n={n} {k}: {['%.2f' % u for u in us]} us per launch")
    for B in (32, 512):
        bd, st = boards(B, cells=N * N)
        mcts = {k: AlphaZeroMCTS(None, SIMS, game="gomoku", graph=True, board_size=N) for k in variants}
        for k, pv in variants.items():  # capture and warm up
            for _ in range(3):
                mcts[k].get_next_actions(bd, st, pv, 1.0, True)
        torch.cuda.synchronize()
        for turn in range(5 if split else 3):
            for k, pv in variants.items():
                ms = time_search(mcts[k], bd, st, pv)
                result["runs"].append({"B": B, "variant": k, "turn": turn, "ms": ms})
        for k in variants:
            med = [statistics.median(r["ms"]) for r in result["runs"] if r["B"] == B and r["variant"] == k]
            allms = [m for r in result["runs"] if r["B"] == B and r["variant"] == k for m in r["ms"]]
            print(f"B={B} sims={SIMS} {k}: median of 5 per turn {['%.3f' % m for m in med]} ms, "
                  f"median {statistics.median(med):.3f} ms, all runs {min(allms):.3f} .. {max(allms):.3f} ms")
    if split:
        result["range_errors"] = net.range_errors()
        print(f"range errors: {result['range_errors']}")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
