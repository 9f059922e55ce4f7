"""Times one Connect4 AlphaZero search (graph=True, 50 simulations) at 512 and 8 boards with the HIP network
(Connect4AZNet.compute_policy_value) and with the torch module's compute_policy_value on the GPU.

Per shape the two variants alternate three times; each turn times five searches with device events and keeps
their median. With --precision split the two variants are the f32 and the split-fp16 HIP networks (five turns). Raw runs go to --out as JSON, the summary to stdout. With --net-only N it only runs the HIP
network N times at --positions (512) positions (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...
--net-only 50).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightzero_amd.alphazero import AlphaZeroMCTS, Connect4AZNet  # noqa: E402
from lightzero_amd.model_az import connect4_alphazero_model  # noqa: E402

SIMS = 50
# conv0 + 4 conv3x3 64->64 + 1x1 heads + the two FC1 per position, multiply-adds x 2
FLOP_PER_POSITION = 2 * (42 * 27 * 64 + 4 * 42 * 576 * 64 + 42 * 64 * 32 + 2 * 672 * 32)


def boards(B, seed=0):
    """positions 0..20 random moves into a game (columns that are full are skipped)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 6, 7), np.int32)
    for b in range(B):
        for k in range(int(rng.integers(0, 21))):
            c = int(rng.integers(0, 7))
            free = np.nonzero(out[b, :, c] == 0)[0]
            if len(free):
                out[b, free[-1], c] = 1 + k % 2
    return out.reshape(B, 42), np.zeros(B, np.int32)


def time_search(mcts, bd, st, pv, n=5):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        mcts.get_next_actions(bd, st, pv, 1.0, True)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="az_connect4_time.json")
    ap.add_argument("--net-only", type=int, default=0)
    ap.add_argument("--positions", type=int, default=512, help="batch of the --net-only calls")
    ap.add_argument("--precision", choices=["f32", "split"], default="f32",
                    help="the HIP network's kernel; split: the searches alternate f32 and split instead of hip and torch")
    args = ap.parse_args()
    torch.manual_seed(0)
    model = connect4_alphazero_model().cuda()
    net = Connect4AZNet(model, precision=args.precision)
    if args.net_only:
        x = torch.rand(args.positions, 3, 6, 7, device="cuda")
        for _ in range(args.net_only):
            net.compute_policy_value(x)
        torch.cuda.synchronize()
        return
    variants = {"hip": net.compute_policy_value, "torch": model.compute_policy_value}
    if args.precision == "split":
        variants = {"f32": Connect4AZNet(model).compute_policy_value, "split": net.compute_policy_value}
    result = {"sims": SIMS, "flop_per_call_512": 512 * FLOP_PER_POSITION, "runs": []}
    for B in (512, 8):
        bd, st = boards(B)
        mcts = {k: AlphaZeroMCTS(None, SIMS, game="connect4", graph=True) for k in variants}
        for k, pv in variants.items():  # capture and warm up
            for _ in range(3):
                mcts[k].get_next_actions(bd, st, pv, 1.0, True)
        torch.cuda.synchronize()
        for turn in range(5 if args.precision == "split" else 3):
            for k, pv in variants.items():
                ms = time_search(mcts[k], bd, st, pv)
                result["runs"].append({"B": B, "variant": k, "turn": turn, "ms": ms})
        for k in variants:
            med = [statistics.median(r["ms"]) for r in result["runs"] if r["B"] == B and r["variant"] == k]
            print(f"B={B} sims={SIMS} {k}: median of 5 per turn {['%.3f' % m for m in med]} ms, "
                  f"median {statistics.median(med):.3f} ms")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
