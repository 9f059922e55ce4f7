"""Times the Stochastic MuZero search over the conv StochasticMuZeroModel (the 2048 config: observation (16, 4, 4),
(A, C, V) = (4, 32, 601), 64 channels, one residual block) on its two per-simulation paths:

  native   cfg.native_network: one lzm_smz_conv_net_step launch per simulation (csrc/lzm_smz_conv.h);
  generic  the torch module, both halves over the whole batch,

both graph-replayed (cfg.use_hip_graph), at 8 roots x 100 simulations (the zoo config) and 256 x 50. DESIGN.md 10's
protocol: device events around the search call alone (roots prepared outside), medians of five after three warm-up
searches, the two paths alternating three times in one session; the generic path's spread is the range of its three
medians. Then the step kernel's own time for P = 1 and P = 2 positions per workgroup at B = 8 and 256 (alternating
kinds), each from `rocprofv3 --kernel-trace --stats` in a run of its own.

Every GPU step is a child process under its own time limit; the first failure ends the run. The raw runs go to
OUT_DIR (default profiles/stochastic_conv).

    python tools/stochastic_conv_time.py [OUT_DIR]
"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
A, C, V = 4, 32, 601


def model():
    import torch
    from lightzero_amd.model_conv import StochasticMuZeroModel
    torch.manual_seed(0)
    return StochasticMuZeroModel((16, 4, 4), A, C, last_linear_layer_init_zero=False).cuda().eval()


def latents(m, B):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1)
    obs = F.one_hot(torch.randint(0, 16, (B, 4, 4), generator=g), 16).permute(0, 3, 1, 2).float().cuda()
    with torch.no_grad():
        return m.representation_network(obs)


def child_search(B, S):
    import numpy as np
    import torch
    from lightzero_amd import StochasticMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    m = model()
    lat = latents(m, B)
    logits = np.random.default_rng(1).normal(size=(B, A)).astype(np.float32).tolist()
    paths = {}
    for name in ("native", "generic"):
        mcts = StochasticMuZeroMCTSCtree(EasyDict(
            num_simulations=S, discount_factor=0.997, device="cuda", use_hip_graph=True,
            native_network=name == "native", model=EasyDict(support_scale=V // 2, categorical_distribution=True)))
        paths[name] = (mcts, mcts.roots(B, [list(range(A))] * B, C))
    for rnd in range(3):
        for name, (mcts, roots) in paths.items():
            ms = []
            for r in range(8):
                roots.prepare_no_noise([0.0] * B, logits, [-1] * B)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mcts.search(roots, m, lat, [-1] * B)
                e1.record()
                torch.cuda.synchronize()
                if r >= 3:
                    ms.append(e0.elapsed_time(e1))
            assert mcts.last_path == ("native-conv" if name == "native" else "generic"), mcts.last_path
            print(json.dumps(dict(roots=B, sims=S, path=name, round=rnd, median_ms=statistics.median(ms), ms=ms)),
                  flush=True)


def child_kernel(B, P):
    import torch
    from lightzero_amd.conv_infer import StochasticConvNet
    m = model()
    net = StochasticConvNet(m)
    pool = latents(m, B).reshape(1, B, 64, 4, 4).contiguous()
    i32 = dict(dtype=torch.int32, device="cuda")
    kind = torch.arange(B, **i32) % 2
    out = net.outputs(B)
    for _ in range(60):
        net.step(pool, torch.zeros(B, **i32), kind, kind, *out, positions=P)
    torch.cuda.synchronize()


def run(cmd, limit):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=REPO)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-1000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child-search":
        return child_search(int(sys.argv[2]), int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-kernel":
        return child_kernel(int(sys.argv[2]), int(sys.argv[3]))
    out = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "stochastic_conv"))
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    runs, summary = [], {}
    for B, S in ((8, 100), (256, 50)):
        rows = [json.loads(l) for l in run(me + ["--child-search", str(B), str(S)], 300).splitlines() if l[:1] == "{"]
        runs += rows
        med = {p: [r["median_ms"] for r in rows if r["path"] == p] for p in ("native", "generic")}
        summary[f"{B}x{S}"] = dict(native_ms=statistics.median(med["native"]),
                                   generic_ms=statistics.median(med["generic"]),
                                   generic_spread_ms=max(med["generic"]) - min(med["generic"]),
                                   native_medians=med["native"], generic_medians=med["generic"])
    for B in (8, 256):
        for P in (1, 2):
            d = os.path.join(out, f"trace_b{B}_p{P}")
            run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "step", "--output-format", "csv", "--"] + me +
                ["--child-kernel", str(B), str(P)], 240)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            rows = [r for f in stats for r in csv.DictReader(open(f)) if "smz_conv_step_kernel" in r["Name"]]
            summary[f"kernel_b{B}_p{P}_us"] = float(rows[0]["AverageNs"]) / 1e3 if rows else None
    with open(os.path.join(out, "searches.json"), "w") as f:
        json.dump(runs, f, indent=1)
    with open(os.path.join(out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
