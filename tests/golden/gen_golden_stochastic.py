"""Generate the Stochastic MuZero golden transcripts tests/golden/stochastic/stmz_*.npz.

Test infrastructure only. Compiles the REFERENCE tree module
``lzero/mcts/ctree/ctree_stochastic_muzero/stochastic_mz_tree.pyx`` from the reference checkout (environment
variable LZ_REFERENCE, default /root/reference) into ``oracle/_ref/`` (git-ignored) with the recipe of
``oracle/build_ref.sh``: ``cython --cplus -3``, then ``g++ -DNDEBUG -fwrapv -O2 -std=c++11`` with
``oracle/ref_time_hook.c`` linked under ``-Wl,--wrap=gettimeofday``, so that the srand(tv_usec) of every
batch_traverse takes a chosen seed. It then drives the module as ``StochasticMuZeroMCTSCtree.search``
(``lzero/mcts/tree_search/mcts_ctree_stochastic.py:116-251``) does — split by leaf kind, two batch_backpropagate
calls with leaf_idx lists — the network replaced by scripted tables that are a function of (simulation, root).

The reference seeds its chance draw from std::random_device. Every chance-node logit row here is one-hot with a
spread of 120: expf underflows to exact zeros, the prior is exactly [.., 1, ..] and the draw is deterministic.

libm entry points the compiled module imports (``nm -D``, printed by this script): expf, logf, sqrtf — the float
forms (cnode.cpp's exp / log / sqrt on float arguments resolve to the <cmath> float overloads); no double exp, log
or sqrt. tests/stochastic_oracle.py restates those.

    python tests/golden/gen_golden_stochastic.py
"""
import ctypes
import os
import subprocess
import sys
import sysconfig

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_DIR = os.path.join(REPO, "oracle", "_ref")
OUT_DIR = os.path.join(HERE, "stochastic")
PB_C_BASE, PB_C_INIT, VDM, NOISE_WEIGHT, ALPHA = 19652, 1.25, 0.01, 0.25, 0.3


def build_reference():
    ref = os.environ.get("LZ_REFERENCE", "/root/reference")
    src = os.path.join(ref, "lzero", "mcts", "ctree", "ctree_stochastic_muzero")
    if not os.path.isdir(src):
        sys.exit(f"{src} not present: the reference checkout is needed to regenerate the goldens")
    bld = os.path.join(REF_DIR, "build")
    os.makedirs(bld, exist_ok=True)
    out = os.path.join(REF_DIR, "stochastic_mz_tree" + sysconfig.get_config_var("EXT_SUFFIX"))
    cpp, hook = os.path.join(bld, "stochastic_mz_tree.cpp"), os.path.join(bld, "ref_time_hook.o")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", os.path.join(REPO, "oracle", "ref_time_hook.c"), "-o", hook])
    subprocess.check_call(["cython", "--cplus", "-3", "-I", src, "-o", cpp, os.path.join(src, "stochastic_mz_tree.pyx")])
    subprocess.check_call(["g++", "-DNDEBUG", "-g0", "-fwrapv", "-O2", "-fPIC", "-shared", "-std=c++11", "-w",
                           "-I" + sysconfig.get_paths()["include"], "-I" + src, cpp, hook,
                           "-Wl,--wrap=gettimeofday", "-o", out])
    syms = subprocess.check_output(["nm", "-D", "--undefined-only", out], text=True).split()
    print("libm imports:", sorted(s.split("@")[0] for s in syms if s.split("@")[0] in
                                  ("exp", "expf", "log", "logf", "sqrt", "sqrtf")))
    return out


def case(name, B, S, A, C, net="rand", noise=False, legal=None, discount=0.997, to_play=None, seed=0):
    return dict(name=name, B=B, S=S, A=A, C=C, net=net, noise=noise, legal=legal, discount=discount,
                to_play=to_play, seed=seed)


CASES = [
    # ragged and permuted root legal lists, B no multiple of 4
    case("stmz_b5_s24_a3_c5", 5, 24, 3, 5, noise=True, legal=[[2, 0, 1], [1], [0, 2], [2, 1], [0, 1, 2]], seed=1),
    case("stmz_b4_s20_a2_c64", 4, 20, 2, 64, seed=2),
    case("stmz_b3_s20_a64_c2", 3, 20, 64, 2, noise=True,
         legal=[list(range(64)), [a for a in range(64) if a % 3], [63, 5]], seed=3),
    case("stmz_deep_b3_s64_a1_c1", 3, 64, 1, 1, seed=4),  # the deepest alternating walk: search_len reaches 64
    case("stmz_2p_b5_s24_a3_c5", 5, 24, 3, 5, to_play=[1, 2, 2, 1, 1], seed=5),
    case("stmz_disc0_b4_s16_a3_c5", 4, 16, 3, 5, discount=0.0, seed=6),
    case("stmz_disc1_b4_s16_a3_c5", 4, 16, 3, 5, discount=1.0, noise=True, seed=7),
    case("stmz_zero_b5_s24_a3_c5", 5, 24, 3, 5, net="zero", legal=[[0, 1, 2], [2, 0], [1], [0, 1, 2], [1, 2]], seed=8),
]


def scripted(c):
    """the inputs of one case: roots, and both head sets for every (simulation, root)"""
    B, S, A, C = c["B"], c["S"], c["A"], c["C"]
    rng = np.random.default_rng(9000 + 31 * c["seed"] + B + 13 * S + A + 7 * C)
    draw = (lambda *s: np.zeros(s, np.float32)) if c["net"] == "zero" else (
        lambda *s: rng.normal(0.0, 1.0, size=s).astype(np.float32))
    legal = c["legal"] or [list(range(A)) for _ in range(B)]
    d = dict(legal_lists=np.full((B, A), -1, np.int32), noises=np.zeros((B, A), np.float32))
    for i, l in enumerate(legal):
        d["legal_lists"][i, :len(l)] = l
        d["noises"][i, :len(l)] = rng.dirichlet([ALPHA] * len(l)).astype(np.float32)
    hot = rng.integers(0, C, size=(S, B))
    d.update(to_play=np.array(c["to_play"] or [-1] * B, np.int32), root_logits=draw(B, A), root_reward=draw(B),
             resp_d_reward=draw(S, B) * np.float32(0.5), resp_d_value=draw(S, B), resp_d_logits=draw(S, B, A),
             resp_c_value=draw(S, B), resp_c_logits=np.full((S, B, C), -60.0, np.float32),
             seeds=np.array([(1000003 * c["seed"] + k) % 1000000 for k in range(S)], np.int64),
             meta=np.array([B, S, A, C, int(c["noise"])], np.int64),
             consts=np.array([PB_C_BASE, PB_C_INIT, np.float32(c["discount"]), VDM, NOISE_WEIGHT], np.float64))
    np.put_along_axis(d["resp_c_logits"], hot[..., None], np.float32(60.0), axis=2)
    return d, legal


def gen_case(c, tree, lib):
    d, legal = scripted(c)
    B, S, A = c["B"], c["S"], c["A"]
    disc, to_play = float(d["consts"][2]), d["to_play"].tolist()
    roots = tree.Roots(B, legal, c["C"])
    if c["noise"]:
        roots.prepare(NOISE_WEIGHT, [d["noises"][i, :len(legal[i])].tolist() for i in range(B)],
                      d["root_reward"].tolist(), d["root_logits"].tolist(), list(to_play))
    else:
        roots.prepare_no_noise(d["root_reward"].tolist(), d["root_logits"].tolist(), list(to_play))
    mms = tree.MinMaxStatsList(B)
    mms.set_delta(VDM)
    req = {k: np.zeros((S, B), np.int32) for k in ("is_chance", "x", "y", "a", "vtp", "len")}
    for k in range(S):
        lib.oracle_set_usec(int(d["seeds"][k]))
        res = tree.ResultsWrapper(num=B)
        ch, x, y, a, vtp = tree.batch_traverse(roots, PB_C_BASE, PB_C_INIT, disc, mms, res, list(to_play))
        for name, v in zip(("is_chance", "x", "y", "a", "vtp"), (ch, x, y, a, vtp)):
            req[name][k] = np.asarray(v, np.int32)
        req["len"][k] = res.get_search_len()
        for kind, rew, val, lg in ((True, np.zeros(B, np.float32), d["resp_c_value"][k], d["resp_c_logits"][k]),
                                   (False, d["resp_d_reward"][k], d["resp_d_value"][k], d["resp_d_logits"][k])):
            idx = [i for i in range(B) if bool(ch[i]) == kind]
            if idx:  # (the chance call is fed the model's reward row too; the tree overwrites it with 0)
                tree.batch_backpropagate(k + 1, disc, rew[idx].tolist(), val[idx].tolist(), lg[idx].tolist(), mms,
                                         res, list(vtp), [kind] * B, idx)
    d.update({"req_" + k: v for k, v in req.items()})
    sys.path.insert(0, os.path.dirname(HERE))
    import stochastic_oracle as so
    d.update(out_dist=so.pad(roots.get_distributions(), A), out_values=np.array(roots.get_values(), np.float32),
             out_traj=so.pad(roots.get_trajectories(), S + 1))
    # whether any tie list held more than one action: a tie-free search is the same under any tie draw
    d["tie_free"] = np.array([so.replay(d, lambda k: (so.glibc_draws(d["seeds"][k]), so.onehot_chance))["ties"] == 0])
    return d


def main():
    so_path = build_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    sys.path.insert(0, REF_DIR)
    sys.path.insert(0, REPO)
    import stochastic_mz_tree  # noqa: E402  (reference build, test infrastructure)
    lib = ctypes.CDLL(so_path)
    lib.oracle_set_usec.argtypes = [ctypes.c_long]
    for c in CASES:
        d = gen_case(c, stochastic_mz_tree, lib)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **d)
        print(f"{c['name']}: max search_len {d['req_len'].max()} chance leaves {d['req_is_chance'].mean():.2f} "
              f"tie_free {bool(d['tie_free'][0])} {os.path.getsize(path)} bytes")
    assert np.load(os.path.join(OUT_DIR, "stmz_deep_b3_s64_a1_c1.npz"))["req_len"].max() == 64


if __name__ == "__main__":
    main()
