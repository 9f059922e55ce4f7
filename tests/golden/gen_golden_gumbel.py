"""Generate the Gumbel MuZero golden transcripts tests/golden/gumbel/gmz_*.npz and gmz_tables.npz (a directory
of their own: tests/test_oracle.py and tests/test_gpu_tree.py replay every tests/golden/*.npz they do not know by
prefix as a MuZero / EfficientZero transcript).

Test infrastructure only. Compiles the REFERENCE tree module
``lzero/mcts/ctree/ctree_gumbel_muzero/gmz_tree.pyx`` from the reference checkout (environment
variable LZ_REFERENCE, default /root/reference) into ``oracle/_ref/`` (git-ignored) with the recipe of
``oracle/build_ref.sh`` minus the gettimeofday wrap (the Gumbel tree never draws): ``cython --cplus -3``
then ``g++ -DNDEBUG -fwrapv -O2 -std=c++11``. It then drives the module as
``GumbelMuZeroMCTSCtree.search`` (``lzero/mcts/tree_search/mcts_ctree.py:956-1123``) does, the network
replaced by scripted tables that are a deterministic function of (simulation, root).

Each transcript holds the inputs (legal mask, to_play, noises, root logits / reward / value), per
simulation the requests (x, y, last action, virtual_to_play, search_len) and the fed outputs, and at the
end the distributions, values, policies, children values and trajectories. The reference's MinMaxStatsList has no
getter (and the Gumbel walk never reads it), so the min-max pair is not recorded. Only recorded data is committed.

    python tests/golden/gen_golden_gumbel.py
"""
import os
import subprocess
import sys
import sysconfig

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_DIR = os.path.join(REPO, "oracle", "_ref")
OUT_DIR = os.path.join(HERE, "gumbel")
NOISE_WEIGHT = 0.25
ALPHA = 0.3


def build_reference():
    ref = os.environ.get("LZ_REFERENCE", "/root/reference")
    src = os.path.join(ref, "lzero", "mcts", "ctree", "ctree_gumbel_muzero")
    if not os.path.isdir(src):
        sys.exit(f"{src} not present: the reference checkout is needed to regenerate the goldens")
    os.makedirs(os.path.join(REF_DIR, "build"), exist_ok=True)
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    out = os.path.join(REF_DIR, "gmz_tree" + ext)
    cpp = os.path.join(REF_DIR, "build", "gmz_tree.cpp")
    subprocess.check_call(["cython", "--cplus", "-3", "-I", src, "-o", cpp, os.path.join(src, "gmz_tree.pyx")])
    subprocess.check_call(["g++", "-DNDEBUG", "-g0", "-fwrapv", "-O2", "-fPIC", "-shared", "-std=c++11", "-w",
                           "-I" + sysconfig.get_paths()["include"], "-I" + src, cpp, "-o", out])
    return out


def case(name, B, S, A, m, net="rand", noise=False, legal=None, discount=0.997, to_play=None, seed=0):
    return dict(name=name, B=B, S=S, A=A, m=m, net=net, noise=noise, legal=legal, discount=discount,
                to_play=to_play, seed=seed)


CASES = [
    case("gmz_b8_s25_a2", 8, 25, 2, 2),
    # ragged: a one-action root, a root with fewer legal actions than m (the legal[0] fallback), a full root
    case("gmz_b4_s16_a6", 4, 16, 6, 4, legal=[[0, 1, 2, 3, 4, 5], [1, 4], [3], [0, 2, 5]], seed=1),
    case("gmz_b3_s50_a18", 3, 50, 18, 16, seed=2),
    case("gmz_noise_b4_s20_a5", 4, 20, 5, 4, noise=True, legal=[[0, 1, 2, 3, 4], [0, 2, 3], [1, 2, 3, 4], [0, 4]],
         seed=3),
    case("gmz_m1_b4_s12_a6", 4, 12, 6, 1, seed=4),
    case("gmz_mgts_b4_s5_a3", 4, 5, 3, 16, seed=5),
    case("gmz_s1_b7_a6", 7, 1, 6, 4, seed=6),
    case("gmz_disc1_b4_s20_a4", 4, 20, 4, 4, discount=1.0, seed=7),
    case("gmz_zero_b4_s20_a5", 4, 20, 5, 4, net="zero", legal=[[0, 1, 2, 3, 4], [2, 4], [1, 2, 3], [3]], seed=8),
    case("gmz_2p_b4_s20_a4", 4, 20, 4, 4, to_play=[1, 2, 2, 1], seed=9),
]


def scripted(rng, net, shape):
    if net == "zero":
        return np.zeros(shape, np.float32)
    return rng.normal(0.0, 1.0, size=shape).astype(np.float32)


def gen_case(c, tree):
    B, S, A, m = c["B"], c["S"], c["A"], c["m"]
    disc = float(np.float32(c["discount"]))
    rng = np.random.default_rng(7000 + 31 * c["seed"] + B + 13 * S + A)
    legal = c["legal"] or [list(range(A)) for _ in range(B)]
    legal_mask = np.zeros((B, A), np.int8)
    for i, l in enumerate(legal):
        legal_mask[i, l] = 1
    to_play = c["to_play"] or [-1] * B
    noises = np.zeros((B, A), np.float32)
    for i in range(B):
        n = len(legal[i])
        noises[i, :n] = rng.dirichlet([ALPHA] * n).astype(np.float32)
    root_logits = scripted(rng, c["net"], (B, A))
    root_reward = np.zeros(B, np.float32)
    root_value = scripted(rng, c["net"], (B,))
    resp_reward = scripted(rng, c["net"], (S, B)) * np.float32(0.5)
    resp_value = scripted(rng, c["net"], (S, B))
    resp_logits = scripted(rng, c["net"], (S, B, A))

    roots = tree.Roots(B, legal)
    if c["noise"]:
        roots.prepare(NOISE_WEIGHT, [noises[i, :len(legal[i])].tolist() for i in range(B)], root_reward.tolist(),
                      root_value.tolist(), root_logits.tolist(), list(to_play))
    else:
        roots.prepare_no_noise(root_reward.tolist(), root_value.tolist(), root_logits.tolist(), list(to_play))
    mms = tree.MinMaxStatsList(B)
    mms.set_delta(0.01)
    req = {k: np.zeros((S, B), np.int32) for k in ("x", "y", "a", "vtp", "len")}
    fallback = 0
    table = tree.pget_table_of_considered_visits(m, S)[min(m, S)]
    for k in range(S):
        dist = roots.get_distributions()
        for i in range(B):
            if table[sum(dist[i])] not in dist[i]:
                fallback += 1  # no child has the considered visit count: cselect_root_child keeps legal[0]
        res = tree.ResultsWrapper(num=B)
        x, y, a, vtp = tree.batch_traverse(roots, S, m, disc, res, list(to_play))
        req["x"][k], req["y"][k], req["a"][k], req["vtp"][k] = x, y, a, vtp
        req["len"][k] = res.get_search_len()
        tree.batch_back_propagate(k + 1, disc, resp_reward[k].tolist(), resp_value[k].tolist(),
                                  resp_logits[k].tolist(), mms, res, list(to_play))
    out_dist = np.full((B, A), -1, np.int32)
    for i, d in enumerate(roots.get_distributions()):
        out_dist[i, :len(d)] = d
    trajs = roots.get_trajectories()
    out_traj = np.full((B, max(1, max(len(t) for t in trajs))), -1, np.int32)
    for i, t in enumerate(trajs):
        out_traj[i, :len(t)] = t
    return dict(meta=np.array([B, S, A, m, int(c["noise"])], np.int64),
                consts=np.array([disc, NOISE_WEIGHT], np.float64), legal_mask=legal_mask,
                to_play=np.array(to_play, np.int32), noises=noises, root_logits=root_logits, root_reward=root_reward,
                root_value=root_value, req_x=req["x"], req_y=req["y"], req_a=req["a"], req_vtp=req["vtp"],
                req_len=req["len"], resp_reward=resp_reward, resp_value=resp_value, resp_logits=resp_logits,
                out_dist=out_dist, out_values=np.array(roots.get_values(), np.float32),
                out_policies=np.array(roots.get_policies(disc, A), np.float32),
                out_children_values=np.array(roots.get_children_values(disc, A), np.float32), out_traj=out_traj,
                fallbacks=np.array([fallback], np.int64))


TABLE_MS = [(0, 8), (1, 12), (2, 25), (4, 8), (4, 16), (4, 1), (4, 20), (16, 5), (16, 50), (16, 33), (3, 7), (5, 64)]


def main():
    build_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    sys.path.insert(0, REF_DIR)
    import gmz_tree  # noqa: E402  (reference build, test infrastructure)
    for c in CASES:
        d = gen_case(c, gmz_tree)
        if c["name"] == "gmz_b4_s16_a6":
            assert d["fallbacks"][0] > 0, "the ragged case must reach the legal[0] fallback"
        np.savez_compressed(os.path.join(OUT_DIR, c["name"] + ".npz"), **d)
        print(f"{c['name']}: mean search_len {d['req_len'].mean():.2f} fallbacks {d['fallbacks'][0]}")
    tabs = {"gumbel": np.array(gmz_tree.pgenerate_gumbel(10.0, 0.0, 64), np.float32),
            "ms": np.array(TABLE_MS, np.int64)}
    for m, S in TABLE_MS:
        # the row cselect_root_child reads: table[min(m, S)] (cnode.cpp:727-729)
        tabs[f"row_{m}_{S}"] = np.array(gmz_tree.pget_table_of_considered_visits(m, S)[min(m, S)], np.int32)
    np.savez_compressed(os.path.join(OUT_DIR, "gmz_tables.npz"), **tabs)
    print("gmz_tables.npz written")


if __name__ == "__main__":
    main()
