"""Generate the Gumbel MuZero golden transcripts tests/golden/gumbel/gmz_*.npz, gmz_tables.npz and
gmz_visits_full.npz (a directory of their own: tests/test_oracle.py and tests/test_gpu_tree.py replay every tests/golden/*.npz they do not know by
prefix as a MuZero / EfficientZero transcript).

Test infrastructure only. Compiles the REFERENCE tree module
``lzero/mcts/ctree/ctree_gumbel_muzero/gmz_tree.pyx`` from the reference checkout (environment
variable LZ_REFERENCE, default /root/reference) into ``oracle/_ref/`` (git-ignored) with the recipe of
``oracle/build_ref.sh`` minus the gettimeofday wrap (the Gumbel tree never draws): ``cython --cplus -3``
then ``g++ -DNDEBUG -fwrapv -O2 -std=c++11``. It then drives the module as
``GumbelMuZeroMCTSCtree.search`` (``lzero/mcts/tree_search/mcts_ctree.py:956-1123``) does, the network
replaced by scripted tables that are a deterministic function of (simulation, root).

Each transcript holds the inputs (legal mask, to_play, noises, root logits / reward / value; the edge cases of
EDGE_CASES also the ordered legal lists, which a mask cannot express), per
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


def case(name, B, S, A, m, net="rand", noise=False, legal=None, discount=0.997, to_play=None, seed=0, values=None):
    """net: the fill kind of the logits (root_logits, resp_logits); values: that of reward and value (default: net)"""
    return dict(name=name, B=B, S=S, A=A, m=m, net=net, values=net if values is None else values, noise=noise,
                legal=legal, discount=discount, to_play=to_play, seed=seed)


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


def rng_(a, b):
    return list(range(a, b))


A64_RAGGED = [rng_(0, 64), [a for a in range(64) if a % 3 != 0], [63]]
PERM9 = [rng_(0, 9)[::-1], [8, 2], [5, 0, 7, 1, 3], [4]]

# The float, shape and legal-list edges. Their transcripts also store the ordered legal lists.
EDGE_CASES = [
    # A = 64 (every lane), ragged roots that miss action 0 or hold only action 63
    case("gmz_a64_b3_s64", 3, 64, 64, 16, legal=A64_RAGGED, seed=10),
    case("gmz_a64_noise_b5_s40", 5, 40, 64, 16, net="sharp", values="rand", noise=True,
         legal=A64_RAGGED + [[5, 63], rng_(1, 64)], seed=11),
    # legal lists that are not ascending: lane j is legal position j
    case("gmz_perm_b4_s33_a9", 4, 33, 9, 7, legal=PERM9, seed=12),
    case("gmz_perm_noise_b3_s20_a64", 3, 20, 64, 16, noise=True,
         legal=[rng_(0, 64)[::-1], [63, 0, 31], [40, 2, 17, 9, 63, 1]], seed=13),
    # a walk as deep as the tree allows
    case("gmz_a1_deep_b3_s64", 3, 64, 1, 4, seed=14),
    case("gmz_a2_deep_b3_s64", 3, 64, 2, 2, net="zero", seed=15),
    # float regimes of the completed Q
    case("gmz_sharp_b4_s30_a6", 4, 30, 6, 4, net="sharp", values="rand", seed=16),
    case("gmz_big_b4_s30_a6", 4, 30, 6, 4, values="big", seed=17),
    case("gmz_huge_b4_s30_a6", 4, 30, 6, 4, values="huge", seed=18),
    case("gmz_const_b4_s30_a6", 4, 30, 6, 4, values="const", seed=19),
    case("gmz_tiny_b4_s30_a6", 4, 30, 6, 4, values="tiny", seed=20),
    case("gmz_near_b4_s30_a6", 4, 30, 6, 4, values="near", seed=21),
    case("gmz_denorm_b4_s30_a6", 4, 30, 6, 4, values="denorm", seed=22),
    case("gmz_quant_b6_s40_a5", 6, 40, 5, 4, net="quant", seed=23),
    # sequential halving: m no power of two, m = 0, m = 64
    case("gmz_m2_b4_s24_a7", 4, 24, 7, 2, seed=24),
    case("gmz_m3_b4_s24_a7", 4, 24, 7, 3, seed=25),
    case("gmz_m5_b4_s64_a9", 4, 64, 9, 5, seed=26),
    case("gmz_m7_rag_b4_s33_a9", 4, 33, 9, 7, legal=[rng_(0, 9), [2, 8], [0, 1, 3, 5, 7], [4]], seed=27),
    case("gmz_m64_b3_s64_a64", 3, 64, 64, 64, seed=28),
    case("gmz_m0_b4_s10_a4", 4, 10, 4, 0, seed=29),
    case("gmz_m6_a64_b4_s64", 4, 64, 64, 6, net="sharp", values="big", noise=True,
         legal=[rng_(0, 64), rng_(32, 64), [0, 63], rng_(0, 64)[::2]], seed=30),
    case("gmz_2p_rag_b5_s20_a5", 5, 20, 5, 3, net="quant", legal=[rng_(0, 5), [1, 3], [4], [0, 2, 4], [2, 3]],
         to_play=[1, 2, 1, 2, 1], seed=31),
    case("gmz_b70_s12_a3", 70, 12, 3, 4, seed=32),
    case("gmz_disc0_b4_s20_a4", 4, 20, 4, 4, discount=0.0, seed=33),
]


def scripted(rng, kind, shape):
    """an N(0, 1) draw, scaled or replaced by the fill kind after it is drawn ("zero" draws nothing)"""
    if kind == "zero":
        return np.zeros(shape, np.float32)
    x = rng.normal(0.0, 1.0, size=shape).astype(np.float32)
    f = np.float32
    if kind == "rand":
        return x
    if kind == "sharp":   # logit spreads past 104: expf underflows, priors become exact zeros
        return x * f(60.0)
    if kind == "big":
        return x * f(1e5)
    if kind == "huge":
        return x * f(1e30)
    if kind == "const":   # all completed Q equal over a non-zero numerator
        return np.full(shape, 0.37, np.float32)
    if kind == "tiny":    # differences far below one ulp of 0.5: equal after rounding
        return (f(0.5) + f(1e-9) * x).astype(np.float32)
    if kind == "near":    # one or two ulps of 0.5 apart
        return (f(0.5) + f(6e-8) * np.rint(f(2.0) * x)).astype(np.float32)
    if kind == "denorm":
        return (f(1e-40) * x).astype(np.float32)
    if kind == "quant":   # a half-integer grid: many exact ties
        return (np.rint(f(2.0) * x) / f(2.0)).astype(np.float32)
    raise ValueError(kind)


def gen_case(c, tree, edge=False):
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
    root_value = scripted(rng, c["values"], (B,))
    resp_reward = scripted(rng, c["values"], (S, B)) * np.float32(0.5)
    resp_value = scripted(rng, c["values"], (S, B))
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
    d = dict(meta=np.array([B, S, A, m, int(c["noise"])], np.int64),
                consts=np.array([disc, NOISE_WEIGHT], np.float64), legal_mask=legal_mask,
                to_play=np.array(to_play, np.int32), noises=noises, root_logits=root_logits, root_reward=root_reward,
                root_value=root_value, req_x=req["x"], req_y=req["y"], req_a=req["a"], req_vtp=req["vtp"],
                req_len=req["len"], resp_reward=resp_reward, resp_value=resp_value, resp_logits=resp_logits,
                out_dist=out_dist, out_values=np.array(roots.get_values(), np.float32),
                out_policies=np.array(roots.get_policies(disc, A), np.float32),
                out_children_values=np.array(roots.get_children_values(disc, A), np.float32), out_traj=out_traj,
                fallbacks=np.array([fallback], np.int64))
    if edge:
        d["legal_lists"] = np.full((B, A), -1, np.int32)
        for i, l in enumerate(legal):
            d["legal_lists"][i, :len(l)] = l
    return d


FALLBACK_CASES = ("gmz_a64_b3_s64", "gmz_a64_noise_b5_s40", "gmz_perm_b4_s33_a9", "gmz_m7_rag_b4_s33_a9")


def check_edge_case(name, d):
    """the property each edge case is there for, and every output finite (children values at legal actions)"""
    lists = d["legal_lists"]
    legal = np.zeros(lists.shape, bool)
    for i, row in enumerate(lists):
        legal[i, row[row >= 0]] = True
    assert np.array_equal(legal, d["legal_mask"].astype(bool)), name
    assert np.all(np.isfinite(d["out_values"])) and np.all(np.isfinite(d["out_policies"])), name
    assert np.all(np.isfinite(d["out_children_values"][legal])), name
    assert np.all(np.isneginf(d["out_children_values"][~legal])) and np.all(d["out_policies"][~legal] == 0), name
    if name in FALLBACK_CASES:
        assert d["fallbacks"][0] > 0, f"{name} must reach the legal[0] fallback"
    if name.startswith("gmz_perm"):
        assert any(np.any(np.diff(row[row >= 0]) < 0) for row in lists), f"{name}: no non-ascending list"
    if name == "gmz_a1_deep_b3_s64":
        assert d["req_len"].max() == 64, f"{name}: the deepest walk is {d['req_len'].max()}"
    if name == "gmz_sharp_b4_s30_a6":
        # (the improved policy is a softmax over prior + completed Q, a spread of a dozen at the most, so a zero
        # prior never shows as a zero there: look at the root priors themselves, CNode::expand's float32 softmax)
        lg = np.where(legal, d["root_logits"], -np.inf).astype(np.float32)
        e = np.exp(lg - lg.max(axis=1, keepdims=True), dtype=np.float32)
        assert np.any((e / e.sum(axis=1, keepdims=True, dtype=np.float32))[legal] == 0), f"{name}: no zero prior"
        assert np.ptp(d["resp_logits"], axis=-1).max() > 110, f"{name}: no zero prior below the root"


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
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        if os.path.exists(path):  # the first ten transcripts never change: same draws, same arrays
            old = np.load(path)
            assert sorted(old.files) == sorted(d), c["name"]
            for k in old.files:
                assert old[k].dtype == d[k].dtype and old[k].shape == d[k].shape, (c["name"], k)
                assert old[k].tobytes() == d[k].tobytes(), (c["name"], k)
        np.savez_compressed(path, **d)
        print(f"{c['name']}: mean search_len {d['req_len'].mean():.2f} fallbacks {d['fallbacks'][0]}")
    for c in EDGE_CASES:
        d = gen_case(c, gmz_tree, edge=True)
        check_edge_case(c["name"], d)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 223 * 1024, (c["name"], os.path.getsize(path))
        print(f"{c['name']}: max search_len {d['req_len'].max()} fallbacks {d['fallbacks'][0]} "
              f"{os.path.getsize(path)} bytes")
    tabs = {"gumbel": np.array(gmz_tree.pgenerate_gumbel(10.0, 0.0, 64), np.float32),
            "ms": np.array(TABLE_MS, np.int64)}
    for m, S in TABLE_MS:
        # the row cselect_root_child reads: table[min(m, S)] (cnode.cpp:727-729)
        tabs[f"row_{m}_{S}"] = np.array(gmz_tree.pget_table_of_considered_visits(m, S)[min(m, S)], np.int32)
    np.savez_compressed(os.path.join(OUT_DIR, "gmz_tables.npz"), **tabs)
    print("gmz_tables.npz written")
    # every row m in [0, 66] x S in {1..64, 100, 200}: one concatenated array and an (m, S, offset) index
    rows, index, off = [], [], 0
    for m in range(67):
        for S in list(range(1, 65)) + [100, 200]:
            row = np.array(gmz_tree.pget_table_of_considered_visits(m, S)[min(m, S)], np.int64)
            assert row.shape == (S,) and row.min() >= 0 and row.max() < 2 ** 15
            rows.append(row.astype(np.int16))
            index.append((m, S, off))
            off += S
    path = os.path.join(OUT_DIR, "gmz_visits_full.npz")
    np.savez_compressed(path, rows=np.concatenate(rows), index=np.array(index, np.int32))
    print(f"gmz_visits_full.npz written: {len(index)} rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
