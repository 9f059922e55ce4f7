"""Generate the golden request/response transcripts under tests/golden/ (SURVEY.md §8(c)).

Test infrastructure only. This script drives the REFERENCE ctree (LightZero
``lzero/mcts/ctree/ctree_muzero/mz_tree.pyx`` and ``ctree_efficientzero/ez_tree.pyx``),
built from the sources under /root/reference by ``oracle/build_ref.sh`` into
``oracle/_ref/`` with ``gettimeofday`` wrapped so that the per-call
``srand(tv_usec)`` (``common_lib/utils.cpp:25``) takes a chosen seed.

The driving loop restates ``MuZeroMCTSCtree.search`` (``lzero/mcts/tree_search/mcts_ctree.py:228-321``)
and ``EfficientZeroMCTSCtree.search`` (``mcts_ctree.py:696-827``) with the network replaced by a
scripted table of responses, so each transcript holds, per simulation:
  requests  (x = latent_state_index_in_search_path, y = latent_state_index_in_batch,
             last_action, virtual_to_play, search_len)
  responses (reward | value_prefix, value, policy logits, and EZ is_reset)
and at the end the root visit distributions, root values and best-action trajectories.

CASES are the 18 first transcripts, all at the reference's default constants; regenerating must leave every array
of theirs as it is (asserted before anything is written). EDGE_CASES (tests/golden/tree/) vary the constants, the
horizon, the float regime of the responses, the depth and the order of the root legal lists; each stores its own
constants in meta / consts and the ordered lists in ``legal_lists``, and asserts the property it is there for.

Run (in the build container, where /root/reference exists):
    bash oracle/build_ref.sh && python tests/golden/gen_golden.py
The committed .npz files are data (inputs + expected outputs); the GPU box never needs
/root/reference.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_DIR = os.path.join(REPO, "oracle", "_ref")
EDGE_DIR = os.path.join(HERE, "tree")  # a directory of its own: the tests' tests/golden/*.npz globs keep their meaning

PB_C_BASE = 19652
PB_C_INIT = 1.25
DISCOUNT = 0.997
VALUE_DELTA_MAX = 0.01
NOISE_WEIGHT = 0.25
ALPHA = 0.3
LSTM_HORIZON = 5


def traverse_seed(seed, k):
    """Per-traverse srand seed, SURVEY.md §8(d): usec_k = (1000003*seed + k) mod 1e6."""
    return (1000003 * seed + k) % 1000000


def make_case(name, tree, B, S, A, net, players, seed, noise=True, ragged=False, pb_c_base=PB_C_BASE,
              pb_c_init=PB_C_INIT, discount=DISCOUNT, value_delta_max=VALUE_DELTA_MAX, noise_weight=NOISE_WEIGHT,
              horizon=LSTM_HORIZON, alpha=ALPHA, logits_fill=None, values_fill=None, legal="mask"):
    """logits_fill / values_fill: a fill kind (fill()) applied to the logits / to reward and value after they are
    drawn; legal: "mask" (ascending lists from the mask), "permuted" (each root's list shuffled) or the lists"""
    return dict(name=name, tree=tree, B=B, S=S, A=A, net=net, players=players, seed=seed,
                noise=noise, ragged=ragged, pb_c_base=pb_c_base, pb_c_init=pb_c_init, discount=discount,
                value_delta_max=value_delta_max, noise_weight=noise_weight, horizon=horizon, alpha=alpha,
                logits_fill=logits_fill, values_fill=values_fill, legal=legal)


CASES = [
    make_case("mz_zero_1p_b8_s25_a2", "mz", 8, 25, 2, "zero", 1, 0),
    make_case("mz_rand_1p_b8_s25_a2", "mz", 8, 25, 2, "rand", 1, 1),
    make_case("mz_zero_1p_b64_s25_a2", "mz", 64, 25, 2, "zero", 1, 2),
    make_case("mz_rand_1p_b64_s25_a2", "mz", 64, 25, 2, "rand", 1, 0),
    make_case("mz_zero_1p_b256_s50_a2", "mz", 256, 50, 2, "zero", 1, 1),
    make_case("mz_rand_1p_b256_s50_a2", "mz", 256, 50, 2, "rand", 1, 2),
    make_case("mz_quant_1p_b64_s50_a4", "mz", 64, 50, 4, "quant", 1, 0),
    make_case("mz_rand_1p_b32_s50_a6", "mz", 32, 50, 6, "rand", 1, 1),
    make_case("mz_zero_1p_b32_s50_a6", "mz", 32, 50, 6, "zero", 1, 2),
    make_case("mz_rand_1p_b32_s30_a4_nonoise", "mz", 32, 30, 4, "rand", 1, 0, noise=False),
    make_case("mz_rand_2p_b16_s50_a9", "mz", 16, 50, 9, "rand", 2, 1, ragged=True),
    make_case("mz_zero_2p_b16_s50_a9", "mz", 16, 50, 9, "zero", 2, 2, ragged=True),
    make_case("mz_quant_2p_b64_s25_a2", "mz", 64, 25, 2, "quant", 2, 0),
    make_case("mz_rand_1p_b48_s40_a5_ragged", "mz", 48, 40, 5, "rand", 1, 2, ragged=True),
    make_case("ez_rand_1p_b32_s50_a6", "ez", 32, 50, 6, "rand", 1, 0),
    make_case("ez_zero_1p_b32_s50_a6", "ez", 32, 50, 6, "zero", 1, 1),
    make_case("ez_quant_1p_b64_s50_a4", "ez", 64, 50, 4, "quant", 1, 2),
    make_case("ez_rand_2p_b16_s50_a9", "ez", 16, 50, 9, "rand", 2, 0, ragged=True),
]


def a64_perm_lists():
    """ragged, shuffled lists over 64 actions (the full set among them) and one root whose only action is 63"""
    rng = np.random.default_rng(6463)
    lists = [rng.permutation(64).tolist()]
    for k in (40, 7):
        lists.append(rng.permutation(64)[:k].tolist())
    return lists + [[63]]


def both(idea, shape, net, seed, ez_kw=None, **kw):
    """the MuZero and the EfficientZero form of one edge case (ez_kw: what only the latter sets)"""
    B, S, A = shape
    tail = f"{idea}_b{B}_s{S}_a{A}"
    ez = dict(kw, **(ez_kw or {}))
    return [make_case("mz_" + tail, "mz", B, S, A, net, kw.pop("players", 1), seed, **kw),
            make_case("ez_" + tail, "ez", B, S, A, net, ez.pop("players", 1), seed + 1, **ez)]


# The setting, float, depth and list-order edges, written to tests/golden/tree/. Each also stores its ordered legal
# lists; check_edge_case asserts what each is there for.
EDGE_CASES = (
    # paths longer than 64 levels: a second 64-lane round of the backup, trajectories past 64 entries
    both("a1_deep", (3, 70, 1), "rand", 100)
    # (two actions: below a node visited once the prior term is times sqrt(0), so the first step from every fresh node is
    # a coin flip whatever the logits, and a line gains about two levels in three simulations: 80 do not reach 64)
    + [make_case("mz_a2_deep_b3_s110_a2", "mz", 3, 110, 2, "rand", 1, 102, logits_fill="x30", values_fill="const"),
       make_case("ez_a2_deep_b3_s140_a2", "ez", 3, 140, 2, "rand", 2, 103, logits_fill="x30", values_fill="denorm")]
    # the 64-bit tie mask at its ends: a 64-way tie, a choice in lane 63
    + both("a64_alltie", (3, 70, 64), "zero", 104, noise=False)
    + both("a64_perm", (4, 30, 64), "rand", 106, legal=a64_perm_lists(), players=2, ez_kw=dict(players=1))
    # root legal lists that are not ascending
    + both("perm_small", (8, 20, 5), "quant", 108, ragged=True, legal="permuted")
    # the pb_c table
    + [make_case("mz_pbc1_b4_s60_a6", "mz", 4, 60, 6, "rand", 1, 110, pb_c_base=1),
       make_case("mz_pbc100_init2.5_b4_s60_a6", "mz", 4, 60, 6, "rand", 1, 111, pb_c_base=100, pb_c_init=2.5)]
    + both("pbc5_init0", (4, 60, 6), "rand", 112, pb_c_base=5, pb_c_init=0.0)
    # the discount at its ends
    + both("disc0", (4, 30, 4), "rand", 114, discount=0.0)
    + both("disc1", (4, 30, 4), "rand", 116, discount=1.0)
    + both("disc05", (4, 30, 4), "rand", 118, discount=0.5)
    # mm_normalize: the delta < value_delta_max branch never taken / taken for the whole search
    + both("vdm0", (4, 30, 4), "rand", 120, value_delta_max=0.0)
    + both("vdm_big", (4, 30, 4), "rand", 122, value_delta_max=10.0, values_fill="small")
    # the noise weight at its ends, over noise rows that hold exact zeros
    + [make_case("mz_nw0_b8_s30_a6", "mz", 8, 30, 6, "rand", 1, 124, noise_weight=0.0, alpha=0.03),
       make_case("mz_nw1_b8_s30_a6", "mz", 8, 30, 6, "rand", 1, 125, noise_weight=1.0, alpha=0.03)]
    # EfficientZero resets: every node, every second level, never
    + [make_case("ez_hor1_b4_s30_a4", "ez", 4, 30, 4, "rand", 1, 126, horizon=1),
       make_case("ez_hor2_b6_s30_a5", "ez", 6, 30, 5, "rand", 2, 127, horizon=2, ragged=True),
       make_case("ez_hor_never_b4_s30_a4", "ez", 4, 30, 4, "rand", 1, 128, horizon=35)]
    # float edges
    + both("spread", (4, 30, 6), "rand", 130, logits_fill="x60")
    + both("big", (4, 30, 6), "rand", 132, values_fill="big")
    + both("huge", (4, 30, 6), "rand", 134, values_fill="huge")
    + both("const", (4, 30, 6), "rand", 136, values_fill="const")
    + both("neg", (4, 30, 6), "rand", 138, values_fill="neg")
    + both("denorm", (4, 30, 6), "rand", 140, values_fill="denorm")
    # arithmetic that one ulp decides: the order of compute_mean_q's sum. Discount 0, so every q is a reward; rewards
    # of 1e5 + x, so a sum of three depends on its order in the last bits while the min-max span stays a few units
    + [make_case("mz_sumorder_b8_s60_a6", "mz", 8, 60, 6, "rand", 1, 144, discount=0.0, values_fill="offset")]
    # wave and workgroup remainders
    + [make_case("mz_b70_s12_a3", "mz", 70, 12, 3, "rand", 1, 142),
       make_case("mz_b257_s12_a3", "mz", 257, 12, 3, "rand", 1, 143)]
)


def fill(kind, x):
    """a drawn float32 array scaled or replaced by the fill kind (None: as drawn)"""
    f = np.float32
    if kind is None:
        return x
    if kind == "x30":     # one line dominates
        return (x * f(30.0)).astype(np.float32)
    if kind == "x60":     # logit spreads past 104: expf underflows, priors become exact zeros
        return (x * f(60.0)).astype(np.float32)
    if kind == "offset":  # 1e5 + x: neighbours 2^-7 apart, sums of three past 2^18: the order of a sum shows in its bits
        return (f(1e5) + x).astype(np.float32)
    if kind == "small":
        return (x * f(1e-2)).astype(np.float32)
    if kind == "big":     # magnitudes 1e4 .. 9e5: sums near the +-1e6 min-max sentinels
        return (np.where(x < 0, f(-1), f(1)) * np.clip(np.abs(x) * f(4e5), f(1e4), f(9e5))).astype(np.float32)
    if kind == "huge":    # past the sentinels
        return (np.where(x < 0, f(-3e6), f(3e6))).astype(np.float32)
    if kind == "const":   # every value equal and non-zero
        return np.full(x.shape, 0.37, np.float32)
    if kind == "neg":
        return (-(np.abs(x) + f(0.1))).astype(np.float32)
    if kind == "denorm":
        return (x * f(1e-40)).astype(np.float32)
    raise ValueError(kind)


def scripted(rng, net, shape):
    """Scripted network output tables (float32)."""
    if net == "zero":
        return np.zeros(shape, np.float32)
    if net == "rand":
        return rng.normal(0.0, 1.0, size=shape).astype(np.float32)
    if net == "quant":  # exact ties among visited children exercise the 1e-6 tie rule
        return rng.integers(-1, 2, size=shape).astype(np.float32)
    raise ValueError(net)


def gen_case(c, mods, lib, edge=False, sort_lists=False):
    """sort_lists: the same inputs with every root's list ascending (the comparison run of the permuted cases)"""
    tree = mods[c["tree"]]
    B, S, A = c["B"], c["S"], c["A"]
    rng = np.random.default_rng(1000 + c["seed"] * 7 + B + S * 13 + A)
    # legal actions (ascending order, as the collector builds them from action_mask)
    legal_mask = np.ones((B, A), np.int8)
    if c["ragged"]:
        for i in range(B):
            k = int(rng.integers(1, A + 1))
            sel = np.sort(rng.choice(A, size=k, replace=False))
            legal_mask[i] = 0
            legal_mask[i, sel] = 1
    legal = [[a for a in range(A) if legal_mask[i, a]] for i in range(B)]
    if c["legal"] == "permuted":  # (a stream of its own: every other draw is the sorted run's)
        prng = np.random.default_rng(977 + c["seed"])
        legal = [prng.permutation(l).tolist() for l in legal]
    elif c["legal"] != "mask":
        legal = [list(l) for l in c["legal"]]
        legal_mask[:] = 0
        for i, l in enumerate(legal):
            legal_mask[i, l] = 1
    if sort_lists:
        legal = [sorted(l) for l in legal]
    if c["players"] == 1:
        to_play = [-1] * B
    else:
        to_play = [int(v) for v in rng.integers(1, 3, size=B)]
    noises = np.zeros((B, A), np.float32)
    for i in range(B):
        n = len(legal[i])
        noises[i, :n] = rng.dirichlet([c["alpha"]] * n).astype(np.float32)
    lfill, vfill = c["logits_fill"], c["values_fill"]
    root_logits = fill(lfill, scripted(rng, c["net"], (B, A)))
    root_reward = np.zeros(B, np.float32) if c["tree"] == "mz" else fill(vfill, scripted(rng, c["net"], (B,)) * 0.5)
    if c["tree"] == "mz" and vfill == "offset":  # (a zero root reward would put 0 into the min-max stats: a span of
        root_reward = fill(vfill, root_reward)   # 1e5, under which the children's differences vanish)

    resp_reward = fill(vfill, scripted(rng, c["net"], (S, B)) * np.float32(0.5))
    resp_value = fill(vfill, scripted(rng, c["net"], (S, B)))
    resp_logits = fill(lfill, scripted(rng, c["net"], (S, B, A)))
    seeds = np.array([traverse_seed(c["seed"], k) for k in range(S)], np.int64)
    pb_c_base, pb_c_init, discount, horizon = c["pb_c_base"], c["pb_c_init"], c["discount"], c["horizon"]

    roots = tree.Roots(B, legal)
    if c["noise"]:
        roots.prepare(c["noise_weight"], [noises[i, :len(legal[i])].tolist() for i in range(B)],
                      root_reward.tolist(), root_logits.tolist(), list(to_play))
    else:
        roots.prepare_no_noise(root_reward.tolist(), root_logits.tolist(), list(to_play))
    mms = tree.MinMaxStatsList(B)
    mms.set_delta(c["value_delta_max"])

    req = {k: np.zeros((S, B), np.int32) for k in ("x", "y", "a", "vtp", "len")}
    resp_reset = np.zeros((S, B), np.int32)
    for k in range(S):
        lib.oracle_set_usec(int(seeds[k]))
        res = tree.ResultsWrapper(num=B)
        x, y, a, vtp = tree.batch_traverse(roots, pb_c_base, pb_c_init, discount, mms, res, list(to_play))
        slen = res.get_search_len()
        req["x"][k], req["y"][k], req["a"][k] = x, y, a
        req["vtp"][k], req["len"][k] = vtp, slen
        if c["tree"] == "mz":
            tree.batch_backpropagate(k + 1, discount, resp_reward[k].tolist(), resp_value[k].tolist(),
                                     resp_logits[k].tolist(), mms, res, vtp)
        else:
            is_reset = (np.array(slen) % horizon == 0).astype(np.int32)
            resp_reset[k] = is_reset
            tree.batch_backpropagate(k + 1, discount, resp_reward[k].tolist(), resp_value[k].tolist(),
                                     resp_logits[k].tolist(), mms, res, is_reset.tolist(), vtp)
    dist = roots.get_distributions()
    out_dist = np.full((B, A), -1, np.int32)
    for i, d in enumerate(dist):
        out_dist[i, :len(d)] = d
    out_values = np.array(roots.get_values(), np.float32)
    trajs = roots.get_trajectories()
    tmax = max(1, max(len(t) for t in trajs))
    out_traj = np.full((B, tmax), -1, np.int32)
    for i, t in enumerate(trajs):
        out_traj[i, :len(t)] = t
    meta = np.array([B, S, A, c["players"], int(c["noise"]), 1 if c["tree"] == "ez" else 0, horizon], np.int64)
    consts = np.array([pb_c_base, pb_c_init, discount, c["value_delta_max"], c["noise_weight"]], np.float64)
    d = dict(meta=meta, consts=consts, legal_mask=legal_mask, to_play=np.array(to_play, np.int32),
             noises=noises, root_logits=root_logits, root_reward=root_reward, seeds=seeds,
             req_x=req["x"], req_y=req["y"], req_a=req["a"], req_vtp=req["vtp"], req_len=req["len"],
             resp_reward=resp_reward, resp_value=resp_value, resp_logits=resp_logits,
             resp_is_reset=resp_reset, out_dist=out_dist, out_values=out_values, out_traj=out_traj)
    if edge:  # the lists in the order the reference was given them: a mask cannot say it
        d["legal_lists"] = np.full((B, A), -1, np.int32)
        for i, l in enumerate(legal):
            d["legal_lists"][i, :len(l)] = l
    return d


def f32_softmax_has_zero(logits, legal):
    """CNode::expand's float32 softmax over the legal entries of some row yields an exact 0"""
    lg = np.where(legal, logits, -np.inf).astype(np.float32)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True), dtype=np.float32)
    return bool(np.any((e / e.sum(axis=-1, keepdims=True, dtype=np.float32))[legal] == 0))


def check_edge_case(c, d, regen):
    """the property each edge case is there for, and every output finite. regen(**overrides) runs the same case
    again with some of its settings changed (nothing of it is written)."""
    name = c["name"]
    idea = name.split("_", 1)[1].rsplit("_b", 1)[0]
    lists, legal = d["legal_lists"], d["legal_mask"].astype(bool)
    from_lists = np.zeros(lists.shape, bool)
    for i, row in enumerate(lists):
        assert len(set(row[row >= 0].tolist())) == (row >= 0).sum(), name
        from_lists[i, row[row >= 0]] = True
    assert np.array_equal(from_lists, legal), name
    assert np.all(np.isfinite(d["out_values"])), f"{name}: the reference's root values are not finite"
    assert np.all(np.where(d["out_dist"] >= 0, d["out_dist"], 0).sum(axis=1) == c["S"]), name
    want = [c["pb_c_base"], c["pb_c_init"], c["discount"], c["value_delta_max"], c["noise_weight"]]
    assert d["consts"].tolist() == [float(v) for v in want] and d["meta"][6] == c["horizon"], name
    vals = np.concatenate([d["resp_reward"].ravel(), d["resp_value"].ravel()])
    ascending = all(np.all(np.diff(row[row >= 0]) > 0) for row in lists)
    if idea in ("a1_deep", "a2_deep"):
        assert d["req_len"].max() > 64, f"{name}: the deepest walk is {d['req_len'].max()}"
    if idea == "a1_deep":
        assert d["out_traj"].shape[1] > 64, f"{name}: the longest trajectory is {d['out_traj'].shape[1]}"
    if idea == "a64_alltie":
        # (64 distinct first choices out of 64 equal scores: the first 64 walks of every root are ties among all the
        # children not yet visited, the first of them a 64-way tie; tests/test_oracle.py looks at its tie list)
        assert np.all((d["out_dist"] > 0).sum(axis=1) == 64), f"{name}: a root distribution holds a zero"
        assert np.any(d["req_a"] == 63), f"{name}: action 63 is never requested"
    if idea == "a64_perm":
        assert not ascending, f"{name}: every list is ascending"
        # the one-action root: every walk passes through 63 (all S visits), the first one requests it
        one = [i for i, row in enumerate(lists) if row[row >= 0].tolist() == [63]]
        assert one, name
        for i in one:
            assert d["out_dist"][i, 0] == c["S"] and d["req_a"][0, i] == 63 and d["out_traj"][i, 0] == 63, name
    if idea == "perm_small":
        assert not ascending, f"{name}: every list is ascending"
        other = regen(sort_lists=True)
        assert np.array_equal(other["legal_mask"], d["legal_mask"]) and np.array_equal(other["noises"], d["noises"])
        assert np.any(other["req_a"][0] != d["req_a"][0]), f"{name}: the list order changes no first action"
    if idea.startswith("pbc"):
        other = regen(pb_c_base=PB_C_BASE, pb_c_init=PB_C_INIT)
        assert np.array_equal(other["resp_value"], d["resp_value"])
        assert not np.array_equal(other["out_dist"], d["out_dist"]), f"{name}: same visits as at the defaults"
    if idea in ("nw0", "nw1"):
        cnt = legal.sum(axis=1)
        assert any(np.any(d["noises"][i, :cnt[i]] == 0) for i in range(len(cnt))), f"{name}: no zero noise entry"
    if idea.startswith("hor"):
        want = dict(hor1="ones", hor2="mixed", hor_never="zeros")[idea]
        r = d["resp_is_reset"]
        assert dict(ones=np.all(r == 1), zeros=np.all(r == 0), mixed=np.any(r == 1) and np.any(r == 0))[want], name
        assert np.all(d["root_reward"] != 0), f"{name}: a zero root value prefix"
    if idea == "spread":
        assert np.ptp(d["resp_logits"], axis=-1).max() > 104, f"{name}: no spread past 104"
        assert f32_softmax_has_zero(d["resp_logits"], np.ones(d["resp_logits"].shape, bool)), f"{name}: no zero prior"
    if idea == "big":
        assert np.abs(vals).min() >= 1e4 and np.abs(vals).max() <= 9e5 and np.abs(d["resp_value"]).max() > 6e5, name
    if idea == "huge":
        assert np.all(np.abs(d["resp_value"]) == np.float32(3e6)), name
    if idea == "const":
        assert np.all(vals == vals[0]) and vals[0] != 0, name
        zero = regen(net="zero", values_fill=None)
        assert d["req_len"].max() >= zero["req_len"].max(), (name, d["req_len"].max(), zero["req_len"].max())
    if idea == "neg":
        assert np.all(vals < 0), name
    if idea == "sumorder":
        f = np.float32
        tri = d["resp_reward"].ravel()[:d["resp_reward"].size // 3 * 3].reshape(-1, 3)
        fw, bw = f(f(tri[:, 0] + tri[:, 1]) + tri[:, 2]), f(f(tri[:, 2] + tri[:, 1]) + tri[:, 0])
        assert np.mean(fw != bw) > 0.1, f"{name}: {np.mean(fw != bw):.3f} of the reward triples sum differently reversed"
        assert np.all(d["root_reward"] == f(1e5)), name
    if idea == "denorm":
        assert np.all(np.abs(vals) < np.finfo(np.float32).tiny) and np.any(vals != 0), name


def glibc_rand_vectors(lib_c):
    """Known-answer vectors of glibc srand/rand (the RNG cbatch_traverse uses, cnode.cpp:592)."""
    seeds = [0, 1, 12345, 999999, 2147483646]
    out = np.zeros((len(seeds), 2000), np.int64)
    for r, s in enumerate(seeds):
        lib_c.srand(ctypes.c_uint(s))
        for j in range(2000):
            out[r, j] = lib_c.rand()
    return np.array(seeds, np.int64), out


def main():
    if not os.path.isdir(REF_DIR):
        sys.exit("oracle/_ref missing: run oracle/build_ref.sh first")
    sys.path.insert(0, REF_DIR)
    import mz_tree  # noqa: E402  (reference build, test infrastructure)
    import ez_tree  # noqa: E402
    lib = ctypes.CDLL(mz_tree.__file__)
    lib.oracle_set_usec.argtypes = [ctypes.c_long]
    lib_ez = ctypes.CDLL(ez_tree.__file__)
    lib_ez.oracle_set_usec.argtypes = [ctypes.c_long]
    mods = {"mz": mz_tree, "ez": ez_tree}
    libs = {"mz": lib, "ez": lib_ez}
    # nothing is written before every case has been generated and checked
    done = []
    for c in CASES:
        d = gen_case(c, mods, libs[c["tree"]])
        path = os.path.join(HERE, c["name"] + ".npz")
        if os.path.exists(path):  # the 18 first transcripts never change: same draws, same arrays
            with np.load(path) as old:
                assert sorted(old.files) == sorted(d), c["name"]
                for k in old.files:
                    assert old[k].dtype == d[k].dtype and old[k].shape == d[k].shape, (c["name"], k)
                    assert old[k].tobytes() == d[k].tobytes(), (c["name"], k)
        done.append((c, d, path))
    assert len(set(c["name"] for c in EDGE_CASES)) == len(EDGE_CASES)
    for c in EDGE_CASES:
        d = gen_case(c, mods, libs[c["tree"]], edge=True)

        def regen(sort_lists=False, c=c, **over):
            return gen_case(dict(c, **over), mods, libs[c["tree"]], edge=True, sort_lists=sort_lists)
        check_edge_case(c, d, regen)
        done.append((c, d, os.path.join(EDGE_DIR, c["name"] + ".npz")))
    os.makedirs(EDGE_DIR, exist_ok=True)
    for c, d, path in done:
        np.savez_compressed(path, **d)
        lens = d["req_len"]
        print(f"{c['name']}: mean search_len {lens.mean():.2f} max {lens.max()} -> {os.path.basename(path)} "
              f"{os.path.getsize(path)} bytes")
    largest = max(os.path.getsize(p) for _, _, p in done[:len(CASES)])
    for _, _, path in done[len(CASES):]:
        assert os.path.getsize(path) <= largest, (path, os.path.getsize(path), largest)
    libc = ctypes.CDLL("libc.so.6")
    seeds, draws = glibc_rand_vectors(libc)
    np.savez_compressed(os.path.join(HERE, "glibc_rand.npz"), seeds=seeds, draws=draws)
    print("glibc_rand.npz written")


if __name__ == "__main__":
    main()
