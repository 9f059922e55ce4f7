"""CPU: the oracle (oracle/lz_oracle.c, a restatement of the reference ctree) pinned against the
golden transcripts recorded from the reference build (tests/golden/gen_golden.py)."""
import glob
import os

import numpy as np
import pytest

from oracle.oracle import (OracleTree, glibc_rand_stream, lib, load_transcript, philox4x32_10,
                           replay_transcript)
from tests.helpers import random_transcript, run_scripted_search_oracle, run_transcript

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRANSCRIPTS = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if not p.endswith("glibc_rand.npz") and not os.path.basename(p).startswith(("az_", "reuse_", "ptree_")))


def test_golden_files_present():
    assert len(TRANSCRIPTS) >= 18


@pytest.mark.parametrize("path", TRANSCRIPTS, ids=lambda p: os.path.basename(p)[:-4])
def test_oracle_reproduces_reference_transcript(path):
    bad = replay_transcript(load_transcript(path))
    assert not bad, bad


# ---------------------------------------------------------------------- the setting, float, depth and list-order edges
TREE_DIR = os.path.join(GOLDEN, "tree")
EDGE_TRANSCRIPTS = sorted(glob.glob(os.path.join(TREE_DIR, "*.npz")))


def edge_case_names():
    """the names tests/golden/gen_golden.py lists (it imports nothing of the reference before main())"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(GOLDEN, "gen_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return sorted(c["name"] for c in mod.EDGE_CASES)


def test_every_edge_transcript_is_present():
    """a missing fixture fails here: the parametrised replays below would only run fewer cases"""
    names = edge_case_names()
    assert len(names) == 44 and len(set(names)) == len(names)
    assert [os.path.basename(p)[:-4] for p in EDGE_TRANSCRIPTS] == names


def idea_of(path):
    return os.path.basename(path)[:-4].split("_", 1)[1].rsplit("_b", 1)[0]


@pytest.mark.parametrize("path", EDGE_TRANSCRIPTS, ids=lambda p: os.path.basename(p)[:-4])
def test_oracle_reproduces_edge_transcript(path):
    tr = load_transcript(path)
    keep = {}
    bad = replay_transcript(tr, keep=keep)
    assert not bad, bad
    # what the reference cannot show (it has no getter): read from the restatement after its bit-exact replay
    t, idea = keep["tree"], idea_of(path)
    B, S, A = (int(v) for v in tr["meta"][:3])
    vdm = np.float32(tr["consts"][3])
    mm = t.minmax()
    span = mm[:, 0] - mm[:, 1]
    if idea == "vdm_big":    # mm_normalize's delta < value_delta_max branch for the whole search
        assert vdm == 10 and np.all(span > 0) and np.all(span < vdm), span
    if idea == "vdm0":       # never
        assert vdm == 0 and np.all(span > 0), span
    if idea in ("big", "huge"):
        assert np.all(np.isfinite(mm)), mm
    if idea == "nw1":        # noise weight 1: the prior is the noise entry, exact zeros included
        cnt = tr["legal_mask"].sum(axis=1)
        pri = t.root_priors()
        assert all(np.array_equal(pri[i, :cnt[i]], tr["noises"][i, :cnt[i]]) for i in range(B))
        assert any(np.any(pri[i, :cnt[i]] == 0) for i in range(B))
    if idea == "nw0":        # noise weight 0: every prior is CNode::expand's softmax, no zero among these logits
        pri = t.root_priors()
        assert np.all(pri[:, :A] > 0) and np.any(tr["noises"] == 0)
    if idea == "a1_deep":
        assert tr["out_traj"].shape[1] > 64 and tr["req_len"].max() > 64
    if "legal_lists" in tr and idea in ("a64_perm", "perm_small"):
        assert any(np.any(np.diff(row[row >= 0]) < 0) for row in tr["legal_lists"])


@pytest.mark.parametrize("tree", ["mz", "ez"])
def test_a64_alltie_first_walk_is_a_64_way_tie(tree):
    """the scores cselect_child sees at every root before the first simulation: 64 equal ones, so the tie list
    holds all 64 actions; again once every child has been visited once (simulation 64)"""
    from tests.helpers import tie_list
    from oracle.oracle import transcript_legal
    path, = [p for p in EDGE_TRANSCRIPTS if os.path.basename(p).startswith(tree + "_a64_alltie")]
    tr = load_transcript(path)
    B, S, A, players, noise, ez, horizon = (int(v) for v in tr["meta"])
    base, init, disc, vdm, nw = (float(v) for v in tr["consts"])
    t = OracleTree(B, A, S, ez=bool(ez))
    t.set_legal(*transcript_legal(tr))
    t.set_delta(np.float32(vdm))
    t.prepare(np.float32(nw), None, tr["root_reward"], tr["root_logits"], tr["to_play"])
    for k in range(S):
        if k in (0, 64):
            for i in range(B):
                sc = t.path_scores(i, np.zeros(0, np.int32), int(base), init, disc, players)
                assert sc.shape[0] == 1 and tie_list(sc[0]) == list(range(64)), (k, i)
        x, y, a, vtp, slen = t.traverse(base, np.float32(init), np.float32(disc), int(tr["seeds"][k]), tr["to_play"])
        assert np.array_equal(a, tr["req_a"][k])
        t.backprop(k + 1, np.float32(disc), tr["resp_reward"][k], tr["resp_value"][k], tr["resp_logits"][k], vtp,
                   tr["resp_is_reset"][k] if ez else None)
    assert np.any(tr["req_a"] == 63)


def test_glibc_rand_restatement_matches_libc_vectors():
    g = np.load(os.path.join(GOLDEN, "glibc_rand.npz"))
    for seed, draws in zip(g["seeds"], g["draws"]):
        assert np.array_equal(glibc_rand_stream(int(seed), draws.shape[0]), draws), seed


def test_philox_known_answers():
    # Random123 kat_vectors for philox4x32_10
    assert philox4x32_10([0, 0, 0, 0], [0, 0]).tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2).tolist() == [0x408f276d, 0x41c83b0e, 0xa20bc7c6,
                                                                            0x6d5451fd]
    assert philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]).tolist() == [
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("fast", [False, True])
def test_oracle_visit_counts_conserved(fast):
    B, S, A = 32, 30, 4
    out = run_transcript(random_transcript(B, S, A, seed=3), OracleTree, fast_rng=fast)
    # every simulation adds exactly one visit below the root
    assert (out["dist"].sum(axis=1) == S).all()
    assert (out["len"] >= 1).all()


def test_oracle_fast_mode_independent_of_batch_composition():
    # Philox draws depend on (seed, root, level) only: the first 8 roots of a 32-root batch
    # search exactly like an 8-root batch (not true of the serial glibc stream).
    tr32 = random_transcript(32, 20, 3, seed=5, net="quant")
    tr8 = {k: (v[:8] if k in ("legal_mask", "to_play", "noises", "root_logits", "root_reward") else v)
           for k, v in tr32.items()}
    tr8["meta"] = tr32["meta"].copy()
    tr8["meta"][0] = 8
    for k in ("resp_reward", "resp_value", "resp_is_reset"):
        tr8[k] = tr32[k][:, :8]
    tr8["resp_logits"] = tr32["resp_logits"][:, :8]
    a = run_transcript(tr32, OracleTree, fast_rng=True)
    b = run_transcript(tr8, OracleTree, fast_rng=True)
    assert np.array_equal(a["dist"][:8], b["dist"])


def test_host_search_loop_is_deterministic():
    a = run_scripted_search_oracle(16, 20, 3, seed=1)
    b = run_scripted_search_oracle(16, 20, 3, seed=1)
    assert np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["values"], b["values"])
    assert (a["dist"].sum(axis=1) == 20).all()


def test_cpu_baseline_driver_runs():
    secs = lib().lzo_bench_tree_only(64, 2, 10, 2, 1, 1)
    assert secs > 0


def test_path_scores_diagnostic_agrees_with_traverse():
    """oracle.path_scores (the divergence attribution's tool): along every root's traverse path the
    action taken is in the tie list of the scores the diagnostic recomputes at that level"""
    from tests.helpers import tie_list
    tr = random_transcript(24, 16, 3, seed=9, net="rand")
    B, S, A = 24, 16, 3
    ot = OracleTree(B, A, S)
    ot.set_delta(np.float32(0.01))
    ot.prepare(np.float32(0.25), tr["noises"], tr["root_reward"], tr["root_logits"], np.full(B, -1, np.int32))
    levels = 0
    for k in range(S):
        x, y, a, vtp, slen = ot.traverse(19652, np.float32(1.25), np.float32(0.997), 1000 + k, np.full(B, -1, np.int32))
        for i in range(B):
            acts = ot.path_actions(i)
            assert len(acts) == slen[i] and acts[-1] == a[i]
            sc = ot.path_scores(i, acts)
            assert sc.shape[0] == len(acts)  # the leaf below the last action is not expanded yet
            for lvl, act in enumerate(acts):
                assert act in tie_list(sc[lvl]), (k, i, lvl)
                levels += 1
        ot.backprop(k + 1, np.float32(0.997), tr["resp_reward"][k], tr["resp_value"][k], tr["resp_logits"][k], vtp)
    assert levels > B * S
