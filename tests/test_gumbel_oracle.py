"""The host restatement of the Gumbel MuZero tree (tests/gumbel_oracle.py) replays every reference
transcript tests/golden/gumbel/gmz_*.npz bit for bit: the requests of every simulation and all five outputs."""
import glob
import os

import numpy as np
import pytest

import gumbel_oracle as go

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(go.GOLDEN, "gmz_*.npz"))
               if not p.endswith(("gmz_tables.npz", "gmz_visits_full.npz")))
EDGE_CASES = ["gmz_a64_b3_s64", "gmz_a64_noise_b5_s40", "gmz_perm_b4_s33_a9", "gmz_perm_noise_b3_s20_a64",
              "gmz_a1_deep_b3_s64", "gmz_a2_deep_b3_s64", "gmz_sharp_b4_s30_a6", "gmz_big_b4_s30_a6",
              "gmz_huge_b4_s30_a6", "gmz_const_b4_s30_a6", "gmz_tiny_b4_s30_a6", "gmz_near_b4_s30_a6",
              "gmz_denorm_b4_s30_a6", "gmz_quant_b6_s40_a5", "gmz_m2_b4_s24_a7", "gmz_m3_b4_s24_a7",
              "gmz_m5_b4_s64_a9", "gmz_m7_rag_b4_s33_a9", "gmz_m64_b3_s64_a64", "gmz_m0_b4_s10_a4",
              "gmz_m6_a64_b4_s64", "gmz_2p_rag_b5_s20_a5", "gmz_b70_s12_a3", "gmz_disc0_b4_s20_a4"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_cases_present():
    assert len(CASES) >= 34
    for name in ["gmz_b8_s25_a2", "gmz_b4_s16_a6", "gmz_b3_s50_a18"] + EDGE_CASES:
        assert name in CASES


def test_fallback_case_reaches_fallback():
    assert int(np.load(os.path.join(go.GOLDEN, "gmz_b4_s16_a6.npz"))["fallbacks"][0]) > 0


def load(name):
    return np.load(os.path.join(go.GOLDEN, name + ".npz"))


@pytest.mark.parametrize("name", ["gmz_a64_b3_s64", "gmz_a64_noise_b5_s40", "gmz_perm_b4_s33_a9",
                                  "gmz_m7_rag_b4_s33_a9"])
def test_edge_fallback_cases_reach_fallback(name):
    assert int(load(name)["fallbacks"][0]) > 0


def test_edge_case_properties():
    """what each edge transcript is there for, read from the stored arrays"""
    for name in EDGE_CASES:
        g = load(name)
        lists = go.legal_lists(g)
        legal = g["legal_mask"].astype(bool)
        for i, l in enumerate(lists):  # the ordered lists and the mask name the same sets
            assert len(set(l)) == len(l) and sorted(l) == np.flatnonzero(legal[i]).tolist(), (name, i)
        assert np.all(np.isfinite(g["out_values"])) and np.all(np.isfinite(g["out_policies"])), name
        assert np.all(np.isfinite(g["out_children_values"][legal])), name
        assert np.all(np.isneginf(g["out_children_values"][~legal])), name
    a64 = go.legal_lists(load("gmz_a64_b3_s64"))
    assert 0 not in a64[1] and a64[2] == [63] and int(load("gmz_a64_b3_s64")["meta"][2]) == 64
    for name in ("gmz_perm_b4_s33_a9", "gmz_perm_noise_b3_s20_a64"):
        assert any(l != sorted(l) for l in go.legal_lists(load(name))), name
    deep = load("gmz_a1_deep_b3_s64")
    assert int(deep["req_len"].max()) == 64 == int(deep["meta"][1])
    assert float(load("gmz_disc0_b4_s20_a4")["consts"][0]) == 0.0
    assert [int(load(n)["meta"][3]) for n in ("gmz_m0_b4_s10_a4", "gmz_m3_b4_s24_a7", "gmz_m5_b4_s64_a9",
                                              "gmz_m7_rag_b4_s33_a9", "gmz_m64_b3_s64_a64")] == [0, 3, 5, 7, 64]
    assert int(load("gmz_b70_s12_a3")["meta"][0]) == 70


def test_sharp_case_has_exact_zero_priors():
    """logit spreads past 104: expf underflows and CNode::expand's priors hold exact zeros. The improved policy
    cannot show them (it is a softmax over prior + completed Q, a spread of a dozen at the most, so every legal
    entry of out_policies is positive); the restatement, pinned to this transcript by test_replay, can."""
    g = load("gmz_sharp_b4_s30_a6")
    assert np.ptp(g["root_logits"], axis=1).max() > 110
    t, _ = go.replay(g)
    zeros, stack = 0, list(t.roots)
    while stack:
        n = stack.pop()
        zeros += sum(1 for c in n.children.values() if c.prior == 0)
        stack.extend(c for c in n.children.values() if c.children)
    assert sum(1 for r in t.roots for c in r.children.values() if c.prior == 0) > 0 and zeros > 10
    legal = g["legal_mask"].astype(bool)
    assert np.all(g["out_policies"][legal] > 0)


@pytest.mark.parametrize("name", CASES)
def test_replay(name):
    g = np.load(os.path.join(go.GOLDEN, name + ".npz"))
    t, req = go.replay(g)
    for k, gk in (("x", "req_x"), ("y", "req_y"), ("a", "req_a"), ("vtp", "req_vtp"), ("len", "req_len")):
        assert np.array_equal(req[k], g[gk]), k
    A = int(g["meta"][2])
    disc = g["consts"][0]
    assert np.array_equal(go.pad(t.distributions(), A), g["out_dist"])
    assert np.array_equal(go.pad(t.trajectories(), g["out_traj"].shape[1])[:, :g["out_traj"].shape[1]], g["out_traj"])
    assert np.array_equal(bits(t.values()), bits(g["out_values"]))
    assert np.array_equal(bits(t.children_values(disc)), bits(g["out_children_values"]))
    assert np.array_equal(bits(t.policies(disc)), bits(g["out_policies"]))


def test_considered_visits_rows():
    tabs = np.load(os.path.join(go.GOLDEN, "gmz_tables.npz"))
    for m, S in tabs["ms"]:
        assert go.considered_visits(int(m), int(S)) == tabs[f"row_{m}_{S}"].tolist(), (m, S)


def test_considered_visits_every_row():
    full = go.visits_full()
    assert len(full) == 67 * 66 == 4422
    assert sorted(set(m for m, _, _ in full)) == list(range(67))
    assert sorted(set(S for _, S, _ in full)) == list(range(1, 65)) + [100, 200]
    for m, S, row in full:
        assert len(row) == S and go.considered_visits(m, S) == row, (m, S)
