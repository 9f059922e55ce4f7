"""GPU: the resident search kernel's register walk (selection mode 5, lzm_search_res.h descend_a2r).

Every case is the fused search's record — each simulation's x, action and search_len — and the
final distributions, values and trajectories, bit-equal to OracleTree fed the recorded network
outputs (tests/test_gpu_fused.py's fused_search / check_tree_exact), over the regimes that reach
the walk's different endings: the leaf tie that needs no mean-q, the node with one visited child
(settle at the last level and, with sharpened heads, in mid-walk), ties between visited children
(settle, then the resumed walk), the root's one- and two-child rules, Philox draws, the largest
search the register walk serves and the first it does not, modes 4 and 5 against each other, and
the NaN guard of the leaf-tie shortcut.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.oracle import OracleTree  # noqa: E402
from tests import test_gpu_fused as tf  # noqa: E402
from tests.helpers import DISC, NOISE_W, PB_C_BASE, PB_C_INIT, VDM  # noqa: E402
from tests.test_gpu_fused import check_tree_exact, fused_search  # noqa: E402

A, H = 2, 128


def fresh_fraction(rec):
    """Fraction of simulations whose leaf's parent latent appears for the first time for its root
    (a node with no visited child: the walk ends in a leaf tie)."""
    x = rec["x"]  # [S, B]
    S, B = x.shape
    fresh = 0
    for i in range(B):
        seen = set()
        for k in range(S):
            if int(x[k, i]) not in seen:
                fresh += 1
                seen.add(int(x[k, i]))
    return fresh / float(S * B)


def assert_both_endings(rec):
    f = fresh_fraction(rec)
    print(f"fresh fraction {f:.3f}")
    assert f >= 1.0 / 3.0, f"only {f:.3f} of the simulations end at a fresh node"
    assert 1.0 - f >= 0.25, f"only {1.0 - f:.3f} of the simulations end at a visited node"


def midwalk_settles(rec):
    """Simulations whose path crosses, above its last level, a node with exactly one expanded child
    (the walk scores it with the mean-q and continues). The node of latent l + 1 is simulation l's
    leaf, a child of latent x[l]."""
    x = rec["x"]
    S, B = x.shape
    n = 0
    for i in range(B):
        parent = {0: -1}
        kids = {}
        for k in range(S):
            p = int(x[k, i])
            q = parent[p]
            hit = False
            while q >= 0:  # p's strict ancestors, up to the root (latent 0)
                hit = hit or kids.get(q, 0) == 1
                q = parent[q]
            n += int(hit)
            parent[k + 1] = p
            kids[p] = kids.get(p, 0) + 1
    return n


def oracle_mismatch(r, B, S, fast=False, legal=None, A=A):
    """None when the search r equals the oracle fed r's recorded network outputs, else what differs."""
    rec = r["rec"]
    ot = OracleTree(B, A, S, fast_rng=fast)
    ot.set_delta(VDM)
    if legal is not None:
        la = np.full((B, A), -1, np.int32)
        for i, l in enumerate(legal):
            la[i, :len(l)] = l
        ot.set_legal(la, np.array([len(l) for l in legal], np.int32))
    ot.prepare(NOISE_W, r["noises"], np.zeros(B, np.float32), r["logits0"], r["to_play"])
    for k in range(S):
        x, y, a, vtp, slen = ot.traverse(PB_C_BASE, PB_C_INIT, DISC, int(rec["seeds"][k]), r["to_play"])
        for name, got, want in (("x", rec["x"][k], x), ("action", rec["action"][k], a), ("search_len", rec["search_len"][k], slen)):
            if not np.array_equal(got, want):
                return f"{name} differs at sim {k}"
        ot.backprop(k + 1, DISC, rec["decoded"][k][:, 0], rec["decoded"][k][:, 1], rec["policy_logits"][k], vtp)
    if not np.array_equal(r["dist"], ot.distributions()):  # (both by legal position, -1 padded)
        return "distributions differ"
    if not np.array_equal(r["values"], ot.values(), equal_nan=True):
        return "values differ"
    if not np.array_equal(r["traj"], ot.trajectories(S + 2)):
        return "trajectories differ"
    return None


def last_linear(seq):
    return [m for m in seq.modules() if isinstance(m, torch.nn.Linear)][-1]


def heads(model):
    return (last_linear(model.prediction_network.fc_value_head), last_linear(model.dynamics_network.fc_reward_head),
            last_linear(model.prediction_network.fc_policy_head))


def patch_model(monkeypatch, edit):
    make = tf.make_model

    def patched(*a, **k):
        m = make(*a, **k)
        with torch.no_grad():
            edit(m)
        return m
    monkeypatch.setattr(tf, "make_model", patched)


# B, S, A, H, zero_heads, players, fast
RAND = [(8, 12, A, H, False, 1, False), (8, 50, A, H, False, 1, False), (1, 10, A, H, False, 1, False),
        (8, 25, A, H, False, 2, False), (8, 50, A, H, False, 1, True)]


@pytest.mark.parametrize("case", RAND, ids=tf._case_id)
def test_default_mode_random_heads(case):
    r = check_tree_exact(case)
    assert_both_endings(r["rec"])


def test_default_mode_zero_heads_settle_then_resume():
    r = check_tree_exact((8, 25, A, H, True, 1, False))
    assert r["diag"][2] > 0, "no tie between visited children was resolved through depth speculation"


def test_ragged_root_legal_sets(monkeypatch):
    from lightzero_amd.mcts_ctree import MuZeroMCTSCtree
    B, S = 6, 25
    legal = [[0], [1], [0, 1]] * 2
    roots = MuZeroMCTSCtree.roots
    monkeypatch.setattr(MuZeroMCTSCtree, "roots", classmethod(lambda cls, n, _l: roots(n, legal)))
    r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A)
    assert r["diag"][0] == 0 and r["diag"][3] == 0
    assert oracle_mismatch(r, B, S, legal=legal) is None
    d = r["dist"]
    assert (d[0] >= 0).sum() == 1 and (d[1] >= 0).sum() == 1 and (d[2] >= 0).sum() == 2


def test_sharpened_heads_settle_in_mid_walk(monkeypatch):
    def sharpen(m):
        for lin in heads(m):
            lin.weight.mul_(30.0)
            lin.bias.mul_(30.0)
    patch_model(monkeypatch, sharpen)
    r = check_tree_exact((8, 50, A, H, False, 1, False))
    n = midwalk_settles(r["rec"])
    print(f"simulations crossing a one-visited-child node above their last level: {n}")
    assert n >= 1, "no walk crossed a node with one visited child and continued"


@pytest.mark.parametrize("S", [62, 63])
def test_register_walk_boundary(S):
    r = check_tree_exact((2, S, A, H, False, 1, False))
    assert_both_endings(r["rec"])


@pytest.mark.parametrize("zero", [False, True], ids=["rand", "zero"])
def test_modes_4_and_5_agree(zero, monkeypatch):
    case = (8, 25 if zero else 50, A, H, zero, 1, False)
    out = {}
    for mode in ("4", "5"):
        monkeypatch.setenv("LZM_RES_SELECT", mode)
        out[mode] = check_tree_exact(case)
    for f in ("x", "action", "search_len"):
        assert np.array_equal(out["4"]["rec"][f], out["5"]["rec"][f]), f
    for f in ("dist", "values", "traj"):
        assert np.array_equal(out["4"][f], out["5"][f]), f
    if not zero:
        assert_both_endings(out["5"]["rec"])


def test_nan_guard(monkeypatch):
    """One NaN in the reward head's last bias makes every decoded reward NaN, so total_q is NaN wherever
    a child is visited: the leaf-tie shortcut must stand down (with a NaN vu the reference picks
    child 1 and consumes no draw). Modes 4 and 5 give the same search; where mode 4 equals the
    oracle on this input, so does mode 5. (On MI355X mode 4 does not: its record leaves the oracle's
    at simulation 1, "x differs at sim 1" — the kernel's NaN handling outside the walk, as before
    the register walk — so there the test compares the two modes only.)"""
    def poison(m):
        heads(m)[1].bias[7] = float("nan")
    patch_model(monkeypatch, poison)
    B, S = 4, 12
    out = {}
    for mode in ("4", "5"):
        monkeypatch.setenv("LZM_RES_SELECT", mode)
        out[mode] = fused_search(B, S, A, H, False, 1, False, seed=B + S + A)
    assert np.isnan(out["4"]["rec"]["decoded"][:, :, 0]).any(), "the NaN did not reach the decoded rewards"
    for f in ("x", "action", "search_len"):
        assert np.array_equal(out["4"]["rec"][f], out["5"]["rec"][f]), f
    assert np.array_equal(out["4"]["dist"], out["5"]["dist"])
    assert np.array_equal(out["4"]["traj"], out["5"]["traj"])
    assert np.array_equal(out["4"]["values"], out["5"]["values"], equal_nan=True)
    m4 = oracle_mismatch(out["4"], B, S)
    print(f"mode 4 against the oracle on the NaN input: {m4 or 'equal'}")
    if m4 is None:
        assert oracle_mismatch(out["5"], B, S) is None
