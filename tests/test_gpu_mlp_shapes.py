"""GPU: the one-launch MLP search kernels (lzm_search_mlp) across the shapes they accept.

Every search case is tests/test_gpu_fused.py's fused_search — the search's record and its final distributions,
values and trajectories bit-equal to OracleTree fed the recorded network outputs — and asserts the launch plan
it ran under (DeviceTree.search_mlp_plan, the function lzm_search_mlp itself decides with):

  resident   search_res_kernel (lzm_search_res.h) at H 128, F 32, V 601, residual dynamics and A != 2: selection
             mode 1 (the wave walk descend_terms, the look-back resume without depth speculation, the policy
             block and one-hot rows for A > 2, expand_wave with more than two children). The handle's reserved
             capacity sizes the kernel's LDS plan, so these cases run on a handle reserved for exactly S
             simulations (Roots' pooled handles hold 64: resident at that capacity for A <= 3 only) and take S
             from the plan query;
  streaming  search_mlp_kernel (lzm_search_mlp.h) without the residual dynamics connection and at the widths that
             reach layer_split / swz_source / tpos beyond H in {64, 128}: padded columns (H 48), the wide-layer
             path (H 512, 1024), the [latent; one-hot] row padding (A 16, 17), the decode switch (V 511, 513,
             1023), several roots per workgroup;
  refused    shapes the kernels' argument checks refuse run the generic per-simulation path, not an error.

The network outputs of both kernels are compared with float64 (tests/mlp_numerics.py).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_gpu_fused as tf  # noqa: E402
from tests.mlp_numerics import check_search_network  # noqa: E402
from tests.test_gpu_fused import fused_search  # noqa: E402
from tests.test_gpu_walk_regs import oracle_mismatch  # noqa: E402

DEV = torch.device("cuda", 0)
H = 128
RES_DIMS = dict(hidden=128, head_hidden=32, support=601, res=True)
RESIDENT = dict(roots_per_wg=1, kernel="resident", mode=1, tree_in_lds=True)


@functools.lru_cache(None)
def largest_resident_S(A):
    """the longest search the plan query reports resident for A actions, on a handle reserved for exactly it"""
    from lightzero_amd.tree import DeviceTree

    def resident(S):
        t = DeviceTree(2, A, S, device=DEV)
        try:
            return t.search_mlp_plan(RES_DIMS, S)["kernel"] == "resident"
        finally:
            t.close()
    lo, hi = 0, 256  # resident(lo) (or lo == 0: none), not resident(hi)
    assert not resident(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if resident(mid):
            lo = mid
        else:
            hi = mid
    print(f"largest resident S at A = {A}: {lo}")
    return lo


def exact(r, B, S, A, fast=False, legal=None):
    assert r["diag"][0] == 0 and r["diag"][3] == 0, "look-back spin timeout or depth speculation mismatch"
    assert oracle_mismatch(r, B, S, fast=fast, legal=legal, A=A) is None
    return r


def resident(B, want, A, zero=False, players=1, fast=False, legal=None, seed=None):
    S = min(want, largest_resident_S(A))
    assert S >= 1, f"no resident search at A = {A}"
    r = fused_search(B, S, A, H, zero, players, fast, seed=B + S + A if seed is None else seed, tree_sims=S)
    assert r["plan"] == RESIDENT, r["plan"]
    return exact(r, B, S, A, fast, legal), S


# ---- B. the resident kernel at A != 2 (selection mode 1) ------------------------------------------------------
# (16 children and 5 simulations: a walk seldom comes back to one child twice. Seed 97 is one at which the
# search does, at three of the 64 roots by the oracle with the module's CPU outputs; the default seed has none)
@pytest.mark.parametrize("A,want,B,seed", [(3, 50, 16, None), (4, 30, 16, None), (6, 30, 16, None), (9, 17, 16, None),
                                           (16, 5, 64, 97), (1, 20, 16, None)])
def test_resident_random_heads(A, want, B, seed):
    r, S = resident(B, want, A, seed=seed)
    rec = r["rec"]
    if S >= A:
        assert set(np.unique(rec["action"])) == set(range(A)), "an action never occurs"
    print(f"A {A} S {S}: deepest search_len {rec['search_len'].max()}")
    assert rec["search_len"].max() >= 3, "no walk descends past the root's children"


@pytest.mark.parametrize("A,want", [(3, 25), (4, 20)])
def test_resident_zero_heads_ties_resume_after_look_back(A, want):
    r, _ = resident(16, want, A, zero=True)
    assert r["diag"][1] > 0, "no status-2 tie was resumed after the look-back"


@pytest.mark.parametrize("A,want", [(9, 17), (3, 30)])
def test_resident_two_players(A, want):
    resident(16, want, A, players=2)


@pytest.mark.parametrize("A,want,zero", [(4, 30, False), (3, 25, True)])
def test_resident_philox(A, want, zero):
    resident(16, want, A, zero=zero, fast=True)


def test_resident_ragged_root_legal_sets(monkeypatch):
    from lightzero_amd.mcts_ctree import MuZeroMCTSCtree
    A, B = 4, 8
    legal = [[2], [0, 3], [1, 2, 3], [0, 1, 2, 3]] * 2
    roots = MuZeroMCTSCtree.roots
    monkeypatch.setattr(MuZeroMCTSCtree, "roots", classmethod(lambda cls, n, _l: roots(n, legal)))
    r, _ = resident(B, 25, A, legal=legal)
    for i, l in enumerate(legal):
        assert (r["dist"][i] >= 0).sum() == len(l) and (r["dist"][i, len(l):] == -1).all()


@pytest.mark.parametrize("B", [1, 37, 256])
def test_resident_batch_edges(B):
    resident(B, 20, 3)


@pytest.mark.parametrize("A", [3, 9])
def test_resident_plan_boundary(A):
    """the longest search the plan reports resident, and the first it does not: both tree-exact"""
    B, S = 4, largest_resident_S(A)
    r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A, tree_sims=S)
    assert r["plan"] == RESIDENT, r["plan"]
    exact(r, B, S, A)
    r = fused_search(B, S + 1, A, H, False, 1, False, seed=B + S + A, tree_sims=S + 1)
    assert r["plan"]["kernel"] == "streaming", r["plan"]
    exact(r, B, S + 1, A)


def test_handle_reserved_for_a_longer_search_streams_a_short_one():
    """a handle's capacity, not the search's length, sizes the resident plan: the query says so and the
    result is exact either way"""
    A, B, S = 9, 4, 10
    assert S < largest_resident_S(A)
    r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A, tree_sims=largest_resident_S(A) + 40)
    assert r["plan"]["kernel"] == "streaming", r["plan"]
    exact(r, B, S, A)
    r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A, tree_sims=S)
    assert r["plan"] == RESIDENT, r["plan"]
    exact(r, B, S, A)


def test_mode_1_at_two_actions_equals_mode_5(monkeypatch):
    B, S, A = 8, 50, 2  # test_gpu_fused.CASES[0], shrunk
    out = {}
    for mode in (1, 5):
        if mode == 1:
            monkeypatch.setenv("LZM_RES_SELECT", "1")
        else:
            monkeypatch.delenv("LZM_RES_SELECT")
        r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A, tree_sims=S)
        assert r["plan"] == dict(RESIDENT, mode=mode), r["plan"]
        out[mode] = exact(r, B, S, A)
    for f in ("x", "action", "search_len", "vtp", "decoded", "policy_logits", "seeds"):
        assert np.array_equal(out[1]["rec"][f], out[5]["rec"][f]), f
    for f in ("dist", "values", "traj"):
        assert np.array_equal(out[1][f], out[5][f]), f


@pytest.mark.parametrize("A,mode", [(2, 5), (3, 1)])
def test_unknown_select_mode_is_ignored(A, mode, monkeypatch):
    """LZM_RES_SELECT takes 1, 4 and 5: a removed mode (3) and garbage (7) leave the default for A in place"""
    B, S = 8, 12
    for value in ("3", "7"):
        monkeypatch.setenv("LZM_RES_SELECT", value)
        r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A, tree_sims=S)
        assert r["plan"] == dict(RESIDENT, mode=mode), (value, r["plan"])
        exact(r, B, S, A)


@pytest.mark.parametrize("A,want", [(4, 30), (9, 17)])
def test_resident_network_matches_float64(A, want):
    B = 16
    r, S = resident(B, want, A)
    check_search_network(f"search resident A{A}", r, S, B, 300)


# ---- C. the streaming kernel across its domain ----------------------------------------------------------------
def streaming(monkeypatch, B, S, A, Hd, zero=False, players=1, fast=False, scale=300, roots=1, **model_kw):
    if Hd == 128:
        monkeypatch.setenv("LZM_FUSED_RES", "0")
    if roots != 1:
        monkeypatch.setenv("LZM_ROOTS_PER_WG", str(roots))
    r = fused_search(B, S, A, Hd, zero, players, fast, seed=B + S + A, support_scale=scale, **model_kw)
    assert r["plan"]["kernel"] == "streaming" and r["plan"]["roots_per_wg"] == roots, r["plan"]
    exact(r, B, S, A, fast)
    F = model_kw.get("head_hidden", 32)
    name = "search streaming H{} F{} V{} A{} res{} R{}{}".format(Hd, F, 2 * scale + 1, A, int(model_kw.get("res", True)),
                                                                  roots, " zero" if zero else "")
    check_search_network(name, r, S, B, scale)
    return r


@pytest.mark.parametrize("zero", [False, True], ids=["rand", "zero"])
@pytest.mark.parametrize("Hd,A", [(128, 2), (64, 3), (256, 4)])
def test_streaming_without_residual_dynamics(Hd, A, zero, monkeypatch):
    streaming(monkeypatch, 8, 12, A, Hd, zero=zero, res=False)


def test_streaming_without_residual_dynamics_philox(monkeypatch):
    streaming(monkeypatch, 8, 12, 3, 64, fast=True, res=False)


def test_streaming_without_residual_dynamics_two_players(monkeypatch):
    streaming(monkeypatch, 8, 12, 4, 256, players=2, res=False)


WIDTHS = [
    # H, F, scale, A, B, S
    (256, 32, 300, 4, 8, 12),    # the model's default latent width
    (48, 16, 10, 3, 8, 12),      # columns padded to a power of two
    (16, 16, 10, 9, 8, 12),      # the narrowest layers; [latent; one-hot] rows 25 -> 32
    (512, 64, 50, 6, 8, 12),     # hidden layers as wide as the workgroup
    (1024, 32, 300, 2, 2, 5),    # two rounds of the wide-layer path
    (128, 48, 300, 2, 8, 12),    # a head width that is no power of two
    (64, 32, 300, 16, 8, 12),    # one-hot rows end on a K chunk
    (64, 32, 300, 17, 8, 12),    # ... and one row past it
    (64, 32, 255, 2, 8, 12),     # V = 511: the last support decoded through LDS
    (64, 32, 256, 2, 8, 12),     # V = 513: the first decoded from registers in two rounds
    (64, 32, 511, 1, 8, 12),     # V + A = 1024: the widest head output
]


@pytest.mark.parametrize("Hd,F,scale,A,B,S", WIDTHS)
def test_streaming_widths(Hd, F, scale, A, B, S, monkeypatch):
    streaming(monkeypatch, B, S, A, Hd, scale=scale, head_hidden=F)


@pytest.mark.parametrize("roots", [2, 8])
@pytest.mark.parametrize("Hd,F,scale,A", [(256, 32, 300, 4), (48, 16, 10, 3)])
def test_streaming_roots_per_workgroup(Hd, F, scale, A, roots, monkeypatch):
    streaming(monkeypatch, 11, 12, A, Hd, scale=scale, head_hidden=F, roots=roots)


# ---- D. shapes the kernels refuse take the generic path ---------------------------------------------------------
REFUSED = {
    "latent_100": dict(A=3, Hd=100, scale=10, group=4),     # lzm_mlp_prepare: H % 16
    "head_hidden_24": dict(A=3, Hd=64, scale=10, head_hidden=24),
    "support_1201": dict(A=2, Hd=64, scale=600),            # V + A > 1024
    "actions_above_latent": dict(A=17, Hd=16, scale=10),    # A > H
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_shapes_search_on_the_generic_path(name):
    kw = dict(REFUSED[name])
    A, Hd, scale = kw.pop("A"), kw.pop("Hd"), kw.pop("scale")
    B, S = 4, 8
    r = fused_search(B, S, A, Hd, False, 1, False, seed=B + S + A, support_scale=scale, fused=False, **kw)
    assert r["path"] == "generic"
    assert oracle_mismatch(r, B, S, A=A) is None


def test_pack_refuses_what_the_kernels_refuse():
    """pack_muzero_mlp asks the library (lzm_search_mlp_supported, tests/test_abi.py) and raises NotPackable"""
    from lightzero_amd.fused import NotPackable, pack_muzero_mlp
    with pytest.raises(NotPackable):
        pack_muzero_mlp(tf.make_model(3, 64, False, support_scale=10, head_hidden=24), DEV)
    pack_muzero_mlp(tf.make_model(3, 64, False, support_scale=10, head_hidden=16), DEV)
