"""GPU: the one-launch conv searches (lzm_search_conv: conv MuZero; lzm_search_conv_ez: conv EfficientZero)
across the shapes their host entry points accept, not only the two Atari configs of tests/test_gpu_conv.py.

Every case builds a MuZeroModel / EfficientZeroModel with explicit arguments (observation 4 x 64 x 64, downsample,
hidden width 32 per head, BatchNorm with non-trivial statistics), feeds the search random non-negative root
latents, random root logits and (EZ) a random root LSTM state, and runs it twice with the same model and seed:
one launch (cfg.fused_search, the default) and the generic per-simulation path. It asserts

  * the path each side took ("fused-conv" / "fused" against "generic": a silent fallback would make the
    comparison vacuous) and the launch plan the library reports for the shape (DeviceTree.search_conv_plan:
    workgroups, LSTM tiles, pb_c table, which head-output branch the kernel takes);
  * array equality of visit counts, root values, trajectories and of every simulation's request (latent index,
    action, search_len), decoded {reward, value}, policy logits and (EZ) is_reset;
  * in glibc mode the oracle replay, bit for bit (tree, legal sets, players, horizon, discount);
  * on the cases marked `torch`: the decoded values against the torch module (test_gpu_conv.torch_replay);
  * that the walk is not trivial: some root's search_len reaches min(3, S).

The seeds were chosen per case on the GPU (the first of 1, 2, ... whose search meets the last condition and,
for lstm_horizon_len = 3, has a reset and a non-reset leaf at depth >= 2).

The branches the cases reach: trunk block loops of 0 / 2 / 3 iterations and partial 1x1 output tiles (reward
planes 2 / 6 / 14, head planes 2 .. 16); dead K-parts of the head hidden layers (K = 128 .. 896) and
off_policy != Khd / 2; the MuZero output loop at N2 <= 768, = 768, = 769 and three rounds; the EfficientZero
single-round / multi-round output forms on either side of 256 columns; scalar heads; unequal reward / value
supports; 1 .. 18 actions, ragged legal sets, two players, discount 1 and 0.9; lstm_horizon_len 1, 3 and
S + 1, and at A = 2 the settings away from the defaults (pb_c_base / pb_c_init (5, 0) and (100, 2.5),
value_delta_max 0 and 10, discount 1 and 0.5, horizon 1 and S + 5); LSTM widths 128 / 256 / 1024 with 1 .. 129 roots (row blocks holding one live row, more roots than
tiles, 2 T > B); S = 1, 2, the pb_c table switch and the LDS boundary; Philox mode and the all-tie search.
Shapes the kernels refuse (supports past 1024, more than 8 residual blocks, a hidden width other than 32, a tree
past the LDS plan, a grid that cannot be co-resident) take another path without raising and equal the oracle.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_conv import DEV, conv_model, oracle_replay, run_search, torch_replay  # noqa: E402


def make_model(kind, seed, zero=False, A=None, blocks=1, r_ch=16, hv=16, hp=16, Vr=None, Vv=None, H=512, cat=True,
               fc_value=(32,)):
    """a conv MuZeroModel / EfficientZeroModel with explicit arguments (defaults: the Atari configs)"""
    from lightzero_amd.model_conv import EfficientZeroModel, MuZeroModel
    ez = kind == "ez"
    A = (6 if ez else 4) if A is None else A
    V = 101 if ez else 601
    kw = dict(observation_shape=(4, 64, 64), action_space_size=A, num_res_blocks=blocks, num_channels=64,
              reward_head_channels=r_ch, value_head_channels=hv, policy_head_channels=hp, fc_reward_layers=(32,),
              fc_value_layers=tuple(fc_value), fc_policy_layers=(32,), reward_support_size=Vr or V,
              value_support_size=Vv or V, self_supervised_learning_loss=False, categorical_distribution=cat,
              downsample=True, norm_type='BN')
    if ez:
        kw["lstm_hidden_size"] = H
    cls = EfficientZeroModel if ez else MuZeroModel
    return conv_model(kind, seed, zero_heads=zero, factory=lambda **k: cls(**kw, **k))


def ragged_legal(B, A, seed):
    """per-root random non-empty legal subsets; root 0 has one action, root 1 all of them"""
    rng = np.random.default_rng(seed)
    legal = [sorted(rng.choice(A, size=int(rng.integers(1, A + 1)), replace=False).tolist()) for _ in range(B)]
    legal[0] = [int(rng.integers(0, A))]
    legal[1] = list(range(A))
    return legal


def c(id, kind, B, S, seed, model=None, search=None, torch=False, plan=None, rng="glibc", zero=False):
    return pytest.param(dict(kind=kind, B=B, S=S, seed=seed, model=model or {}, search=search or {}, torch=torch,
                             plan=plan or {}, rng=rng, zero=zero), id=id)


def tiles(B, H):
    return -(-B // 64) * (H // 16)


# EfficientZero plan facts of the Atari head (support 101, 6 actions): both outputs one column per thread
EZ1 = dict(out_one_round=True, reward_one_round=True)
PBT = 64 + 8  # rows of the pb_c table: a fresh tree reserves 64 simulations

CASES = [
    # ---- residual blocks
    c("mz-blocks0", "mz", 9, 10, 1, dict(blocks=0)),
    c("mz-blocks2", "mz", 7, 10, 1, dict(blocks=2), torch=True),
    c("mz-blocks3", "mz", 5, 8, 1, dict(blocks=3)),
    c("ez-blocks0", "ez", 9, 10, 1, dict(blocks=0), plan=EZ1),
    c("ez-blocks2", "ez", 7, 10, 1, dict(blocks=2), torch=True, plan=EZ1),
    c("ez-blocks3", "ez", 5, 8, 1, dict(blocks=3), plan=EZ1),
    # ---- reward planes (K = 128, 384, 896; EZ: the LSTM K)
    c("mz-rch2", "mz", 11, 10, 1, dict(r_ch=2)),
    c("mz-rch6", "mz", 13, 10, 1, dict(r_ch=6), torch=True),
    c("mz-rch14", "mz", 6, 12, 1, dict(r_ch=14)),
    c("ez-rch2", "ez", 11, 10, 1, dict(r_ch=2), plan=EZ1),
    c("ez-rch6", "ez", 13, 10, 1, dict(r_ch=6), torch=True, plan=EZ1),
    c("ez-rch14", "ez", 6, 12, 1, dict(r_ch=14), plan=EZ1),
    # ---- head planes (value, policy): unequal K, dead K-parts, off_policy != Khd / 2
    c("mz-head2x2", "mz", 8, 10, 1, dict(hv=2, hp=2)),
    c("mz-head2x16", "mz", 10, 10, 1, dict(hv=2, hp=16)),
    c("mz-head16x2", "mz", 12, 10, 1, dict(hv=16, hp=2)),
    c("mz-head6x10", "mz", 14, 10, 1, dict(hv=6, hp=10), torch=True),
    c("ez-head2x2", "ez", 8, 10, 2, dict(hv=2, hp=2), plan=EZ1),
    c("ez-head2x16", "ez", 10, 10, 1, dict(hv=2, hp=16), plan=EZ1),
    c("ez-head16x2", "ez", 12, 10, 1, dict(hv=16, hp=2), plan=EZ1),
    c("ez-head6x10", "ez", 14, 10, 1, dict(hv=6, hp=10), torch=True, plan=EZ1),
    # ---- supports, MuZero: the output loop's rounds of 768 columns
    c("mz-sup601x21", "mz", 9, 10, 1, dict(Vr=601, Vv=21), torch=True, plan=dict(out_rounds=1)),
    c("mz-sup21x601", "mz", 9, 10, 1, dict(Vr=21, Vv=601), plan=dict(out_rounds=1)),
    c("mz-sup255x255", "mz", 9, 10, 1, dict(Vr=255, Vv=255), plan=dict(out_rounds=1)),
    c("mz-n2-768", "mz", 9, 10, 1, dict(Vr=383, Vv=381, A=4), plan=dict(out_rounds=1)),
    c("mz-n2-769", "mz", 9, 10, 1, dict(Vr=383, Vv=381, A=5), plan=dict(out_rounds=2)),
    c("mz-sup1023", "mz", 9, 10, 1, dict(Vr=1023, Vv=1023), plan=dict(out_rounds=3)),
    # ---- supports, EfficientZero: one column per thread up to 256 columns, rounds past them
    c("ez-sup601", "ez", 9, 10, 1, dict(Vr=601, Vv=601), torch=True,
      plan=dict(out_one_round=False, out_rounds=1, reward_one_round=False)),
    c("ez-sup257x101", "ez", 9, 10, 1, dict(Vr=257, Vv=101), plan=dict(out_one_round=True, reward_one_round=False)),
    c("ez-vp256", "ez", 9, 10, 1, dict(Vr=101, Vv=251, A=5), plan=dict(out_one_round=True, reward_one_round=True)),
    c("ez-vp257", "ez", 9, 10, 2, dict(Vr=101, Vv=251, A=6),
      plan=dict(out_one_round=False, out_rounds=1, reward_one_round=True)),
    c("ez-sup1023", "ez", 9, 10, 1, dict(Vr=1023, Vv=1023),
      plan=dict(out_one_round=False, out_rounds=2, reward_one_round=False)),
    # ---- scalar heads (categorical_distribution=False, supports 1): the decode's raw-value branch
    c("mz-scalar", "mz", 9, 10, 1, dict(cat=False), dict(categorical=False), torch=True, plan=dict(out_rounds=1)),
    c("ez-scalar", "ez", 9, 10, 1, dict(cat=False), dict(categorical=False), torch=True, plan=EZ1),
    # ---- actions
    c("mz-A1", "mz", 5, 8, 1, dict(A=1)),
    c("mz-A2", "mz", 7, 10, 1, dict(A=2)),
    c("mz-A3", "mz", 9, 10, 1, dict(A=3)),
    c("mz-A9", "mz", 11, 12, 1, dict(A=9)),
    c("mz-A18", "mz", 13, 16, 1, dict(A=18), torch=True),
    c("ez-A1", "ez", 5, 8, 1, dict(A=1), plan=EZ1),
    c("ez-A2", "ez", 7, 10, 1, dict(A=2), plan=EZ1),
    c("ez-A3", "ez", 9, 10, 1, dict(A=3), plan=EZ1),
    c("ez-A9", "ez", 11, 12, 4, dict(A=9), plan=EZ1),
    c("ez-A18", "ez", 13, 16, 2, dict(A=18), torch=True, plan=EZ1),
    c("mz-ragged", "mz", 17, 12, 1, dict(A=9), dict(legal="ragged")),
    c("ez-ragged", "ez", 17, 12, 1, dict(A=9), dict(legal="ragged"), plan=EZ1),
    # ---- two players
    c("mz-players", "mz", 16, 12, 1, {}, dict(to_play="two")),
    c("ez-players", "ez", 16, 12, 1, {}, dict(to_play="two"), plan=EZ1),
    # ---- discount
    c("mz-disc1", "mz", 10, 12, 1, {}, dict(discount=1.0)),
    c("ez-disc09", "ez", 10, 12, 1, {}, dict(discount=0.9), plan=EZ1),
    # ---- EfficientZero: lstm_horizon_len
    c("ez-horizon1", "ez", 9, 10, 1, {}, dict(horizon=1), plan=EZ1),
    c("ez-horizon3", "ez", 9, 12, 1, {}, dict(horizon=3), torch=True, plan=EZ1),
    c("ez-horizonS1", "ez", 9, 10, 1, {}, dict(horizon=11), plan=EZ1),
    # ---- EfficientZero: LSTM width and the tile grid (T = ceil(B / 64) H / 16 tiles, max(B, 2 T) workgroups)
    c("ez-H128", "ez", 21, 10, 1, dict(H=128), torch=True, plan=dict(lstm_tiles=8, workgroups=21)),
    c("ez-H256", "ez", 21, 10, 1, dict(H=256), plan=dict(lstm_tiles=16, workgroups=32)),
    c("ez-H1024", "ez", 21, 10, 1, dict(H=1024), plan=dict(lstm_tiles=64, workgroups=128)),
    c("ez-H128-B1", "ez", 1, 10, 1, dict(H=128), plan=dict(lstm_tiles=8, workgroups=16)),
    c("ez-H128-B63", "ez", 63, 8, 1, dict(H=128), plan=dict(lstm_tiles=8, workgroups=63)),
    c("ez-H128-B64", "ez", 64, 8, 1, dict(H=128), plan=dict(lstm_tiles=8, workgroups=64)),
    c("ez-H128-B65", "ez", 65, 8, 1, dict(H=128), plan=dict(lstm_tiles=16, workgroups=65)),
    c("ez-H128-B129", "ez", 129, 8, 1, dict(H=128), plan=dict(lstm_tiles=24, workgroups=129)),
    c("ez-H1024-B37", "ez", 37, 8, 1, dict(H=1024), plan=dict(lstm_tiles=64, workgroups=128)),
    # ---- S = 1, 2
    c("mz-S1", "mz", 9, 1, 1),
    c("mz-S2", "mz", 9, 2, 6),
    c("ez-S1", "ez", 9, 1, 1, plan=EZ1),
    c("ez-S2", "ez", 9, 2, 2, plan=EZ1),
    # ---- Philox mode (one launch against the generic path only) and zero-initialised heads (the all-tie search)
    c("mz-blocks2-philox", "mz", 7, 10, 1, dict(blocks=2), rng="philox"),
    c("mz-n2-769-philox", "mz", 9, 10, 1, dict(Vr=383, Vv=381, A=5), rng="philox", plan=dict(out_rounds=2)),
    c("ez-sup601-philox", "ez", 9, 10, 1, dict(Vr=601, Vv=601), rng="philox",
      plan=dict(out_one_round=False, out_rounds=1, reward_one_round=False)),
    c("ez-H128-B65-philox", "ez", 65, 8, 1, dict(H=128), rng="philox", plan=dict(lstm_tiles=16, workgroups=65)),
    c("mz-head6x10-zero", "mz", 14, 10, 1, dict(hv=6, hp=10), zero=True),
    c("ez-rch6-zero", "ez", 13, 10, 3, dict(r_ch=6), zero=True, plan=EZ1),
    # ---- settings away from the reference's defaults, at the A = 2 shape: the pb_c table (and the triangular table
    # built from it), mm_normalize's value_delta_max branch never / always taken, the discount, the horizon's ends
    c("mz-pbc5-init0", "mz", 7, 10, 1, dict(A=2), dict(pb_c_base=5, pb_c_init=0.0)),
    c("mz-pbc100-init2.5", "mz", 7, 10, 1, dict(A=2), dict(pb_c_base=100, pb_c_init=2.5)),
    c("mz-vdm0", "mz", 7, 10, 1, dict(A=2), dict(value_delta_max=0.0)),
    c("mz-vdm10", "mz", 7, 10, 1, dict(A=2), dict(value_delta_max=10.0)),
    c("mz-A2-disc1", "mz", 7, 10, 1, dict(A=2), dict(discount=1.0)),
    c("mz-A2-disc05", "mz", 7, 10, 1, dict(A=2), dict(discount=0.5)),
    c("ez-pbc5-init0", "ez", 7, 10, 1, dict(A=2), dict(pb_c_base=5, pb_c_init=0.0), plan=EZ1),
    c("ez-pbc100-init2.5", "ez", 7, 10, 1, dict(A=2), dict(pb_c_base=100, pb_c_init=2.5), plan=EZ1),
    c("ez-vdm0", "ez", 7, 10, 1, dict(A=2), dict(value_delta_max=0.0), plan=EZ1),
    c("ez-vdm10", "ez", 7, 10, 1, dict(A=2), dict(value_delta_max=10.0), plan=EZ1),
    c("ez-A2-disc1", "ez", 7, 10, 1, dict(A=2), dict(discount=1.0), plan=EZ1),
    c("ez-A2-disc05", "ez", 7, 10, 1, dict(A=2), dict(discount=0.5), plan=EZ1),
    c("ez-A2-horizon1", "ez", 7, 10, 1, dict(A=2), dict(horizon=1), plan=EZ1),
    c("ez-A2-horizonS5", "ez", 7, 10, 1, dict(A=2), dict(horizon=15), plan=EZ1),
]


def search_kwargs(case, model):
    kw = dict(case["search"])
    A, B = model.action_space_size, case["B"]
    if kw.get("legal") == "ragged":
        kw["legal"] = ragged_legal(B, A, case["seed"])
    if kw.get("to_play") == "two":
        kw["to_play"] = np.random.default_rng(case["seed"]).integers(1, 3, size=B).tolist()
    if kw.get("categorical", True):
        dyn, pred = model.dynamics_network, model.prediction_network
        Vr, Vv = dyn.fc_reward_head[-1].out_features, pred.fc_value[-1].out_features
        kw["scales"] = ((Vr - 1) // 2, (Vv - 1) // 2)
    else:
        kw["scales"] = (1, 1)
    return kw


def both_paths(case, seed=None):
    """the case's search by one launch and by the generic path: (fused result, generic result)"""
    seed = case["seed"] if seed is None else seed
    model = make_model(case["kind"], seed + 100, zero=case["zero"], **case["model"])
    kw = search_kwargs(case, model)
    return [run_search(case["kind"], case["B"], case["S"], seed, model=model, fused=f, rng=case["rng"], direct=True,
                       check=True, fresh_tree=True, **kw) for f in (True, False)]


def assert_same_search(kind, a, b):
    for key in ("dist", "values", "traj"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("x", "action", "search_len", "decoded", "policy_logits") + (("is_reset",) if kind == "ez" else ()):
        assert np.array_equal(a["rec"][key], b["rec"][key]), key


def assert_walk_not_trivial(case, res):
    rec, S = res["rec"], case["S"]
    assert rec["search_len"].max() >= min(3, S), int(rec["search_len"].max())
    if case["kind"] == "ez":
        deep = rec["search_len"] >= 2
        h = res["horizon"]
        assert np.array_equal(rec["is_reset"], (rec["search_len"] % h == 0).astype(np.int32))
        if h == 1:
            assert rec["is_reset"].all()
        elif h > S:
            assert not rec["is_reset"].any()
        elif h == 3:  # a reset and a non-reset leaf at depth >= 2, where % 3 and % 5 differ
            assert (deep & (rec["is_reset"] == 1)).any() and (deep & (rec["is_reset"] == 0)).any()


def expected_plan(case):
    """what the library's plan must report for the case: its own entries over the shape's defaults"""
    ez, B = case["kind"] == "ez", case["B"]
    exp = dict(supported=True, code=0)
    if ez:
        H = case["model"].get("H", 512)
        T = tiles(B, H)
        exp.update(lstm_tiles=T, workgroups=max(B, 2 * T), pinned=0)
    else:
        exp.update(lstm_tiles=0, workgroups=B, pbt_rows=0, out_one_round=False, reward_one_round=False, out_rounds=2)
    exp.update(case["plan"])
    return exp


@pytest.mark.parametrize("case", CASES)
def test_one_launch_equals_generic_equals_oracle(case):
    kind, B, S = case["kind"], case["B"], case["S"]
    a, b = both_paths(case)
    assert a["path"] == ("fused" if kind == "ez" else "fused-conv") and b["path"] == "generic", (a["path"], b["path"])
    plan, exp = a["plan"], expected_plan(case)
    assert {k: plan[k] for k in exp} == exp, plan
    assert 0 < plan["lds_bytes"] <= 160 * 1024
    if kind == "ez":  # the walk reads the pb_c table in LDS (the fresh tree reserves 64 simulations)
        assert plan["pbt_rows"] == PBT, plan
    assert_same_search(kind, a, b)
    assert (np.where(a["dist"] >= 0, a["dist"], 0).sum(axis=1) == S).all()  # (-1: past a root's legal actions)
    assert_walk_not_trivial(case, a)
    if case["rng"] == "glibc":
        oracle_replay(kind, a, B, S)
    if case["torch"]:
        torch_replay(kind, a, B, S)


# ---- dead K-parts of the head hidden layers ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mz", "ez"])
def test_dead_k_parts_are_never_read(kind):
    """A head whose K is below 1024 leaves the K-parts past it dead: the kernels skip them, so the zero padding
    the packed first-layer weights carry there is never read. With that padding overwritten by NaN in the packed
    network the search uses, the one-launch search and the generic path give the bits they gave before."""
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree, MuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    B, S, seed = 9, 10, 1
    mkw = dict(r_ch=6, hv=6, hp=10, H=256) if kind == "ez" else dict(r_ch=6, hv=6, hp=10)
    model = make_model(kind, 31, **mkw)
    kw = search_kwargs(dict(search={}, B=B, seed=seed), model)
    cls = EfficientZeroMCTSCtree if kind == "ez" else MuZeroMCTSCtree
    for fused in (True, False):
        clean = run_search(kind, B, S, seed, model=model, fused=fused, direct=True, check=True, **kw)
        cfg = EasyDict(dict(num_simulations=S, discount_factor=0.997, device=DEV, lstm_horizon_len=5,
                            fused_search=fused, model=dict(support_scale=kw["scales"][0],
                                                           categorical_distribution=True)))
        mcts = cls(cfg)
        hp = mcts._folded.get(model).heads
        dead = 0
        for head, K in enumerate((hp["Kr"], hp["off_policy"], hp["Khd"] - hp["off_policy"])):
            assert K % 128 == 0 and K < 1024
            hp["w1t"][head, K // 128:] = float("nan")
            dead += 8 - K // 128
        assert dead >= 10
        poisoned = run_search(kind, B, S, seed, model=model, mcts=mcts, fused=fused, direct=True, check=True, **kw)
        assert poisoned["path"] == clean["path"] and ("generic" == clean["path"]) == (not fused), clean["path"]
        assert_same_search(kind, clean, poisoned)
        assert np.isfinite(poisoned["rec"]["decoded"]).all() and np.isfinite(poisoned["rec"]["policy_logits"]).all()


# ---- S on either side of the pb_c table switch (EfficientZero) ------------------------------------------------
def _pbt_switch():
    """the largest S whose tree (lut_n = S + 8 pb_c rows once S simulations are reserved) still keeps the
    triangular pb_c table in LDS: lut_n (lut_n + 1) / 2 <= 4096 entries"""
    S = 65  # (past the 64 simulations a fresh tree reserves, so lut_n follows S)
    while (S + 9) * (S + 10) // 2 <= 4096:
        S += 1
    return S


@pytest.mark.parametrize("side", ["table", "division"])
def test_ez_pbt_table_switch(side):
    """EfficientZero at the last S that walks with the LDS pb_c table and the first that divides instead: the
    plan reports the switch, both equal the generic path and the oracle. (The trees are created for the test: the
    pool could hand over one that another search grew past the switch.)"""
    S = _pbt_switch() + (side == "division")
    B = 6 if side == "table" else 7
    case = dict(kind="ez", B=B, S=S, seed=1, model={}, search={}, rng="glibc", zero=False)
    a, b = both_paths(case)
    assert a["path"] == "fused" and b["path"] == "generic", (a["path"], b["path"])
    assert a["plan"]["supported"] and a["plan"]["pbt_rows"] == (S + 8 if side == "table" else 0), a["plan"]
    assert_same_search("ez", a, b)
    assert_walk_not_trivial(case, a)
    oracle_replay("ez", a, B, S)


# ---- the LDS boundary (MuZero) -----------------------------------------------------------------------------
def _mz_largest_S(model, B, lo=16, hi=400):
    """the largest S the plan accepts for `model` on a fresh tree of B roots (the tree lives in the workgroup's
    LDS): bisection over fresh trees"""
    from lightzero_amd.conv_infer import FoldedConvNet
    from lightzero_amd.tree import DeviceTree
    net = FoldedConvNet(model)

    def ok(S):
        t = DeviceTree(B, model.action_space_size, S, device=DEV)
        try:
            return t.search_conv_plan(net, S)["supported"]
        finally:
            t.close()
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("side", ["fits", "beyond"])
def test_mz_lds_boundary(side):
    """MuZero with 18 actions at the largest S whose tree fits the workgroup's LDS (one launch, = generic =
    oracle), and one simulation more: the plan refuses it, search() takes the generic path instead of raising
    and equals the oracle"""
    B = 5  # (each search on a tree created for it: the plan counts the tree's reserved capacity)
    model = make_model("mz", 7, A=18)
    S = _mz_largest_S(model, B) + (side == "beyond")
    kw = search_kwargs(dict(search={}, B=B, seed=1), model)
    a = run_search("mz", B, S, 1, model=model, direct=True, check=True, fresh_tree=True, **kw)
    assert a["path"] == ("fused-conv" if side == "fits" else "generic"), a["path"]
    assert a["plan"]["supported"] == (side == "fits"), a["plan"]
    if side == "fits":
        assert 158 * 1024 < a["plan"]["lds_bytes"] <= 159 * 1024, a["plan"]  # (one more simulation: ~0.7 KiB)
        b = run_search("mz", B, S, 1, model=model, fused=False, direct=True, check=True, fresh_tree=True, **kw)
        assert b["path"] == "generic"
        assert_same_search("mz", a, b)
    else:
        assert "LDS" in a["plan"]["reason"], a["plan"]
    assert a["rec"]["search_len"].max() >= 3
    oracle_replay("mz", a, B, S)


# ---- refusals: another path, never an exception ---------------------------------------------------------------
def test_ez_residency_refused_grid_runs_generic():
    """130 roots at LSTM width 1024: 3 x 64 tiles x 2 = 384 workgroups cannot be co-resident. The plan says so,
    search() launches nothing, counts the fallback and runs the generic path: equal to the oracle and to the
    generic path asked for directly. Inside a caller's stream capture the same search captures the generic path
    without launching or raising (a collector's graph with more envs than the grid holds)."""
    from lightzero_amd import _lib
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    from tests.test_gpu_conv import captured_search_equals_eager_generic
    B, S = 130, 8
    case = dict(kind="ez", B=B, S=S, seed=1, model=dict(H=1024), search={}, rng="glibc", zero=False)
    a, b = both_paths(case)
    assert a["path"] == "generic (co-residency refused)" and b["path"] == "generic", (a["path"], b["path"])
    plan = a["plan"]
    assert not plan["supported"] and plan["code"] == _lib.LZM_ERR_RESIDENCY and plan["lstm_tiles"] == 192 \
        and plan["workgroups"] == 384, plan
    assert_same_search("ez", a, b)
    assert_walk_not_trivial(case, a)
    oracle_replay("ez", a, B, S)
    # captured by the caller: an eager search first (buffers and packed network in place), then the capture
    model = a["model"]
    kw = search_kwargs(case, model)
    cfg = EasyDict(dict(num_simulations=S, discount_factor=0.997, device=DEV, lstm_horizon_len=5,
                        model=dict(support_scale=kw["scales"][0], categorical_distribution=True)))
    mcts = EfficientZeroMCTSCtree(cfg)
    w = run_search("ez", B, S, 1, model=model, mcts=mcts, record=False, direct=True, **kw)
    assert w["path"] == "generic (co-residency refused)" and mcts.residency_fallbacks == 1
    captured_search_equals_eager_generic(mcts, model, B, S, a["logits0"], a["lat0"], a["hidden0"])
    assert mcts.residency_fallbacks == 1 and mcts.last_path == "generic"
    assert mcts.last_plan["code"] == _lib.LZM_ERR_RESIDENCY


@pytest.mark.parametrize("kind", ["mz", "ez"])
def test_support_801_runs_on_both_paths(kind):
    """a support of 801 (past the 768 columns of lzm_conv_heads' three-per-thread form): the one-launch search
    takes it and the generic path's head kernel takes it in its four-column form — same bits, = oracle, =
    the torch module"""
    B, S = 9, 10
    case = dict(kind=kind, B=B, S=S, seed=1, model=dict(Vr=801, Vv=801), search={}, rng="glibc", zero=False)
    a, b = both_paths(case)
    assert a["path"] == ("fused" if kind == "ez" else "fused-conv") and b["path"] == "generic", (a["path"], b["path"])
    assert a["plan"]["supported"], a["plan"]
    assert_same_search(kind, a, b)
    assert_walk_not_trivial(case, a)
    oracle_replay(kind, a, B, S)
    torch_replay(kind, a, B, S)


REFUSED = [  # (id, kind, model arguments, native trunk packed, seed)
    ("support1201", "mz", dict(Vr=1201, Vv=1201), True, 1),   # past every head kernel: torch Linears
    ("support1201", "ez", dict(Vr=1201, Vv=1201), True, 1),
    ("blocks9", "mz", dict(blocks=9), False, 2),              # past the trunk kernel: the folded torch step
    ("blocks9", "ez", dict(blocks=9), False, 1),
    ("fc_value64", "mz", dict(fc_value=(64,)), True, 1),      # a hidden width the head kernels do not have
]


@pytest.mark.parametrize("id,kind,model_kw,native,seed", REFUSED)
def test_refused_network_runs_folded_torch_path(id, kind, model_kw, native, seed):
    """networks the native kernels refuse are folded and run through torch on the generic path: search() does not
    raise, the tree equals the oracle and the decoded values the torch module"""
    from lightzero_amd.conv_infer import FoldedConvNet
    B, S = 7, 8
    model = make_model(kind, seed + 100, **model_kw)
    net = FoldedConvNet(model)
    assert (net.native is not None) == native and getattr(net, "heads", None) is None
    kw = search_kwargs(dict(search={}, B=B, seed=seed), model)
    for fused in (True, False):
        a = run_search(kind, B, S, seed, model=model, fused=fused, direct=True, check=True, **kw)
        assert a["path"] == "generic", a["path"]
        assert a["rec"]["search_len"].max() >= 3
        oracle_replay(kind, a, B, S)
        torch_replay(kind, a, B, S)
