"""GPU: the one-launch Gumbel MuZero search (lzm_search_mlp_gumbel: search_mlp_kernel<R, TL, false, true>) behind
GumbelMuZeroMCTSCtree with cfg.fused_search set.

The tree logic is compared bit for bit with the host restatement (tests/gumbel_oracle.py, pinned to the reference's
transcripts by tests/test_gumbel_oracle.py): fed the decoded reward / value and the policy logits the kernel
recorded, the restatement asks the same requests (x, action, search_len, vtp) at every simulation and ends with
the same visit distributions, root values, improved policies, completed Q, trajectories and min-max pairs
(test_gpu_gumbel.assert_matches_restatement, the check the generic path passes). Nothing here has a tolerance
except the one network comparison, which is tests/mlp_numerics.py's with its own bounds.

Every one-launch case asserts last_path == "fused-mlp" and the launch plan it ran under
(DeviceTree.search_mlp_gumbel_plan, the function the launch itself decides with): roots per workgroup, the
streaming kernel, and whether the tree slice is in LDS — 2 x 16 B x cap x R <= 96 KB with cap = 1 + A (sims + 1)
nodes per root, sims the handle's reserved capacity (64 on pooled handles).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_gumbel as tg  # noqa: E402
from lightzero_amd import _lib  # noqa: E402
from mlp_numerics import check_search_network  # noqa: E402

DEV = torch.device("cuda", 0)


def wide_model(A, H, F, scale, seed=0, zero_heads=False, sharpen=None):
    """test_gpu_gumbel.mlp_model with the heads' hidden width F"""
    from lightzero_amd.model_mlp import MuZeroModelMLP
    torch.manual_seed(seed)
    V = 2 * scale + 1
    m = MuZeroModelMLP(observation_shape=4, action_space_size=A, latent_state_dim=H, fc_reward_layers=(F,),
                       fc_value_layers=(F,), fc_policy_layers=(F,), categorical_distribution=True,
                       reward_support_size=V, value_support_size=V, last_linear_layer_init_zero=zero_heads,
                       norm_type='BN')
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
    if sharpen is not None:
        tg.sharpen_heads(m, sharpen)
    return m.to(DEV).eval()


def expected_plan(t, R=1):
    cap = 1 + t.A * (t.sims_capacity + 1)
    return dict(roots_per_wg=R, kernel="streaming", mode=0, tree_in_lds=2 * 16 * cap * R <= 96 * 1024)


def make_mcts(S, m, discount=0.997, categorical=True, support_scale=10, fused=True):
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    cfg = dict(num_simulations=S, max_num_considered_actions=m, discount_factor=discount, device=DEV,
               use_hip_graph=False, env_type='not_board_games',
               model=dict(support_scale=support_scale, categorical_distribution=categorical))
    if fused is not None:  # None: the key absent
        cfg["fused_search"] = fused
    mcts = GumbelMuZeroMCTSCtree(EasyDict(cfg))
    mcts.record = True
    return mcts


def inputs(model, B, A, legal, seed):
    rng = np.random.default_rng(100 + seed)
    obs = torch.from_numpy(rng.random(size=(B, 4)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        out = model.initial_inference(obs)
    legal = [list(range(A))] * B if legal is None else [list(l) for l in legal]
    noises = np.zeros((B, A), np.float32)
    for i, l in enumerate(legal):
        noises[i, :len(l)] = rng.dirichlet([0.3] * len(l)).astype(np.float32)
    return dict(lat0=out.latent_state, logits0=out.policy_logits.float().cpu().numpy(), legal=legal, noises=noises,
                root_value=rng.normal(size=B).astype(np.float32))


def prepare(roots, x, noise, to_play):
    B = len(x["legal"])
    if noise:
        roots.prepare(0.25, [x["noises"][i, :len(l)].tolist() for i, l in enumerate(x["legal"])], [0.0] * B,
                      x["root_value"].tolist(), x["logits0"].tolist(), to_play)
    else:
        roots.prepare_no_noise([0.0] * B, x["root_value"].tolist(), x["logits0"].tolist(), to_play)


def run_search(model, B, A, S, m, legal=None, noise=True, discount=0.997, categorical=True, seed=0, support_scale=10,
               to_play=None, fused=True, path="fused-mlp", R=1, reserve=None):
    """test_gpu_gumbel.run_search with cfg.fused_search; path: the path the search must report (None: the one
    launch exactly when the library's plan takes the shape); R: the roots per workgroup the plan must report; reserve: a fresh handle reserved for that many simulations (closed by
    finish()) instead of a pooled one of the default capacity. Returns its result dict plus model, pool, plan."""
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    from lightzero_amd.tree import DeviceTree
    x = inputs(model, B, A, legal, seed)
    to_play = [-1] * B if to_play is None else to_play
    mcts = make_mcts(S, m, discount, categorical, support_scale, fused)
    roots = GumbelMuZeroMCTSCtree.roots(B, x["legal"])
    if reserve is not None:
        roots.tree = DeviceTree(B, A, reserve, gumbel=True, device=DEV)
    prepare(roots, x, noise, to_play)
    mcts.search(roots, model, x["lat0"], to_play)
    if path is None:
        took = roots.tree.search_mlp_gumbel_plan(mcts._packed.get(model, DEV)[1], S)["kernel"] is not None
        path = "fused-mlp" if took else "generic"
    assert mcts.last_path == path
    plan = None
    if path == "fused-mlp":
        dims = mcts._packed.get(model, DEV)[1]
        plan = roots.tree.search_mlp_gumbel_plan(dims, S)
        assert plan == expected_plan(roots.tree, R), plan
    disc = float(np.float32(discount))
    return dict(out=tg.device_outputs(roots, disc, A, S), roots=roots, mcts=mcts, legal=x["legal"],
                noises=x["noises"] if noise else None, root_value=x["root_value"], logits0=x["logits0"], disc=disc,
                to_play=to_play, rec=mcts.last_record.numpy(), model=model, pool=mcts._buf.pool.clone(), plan=plan,
                owned=reserve is not None, inputs=x)


def finish(r):
    if r["owned"]:
        t = r["roots"].tree
        r["roots"].tree = None
        t.close()
    else:
        r["roots"].clear()


# ------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("B,A,S,m,kw", [
    (5, 2, 8, 4, {}),
    (7, 6, 1, 4, {}),                               # one simulation
    (4, 6, 12, 1, {}),                              # m = 1
    (4, 3, 5, 16, {}),                              # m > S and m > A
    (2, 64, 33, 16, dict(H=64)),                    # the lane limit, A = H (the tree stays in HBM: 4161 nodes)
    (4, 4, 8, 4, dict(discount=1.0)),
    (4, 4, 8, 4, dict(noise=False)),
    (4, 4, 8, 4, dict(to_play=[1, 2, 2, 1])),       # to_play passes through: no flip in the kernel's expand
    (16, 18, 50, 16, {}),                           # the long case
])
def test_one_launch_matches_restatement(B, A, S, m, kw):
    kw = dict(kw)
    model = tg.mlp_model(A, H=kw.pop("H", 32), seed=B + A)
    r = run_search(model, B, A, S, m, seed=B + S, **kw)
    tg.assert_matches_restatement(r, A, S, m)
    if "to_play" in kw:
        assert r["rec"]["vtp"].tolist() == [kw["to_play"]] * S
    if A == 64:
        assert r["plan"]["tree_in_lds"] is False
    finish(r)


def test_ragged_case_reaches_the_fallback():
    """test_gpu_gumbel's case of the same name through the one launch: the two-legal root finds no child with the
    considered visit count at simulations 2 and 3 and takes legal[0]; the one-action root has one choice"""
    model = tg.mlp_model(4, seed=7)
    r = run_search(model, 3, 4, 8, 4, legal=tg.RAGGED, seed=11)
    dist = r["out"]["dist"]
    assert dist[1, :2].sum() == 8 and dist[2, 0] == 8 and dist[0].sum() == 8
    tg.assert_matches_restatement(r, 4, 8, 4)
    finish(r)


def test_zeroed_heads_all_ties():
    model = tg.mlp_model(5, zero_heads=True, seed=3)
    r = run_search(model, 6, 5, 12, 4, legal=[[0, 1, 2, 3, 4], [2, 4], [1, 2, 3], [3], [0, 4], [0, 1, 2, 3, 4]], seed=5)
    assert np.all(r["rec"]["policy_logits"] == r["rec"]["policy_logits"][..., :1])
    assert np.all(r["rec"]["decoded"] == 0)
    tg.assert_matches_restatement(r, 5, 12, 4)
    finish(r)


# ------------------------------------------------------------------------------------------- float and shape edges
A64_RAGGED = [list(range(64)), [a for a in range(64) if a % 3 != 0], [63]]
PERM9 = [list(range(9))[::-1], [8, 2], [5, 0, 7, 1, 3], [4]]


def assert_sharp(r, extreme):
    """extreme (sharpen 400): the policy logits spread past 104, where expf underflows and priors become exact
    zeros, and the categorical heads sit on single support bins, so decoded values repeat exactly (these models'
    logits spread about 0.34 per unit of sharpening: 10 at 30, 34 at 100, 135 at 400)"""
    dec = r["rec"]["decoded"]
    assert np.all(np.isfinite(dec)) and np.all(np.isfinite(r["rec"]["policy_logits"]))
    if extreme:
        assert np.ptp(r["rec"]["policy_logits"], axis=-1).min() > 104
        assert np.unique(dec[..., 1]).size < dec[..., 1].size


@pytest.mark.parametrize("sharpen", [30, 100, 400])
@pytest.mark.parametrize("fused", [True, None])
def test_sharpened_heads(sharpen, fused):
    """(fused None: the twin on the generic path, so both kernels see the same regime)"""
    B, A, S, m = 4, 6, 30, 4
    model = tg.mlp_model(A, seed=B + A, sharpen=sharpen)
    r = run_search(model, B, A, S, m, seed=B + S, fused=fused, path="generic" if fused is None else "fused-mlp")
    assert_sharp(r, sharpen >= 400)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


def test_sharpened_heads_wide_ragged():
    """A = 64 = H with ragged roots that miss action 0 or hold only action 63; 4,161 nodes per root: the tree in HBM"""
    B, A, S, m = 3, 64, 40, 16
    model = tg.mlp_model(A, H=64, seed=B + A, sharpen=30)
    r = run_search(model, B, A, S, m, legal=A64_RAGGED, seed=B + S)
    assert r["plan"]["tree_in_lds"] is False
    assert_sharp(r, False)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


def test_deepest_path():
    """one action, 64 simulations: every walk one node longer than the last, the 64th 64 long, at the pooled
    handle's full capacity (depth_cap = 66 path entries in the workgroup's LDS slice)"""
    B, A, S, m = 3, 1, 64, 4
    r = run_search(tg.mlp_model(A, seed=B + A), B, A, S, m, seed=B + S, path=None)
    assert r["roots"].tree.sims_capacity == S
    assert r["rec"]["search_len"].tolist() == [[k + 1] * B for k in range(S)]
    if r["plan"] is not None:
        assert r["plan"]["tree_in_lds"] is True
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


@pytest.mark.parametrize("S,m", [(33, 0), (33, 3), (33, 5), (33, 7), (64, 5)])
def test_odd_considered_counts(S, m):
    """sequential halving with m no power of two and m = 0; (64, 5) at the pooled handle's full capacity"""
    B, A = 4, 9
    r = run_search(tg.mlp_model(A, seed=B + A + m), B, A, S, m, seed=S + m)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


@pytest.mark.parametrize("R", [1, 2])
def test_permuted_legal_lists(R, monkeypatch):
    """legal lists that are not ascending: lane j is legal position j, the noise and the Gumbel vector are by
    position, and only the root outputs map position back to action"""
    monkeypatch.setenv("LZM_ROOTS_PER_WG", str(R))
    B, A, S, m = 4, 9, 20, 4
    r = run_search(tg.mlp_model(A, seed=B + A), B, A, S, m, legal=PERM9, seed=B + S, R=R)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


def test_discount_zero():
    B, A, S, m = 4, 4, 8, 4
    r = run_search(tg.mlp_model(A, seed=B + A), B, A, S, m, seed=B + S, discount=0.0)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


# ------------------------------------------------------------------------------------------- roots per workgroup
@pytest.mark.parametrize("R", [2, 8])
def test_roots_per_workgroup(R, monkeypatch):
    """a partial last workgroup (11 roots) and several waves walking at once"""
    monkeypatch.setenv("LZM_ROOTS_PER_WG", str(R))
    B, A, S, m = 11, 3, 12, 4
    r = run_search(tg.mlp_model(A, seed=R), B, A, S, m, seed=R, R=R)
    assert r["plan"]["tree_in_lds"] is True
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


@pytest.mark.parametrize("R,in_lds", [(4, False), (1, True)])
def test_tree_in_hbm_and_in_lds(R, in_lds, monkeypatch):
    """18 actions x 50 simulations reserved: 919 nodes per root. Four roots' two 16-byte arrays are past 96 KB, so
    the records and raw_value stay in HBM while the paths stay in LDS; one root's fit."""
    monkeypatch.setenv("LZM_ROOTS_PER_WG", str(R))
    B, A, S, m = 6, 18, 50, 16
    r = run_search(tg.mlp_model(A, seed=4), B, A, S, m, seed=9, R=R, reserve=S)
    assert r["roots"].tree.sims_capacity == S
    assert r["plan"] == dict(roots_per_wg=R, kernel="streaming", mode=0, tree_in_lds=in_lds)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


# ------------------------------------------------------------------------------------------- network widths
@pytest.mark.parametrize("H,F,scale,A,numerics", [
    (16, 16, 10, 9, False),
    (256, 32, 300, 4, True),
    (64, 32, 256, 2, False),   # V = 513: decoded from registers
])
def test_network_widths(H, F, scale, A, numerics):
    """the raw_value slice and the Gumbel tables beside other schedules' LDS layouts"""
    B, S, m = 8, 12, 4
    model = wide_model(A, H, F, scale, seed=H + A)
    r = run_search(model, B, A, S, m, seed=H, support_scale=scale)
    tg.assert_matches_restatement(r, A, S, m)
    if numerics:  # the network code is the shared one: this shows the schedule still sees the right rows
        check_search_network(f"gumbel search H{H} F{F} V{2 * scale + 1} A{A}", r, S, B, scale)
    finish(r)


# ------------------------------------------------------------------------------------------- repeatability
def same_outputs(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              np.asarray(b[k]).view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


@pytest.mark.parametrize("reserve", [None, 40])
def test_repeat_on_the_same_roots(reserve):
    """the same Roots prepared again and searched again — on a pooled handle and on one reserved for more
    simulations than the search runs — gives the same bits: nothing of a search outlives it"""
    B, A, S, m = 9, 6, 10, 4
    model = tg.mlp_model(A, seed=21)
    r = run_search(model, B, A, S, m, seed=2, reserve=reserve)
    tg.assert_matches_restatement(r, A, S, m)
    mm1 = r["roots"]._last_minmax.cpu().numpy().copy()
    prepare(r["roots"], r["inputs"], True, r["to_play"])
    r["mcts"].search(r["roots"], model, r["inputs"]["lat0"], r["to_play"])
    assert r["mcts"].last_path == "fused-mlp"
    again = tg.device_outputs(r["roots"], r["disc"], A, S)
    assert same_outputs(r["out"], again)
    assert np.array_equal(mm1.view(np.uint32), r["roots"]._last_minmax.cpu().numpy().view(np.uint32))
    rec2 = r["mcts"].last_record.numpy()
    for k in ("x", "action", "search_len", "vtp"):
        assert np.array_equal(r["rec"][k], rec2[k]), k
    finish(r)


# ------------------------------------------------------------------------------------------- fallbacks
@pytest.mark.parametrize("why", ["scalar heads", "head_hidden 24", "fused_search absent"])
def test_fallbacks_take_the_generic_path(why):
    B, A, S, m = 4, 4, 8, 4
    if why == "scalar heads":
        r = run_search(tg.mlp_model(A, categorical=False, seed=1), B, A, S, m, categorical=False, path="generic")
    elif why == "head_hidden 24":
        r = run_search(wide_model(A, 32, 24, 10, seed=1), B, A, S, m, path="generic")
    else:
        r = run_search(tg.mlp_model(A, seed=1), B, A, S, m, fused=None, path="generic")
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


def test_wide_latent_with_several_roots_per_workgroup_takes_the_generic_path(monkeypatch):
    """the measured routing rule of _fused: a latent wider than 512 runs the one launch only at one root per
    workgroup (the kernel itself accepts both: the plan reports it)"""
    B, A, S, m, H = 2, 3, 2, 2, 1024
    model = wide_model(A, H, 32, 10, seed=6)
    r = run_search(model, B, A, S, m, seed=1)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)
    monkeypatch.setenv("LZM_ROOTS_PER_WG", "2")
    r = run_search(model, B, A, S, m, seed=1, path="generic")
    dims = r["mcts"]._packed.get(model, DEV)[1]
    assert r["roots"].tree.search_mlp_gumbel_plan(dims, S) == expected_plan(r["roots"].tree, 2)
    tg.assert_matches_restatement(r, A, S, m)
    finish(r)


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch():
    from lightzero_amd.fused import PackedCache
    from lightzero_amd.tree import DeviceTree, new_minmax, seed_tensor
    B, A, S, H = 4, 3, 8, 32
    model = tg.mlp_model(A, seed=2)
    packed, dims = PackedCache().get(model, DEV)
    gt = DeviceTree(B, A, S, gumbel=True, device=DEV)
    mt = DeviceTree(B, A, S, device=DEV)
    sentinel = torch.full((B, 4), 7.0, device=DEV)
    mm = sentinel.clone()
    vtp = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    pool = torch.zeros((S + 2, B, H), device=DEV)
    seeds = torch.zeros(S + 1, dtype=torch.int32, device=DEV)
    L, p = _lib.load(), _lib.ptr

    def gumbel(h, sims=S, considered=4):
        rc = L.lzm_search_mlp_gumbel(h, dims["hidden"], dims["head_hidden"], dims["support"], int(dims["res"]),
                                     p(packed), sims, considered, 0.997, p(mm), p(vtp), p(pool), None, None, None,
                                     None, None, _lib.stream_ptr())
        return rc, L.lzm_last_error().decode()

    assert gt.search_mlp_gumbel_plan(dims, S) == expected_plan(gt)
    assert mt.search_mlp_gumbel_plan(dims, S)["kernel"] is None    # a handle of another kind
    assert gt.search_mlp_plan(dims, S)["kernel"] is None
    # lzm_search_mlp_gumbel on a MuZero handle
    rc, msg = gumbel(mt.h)
    assert rc == _lib.LZM_ERR_STATE and msg.startswith("lzm_search_mlp_gumbel:"), (rc, msg)
    with pytest.raises(_lib.LzmError):
        mt.search_mlp_gumbel(dims, packed, S, 4, mm, vtp, pool)
    # lzm_search_mlp on a Gumbel handle
    rc = L.lzm_search_mlp(gt.h, dims["hidden"], dims["head_hidden"], dims["support"], int(dims["res"]), p(packed), S,
                          19652, 1.25, 0.997, p(mm), p(seeds), p(vtp), p(pool), None, None, None, None, None,
                          _lib.stream_ptr())
    assert rc == _lib.LZM_ERR_STATE
    with pytest.raises(_lib.LzmError):
        gt.search_mlp(dims, packed, S, mm, seeds, vtp, pool)
    # S beyond the reserved capacity; S <= 0 and m < 0
    rc, msg = gumbel(gt.h, sims=S + 1)
    assert rc == _lib.LZM_ERR_CAPACITY and msg.startswith("lzm_search_mlp_gumbel:"), (rc, msg)
    with pytest.raises(_lib.LzmError):
        gt.search_mlp_gumbel(dims, packed, S + 1, 4, mm, vtp, pool)
    for kw in (dict(sims=0), dict(considered=-1)):
        rc, msg = gumbel(gt.h, **kw)
        assert rc == _lib.LZM_ERR_ARG and msg.startswith("lzm_search_mlp_gumbel:"), (rc, msg)
    # a handle in collect-step mode: there is no Gumbel collect step
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    dist = torch.zeros((B, A), dtype=torch.int32, device=DEV)
    vals = torch.zeros(B, device=DEV)
    gt.set_step(count, 0, True, dist, vals, True, 0.01)
    rc, msg = gumbel(gt.h)
    assert rc == _lib.LZM_ERR_STATE and msg.startswith("lzm_search_mlp_gumbel:"), (rc, msg)
    gt.set_step()
    # nothing ran: the min-max rows, the counter and the handle's visit counts are as they were
    torch.cuda.synchronize()
    assert torch.equal(mm, sentinel) and int(count.item()) == 0
    assert int(gt.distributions().clamp(min=0).sum().item()) == 0
    gt.close()
    mt.close()
