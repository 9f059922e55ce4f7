"""GPU: the one-launch EfficientZero search over EfficientZeroModelMLP (lzm_search_mlp_ez), the reward LSTM in the
kernel.

1. Tree parity: OracleTree(ez=True) reproduces every search when fed the recorded decoded value prefix, value,
   policy logits and is_reset: requests and is_reset at every simulation, final visit counts and trajectories bit
   for bit, root values within 1e-5 — over the reset rule, the batch edges, every roots-per-workgroup variant, both
   lane splits of the gate layer, several actions / two players / ragged legal sets, all-tie trees and Philox.
2. Network numerics (base and width cases): next latent and policy logits through tests/mlp_numerics.check_scaled
   (at most 4 x torch-f32's error ratio and at most 2^-16 of the element's scale); h1 / c1 read back from the state
   pools' non-reset rows against float64 with the cell's scale (the largest gate chunk of |W| |[x; h]| + |b|, times
   1 + |c0|, x's scale propagated through the dynamics layers); reset rows exactly 0; decoded value prefix and
   value rtol 1e-4, atol 1e-5 x support scale against the float64 decode.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.oracle import OracleTree  # noqa: E402
from tests.helpers import DISC, NOISE_W, PB_C_BASE, PB_C_INIT, VDM  # noqa: E402
from tests.mlp_numerics import check_scaled, inverse_scalar_transform64  # noqa: E402
from tests.test_gpu_fused import DEV, SETTINGS, settings_id  # noqa: E402


def make_ez_model(A, H, Hl, zero_heads=False, seed=0, support_scale=300, res=False):
    from lightzero_amd.model_mlp import EfficientZeroModelMLP
    torch.manual_seed(seed)
    m = EfficientZeroModelMLP(observation_shape=4, action_space_size=A, lstm_hidden_size=Hl, latent_state_dim=H,
                              reward_support_size=2 * support_scale + 1, value_support_size=2 * support_scale + 1,
                              categorical_distribution=True, last_linear_layer_init_zero=zero_heads, norm_type='BN',
                              res_connection_in_dynamics=res)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
    return m.to(DEV).eval()


def ez_fused_search(B, S, A=2, H=128, Hl=128, horizon=5, zero_heads=False, players=1, fast=False, seed=0,
                    support_scale=300, res=False, fused=True, ragged=False, settings=None):
    """tests/test_gpu_fused.py's fused_search for EfficientZeroMCTSCtree over an EfficientZeroModelMLP: a seeded
    model with randomised BatchNorm statistics, Dirichlet noise, SequentialSeeds and record = True; the roots'
    LSTM state is random. ragged: random legal subsets per root. Returns the record (with is_reset),
    distributions, values, trajectories, the three pools, the search diagnostics of this search and its plan."""
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree
    from lightzero_amd.tree import SequentialSeeds, set_seed_source
    from lightzero_amd.utils import EasyDict
    model = make_ez_model(A, H, Hl, zero_heads, seed, support_scale, res)
    rng = np.random.default_rng(seed)
    obs = torch.from_numpy(rng.normal(size=(B, 4)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        out = model.initial_inference(obs)
    hidden0 = tuple(torch.from_numpy((0.5 * rng.standard_normal((1, B, Hl))).astype(np.float32)).to(DEV)
                    for _ in range(2))
    logits0 = out.policy_logits.float().cpu().numpy()
    noises = rng.dirichlet([0.3] * A, size=B).astype(np.float32)
    to_play = [-1] * B if players == 1 else rng.integers(1, 3, size=B).tolist()
    legal = [list(range(A))] * B
    if ragged:
        legal = [sorted(rng.choice(A, size=int(rng.integers(1, A + 1)), replace=False).tolist()) for _ in range(B)]
    cfg = EasyDict(dict(dict(num_simulations=S, discount_factor=float(DISC), device=DEV, lstm_horizon_len=horizon,
                             model=dict(support_scale=support_scale, categorical_distribution=True)), **(settings or {})))
    cls = EfficientZeroMCTSCtree
    old = cls.rng_mode
    cls.rng_mode = "philox" if fast else "glibc"
    try:
        mcts = cls(cfg)
        mcts.record = True
        roots = cls.roots(B, legal)
        roots.prepare(float(NOISE_W), [n.tolist() for n in noises], [0.0] * B, logits0.tolist(), to_play)
        t = roots.tree
        diag0 = t.search_diagnostics()
        set_seed_source(SequentialSeeds(seed))
        try:
            mcts.search(roots, model, out.latent_state, hidden0, to_play)
        finally:
            set_seed_source(None)
        fz = mcts._fused(model, t, Hl, S)
        assert (fz is not None) == fused, "model should take the {} path".format("fused" if fused else "generic")
        assert mcts.last_path == ("fused-mlp" if fused else "generic")
        rec = mcts.last_record.numpy() | {"is_reset": mcts.last_record.is_reset.cpu().numpy()}
        buf = mcts._buf
        res_ = dict(rec=rec, dist=t.distributions().cpu().numpy(), values=t.values().cpu().numpy(),
                    traj=t.trajectories(S + 2).cpu().numpy(), pool=buf.pool.clone(), hpool=buf.extra[0].clone(),
                    cpool=buf.extra[1].clone(), diag=[a - b for a, b in zip(t.search_diagnostics(), diag0)],
                    model=model, logits0=logits0, noises=noises, to_play=np.array(to_play, np.int32), legal=legal,
                    plan=t.search_mlp_ez_plan(fz[1], S) if fused else None, horizon=horizon, fast=fast, B=B, S=S, A=A,
                    scale=support_scale)
        roots.clear()
        return res_
    finally:
        cls.rng_mode = old


def check_tree_exact(B, S, pb_c_base=PB_C_BASE, pb_c_init=PB_C_INIT, value_delta_max=VDM, discount=DISC, horizon=5,
                     **search_kw):
    """tests/test_gpu_fused.py's check_tree_exact for the EfficientZero search: the settings go both to the search
    cfg and to the oracle; the root values bit for bit"""
    pb_c_init, value_delta_max, discount = np.float32(pb_c_init), np.float32(value_delta_max), np.float32(discount)
    settings = dict(pb_c_base=int(pb_c_base), pb_c_init=float(pb_c_init), value_delta_max=float(value_delta_max),
                    discount_factor=float(discount))
    r = fused(ez_fused_search(B, S, horizon=horizon, settings=settings, **search_kw))
    return check_oracle(r, pb_c_base, pb_c_init, value_delta_max, discount, exact_values=True)


def check_oracle(r, pb_c_base=PB_C_BASE, pb_c_init=PB_C_INIT, value_delta_max=VDM, discount=DISC, exact_values=False):
    """OracleTree(ez=True) fed the recorded network outputs and is_reset reproduces the run
    (tests/test_gpu_conv.py's oracle_replay, with the Philox form of tests/test_gpu_fused.py)"""
    rec, B, S, A, horizon = r["rec"], r["B"], r["S"], r["A"], r["horizon"]
    assert r["diag"][0] == 0, "look-back spin timeout"
    assert r["diag"][3] == 0
    ot = OracleTree(B, A, S, ez=True, fast_rng=r["fast"])
    la = np.full((B, A), -1, np.int32)
    for i, l in enumerate(r["legal"]):
        la[i, :len(l)] = l
    ot.set_legal(la, np.array([len(l) for l in r["legal"]], np.int32))
    ot.set_delta(value_delta_max)
    ot.prepare(NOISE_W, r["noises"], np.zeros(B, np.float32), r["logits0"], r["to_play"])
    for k in range(S):
        x, y, a, vtp, slen = ot.traverse(pb_c_base, pb_c_init, discount, int(rec["seeds"][k]), r["to_play"])
        assert np.array_equal(x, rec["x"][k]), f"sim {k}: latent index differs"
        assert np.array_equal(a, rec["action"][k]), f"sim {k}: action differs"
        assert np.array_equal(slen, rec["search_len"][k]), f"sim {k}: search_len differs"
        is_reset = (slen % horizon == 0).astype(np.int32)
        assert np.array_equal(is_reset, rec["is_reset"][k]), f"sim {k}: is_reset differs"
        ot.backprop(k + 1, discount, rec["decoded"][k][:, 0], rec["decoded"][k][:, 1], rec["policy_logits"][k], vtp,
                    is_reset)
    assert np.array_equal(r["dist"], ot.distributions())
    assert np.array_equal(r["traj"], ot.trajectories(S + 2))
    np.testing.assert_allclose(r["values"], ot.values(), rtol=0, atol=1e-5)
    if exact_values:
        assert np.array_equal(r["values"].view(np.uint32), ot.values().view(np.uint32))
    return r


def fused(r, roots_per_wg=None):
    assert r["plan"]["kernel"] == "streaming", r["plan"]
    if roots_per_wg is not None:
        assert r["plan"]["roots_per_wg"] == roots_per_wg, r["plan"]
    return r


def ez_scales(model, lat, h0, c0, act):
    """A of (next latent, policy logits, the cell) for recurrent_inference(lat, (h0, c0), act), float64 inputs:
    the network with every weight, bias and input replaced by its absolute value and every activation by the
    identity (tests/mlp_numerics.py), the cell's as tests/test_gpu_conv_numerics.py's LSTM check"""
    from lightzero_amd.fused import describe_ez
    layers, dims = describe_ez(model)
    W = [(w.detach().cpu().double().abs(), b.detach().cpu().double().abs()) for (w, b), _ in layers]
    lin = lambda x, l: F.linear(x, W[l][0], W[l][1])
    x = torch.cat((lat.abs(), F.one_hot(act, dims["actions"]).double()), dim=1)
    nxt = lin(lin(x, 0), 1)
    o, xin = 2, nxt
    if dims["res"]:
        nxt = nxt + lat.abs()
        xin = lin(lin(nxt, 2), 3)
        o = 4
    Ag = lin(torch.cat((xin, h0.abs()), dim=1), o)
    Ab = torch.stack(Ag.chunk(4, dim=1)).amax(dim=0) * (1 + c0.abs())
    p = lin(lin(nxt, o + 3), o + 4)
    return nxt, lin(lin(p, o + 7), o + 8), Ab


def check_network(name, r):
    model, rec, B, S, A, scale = r["model"], r["rec"], r["B"], r["S"], r["A"], r["scale"]
    pool, hpool, cpool = r["pool"].cpu(), r["hpool"].cpu(), r["cpool"].cpu()
    x = torch.from_numpy(rec["x"]).long()
    idx = torch.arange(B)
    gat = lambda p: torch.stack([p[x[k], idx] for k in range(S)]).reshape(S * B, -1)
    lat, h0, c0 = gat(pool), gat(hpool), gat(cpool)
    act = torch.from_numpy(rec["action"]).long().reshape(S * B)
    with torch.no_grad():
        m64, m32 = copy.deepcopy(model).cpu().double().eval(), copy.deepcopy(model).cpu().float().eval()
        ref = m64.recurrent_inference(lat.double(), (h0.double().unsqueeze(0), c0.double().unsqueeze(0)), act)
        f32 = m32.recurrent_inference(lat, (h0.unsqueeze(0), c0.unsqueeze(0)), act)
        a_lat, a_pol, a_cell = ez_scales(model, lat.double(), h0.double(), c0.double(), act)
    keep = torch.from_numpy(rec["is_reset"]).reshape(S * B) == 0
    h1, c1 = hpool[1:S + 1].reshape(S * B, -1), cpool[1:S + 1].reshape(S * B, -1)
    assert keep.any()
    assert not h1[~keep].any() and not c1[~keep].any(), "reset rows of the state pools must be exactly 0"
    rh, rc = ref.reward_hidden_state[0][0], ref.reward_hidden_state[1][0]
    fh, fc = f32.reward_hidden_state[0][0], f32.reward_hidden_state[1][0]
    check_scaled(name, dict(
        latent=(pool[1:S + 1].reshape(S * B, -1), ref.latent_state, a_lat, f32.latent_state),
        policy=(torch.from_numpy(rec["policy_logits"]).reshape(S * B, A), ref.policy_logits, a_pol, f32.policy_logits),
        h1=(h1[keep], rh[keep], a_cell[keep], fh[keep]),
        c1=(c1[keep], rc[keep], a_cell[keep], fc[keep])))
    dec = torch.from_numpy(rec["decoded"]).reshape(S * B, 2)
    torch.testing.assert_close(dec[:, 0], inverse_scalar_transform64(ref.value_prefix, scale).float(), rtol=1e-4,
                               atol=1e-5 * scale)
    torch.testing.assert_close(dec[:, 1], inverse_scalar_transform64(ref.value, scale).float(), rtol=1e-4,
                               atol=1e-5 * scale)


def test_base_zoo_shape():
    r = check_oracle(fused(ez_fused_search(16, 20, A=2, H=128, Hl=128, horizon=5, seed=1)))
    check_network("ez mlp base", r)
    assert r["rec"]["is_reset"].any() and not r["rec"]["is_reset"].all()


@pytest.mark.parametrize("horizon", [1, 3, 17])  # every leaf resets; a mix; S + 1: no leaf ever resets
def test_reset_rule(horizon):
    B, S = 8, 16
    r = check_oracle(fused(ez_fused_search(B, S, horizon=horizon, seed=horizon)))
    rst, slen = r["rec"]["is_reset"], r["rec"]["search_len"]
    if horizon == 1:
        assert rst.all() and not r["hpool"][1:].any() and not r["cpool"][1:].any()
    elif horizon == 3:
        deep = slen >= 2
        assert (rst[deep] == 1).any() and (rst[deep] == 0).any(), "no reset and non-reset leaf at search_len >= 2"
    else:
        assert not rst.any()


@pytest.mark.parametrize("B,S,rpw", [(1, 20, None), (7, 20, 4), (300, 8, 1)],
                         ids=["one_root", "partial_last_workgroup", "more_workgroups_than_cus"])
def test_batch_edges(B, S, rpw, monkeypatch):
    if rpw is not None:
        monkeypatch.setenv("LZM_ROOTS_PER_WG", str(rpw))
    check_oracle(fused(ez_fused_search(B, S, seed=B), rpw))


@pytest.mark.parametrize("rpw", [1, 2, 4])
def test_roots_per_workgroup(rpw, monkeypatch):
    monkeypatch.setenv("LZM_ROOTS_PER_WG", str(rpw))
    check_oracle(fused(ez_fused_search(16, 12, A=3, players=2, seed=5), rpw))


# (H, Hl): (48, 80) padded columns, the split gate layer; (64, 128) gates exactly one round of 512; (128, 64) two
# lanes per gate column; (128, 256) two gate columns per lane; (256, 512) the model's defaults, four per lane
@pytest.mark.parametrize("scale", [300, 50], ids=["v601", "v101"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("H,Hl", [(48, 80), (64, 128), (128, 64), (128, 256), (256, 512)])
def test_widths(H, Hl, res, scale):
    r = check_oracle(fused(ez_fused_search(16, 20, A=2, H=H, Hl=Hl, res=res, support_scale=scale, seed=H + Hl)))
    check_network(f"ez mlp H{H} Hl{Hl} res{int(res)} V{2 * scale + 1}", r)


@pytest.mark.parametrize("rpw", [None, 4])
@pytest.mark.parametrize("A", [3, 6])
def test_actions_players_ragged_legal(A, rpw, monkeypatch):
    if rpw is not None:
        monkeypatch.setenv("LZM_ROOTS_PER_WG", str(rpw))
    check_oracle(fused(ez_fused_search(16, 20, A=A, players=2, ragged=True, seed=A), rpw))


def test_all_tie_trees_resolved_serially():
    r = check_oracle(fused(ez_fused_search(16, 20, zero_heads=True, seed=2)))
    assert r["diag"][1] > 0, "no slice was resolved serially (a tie that reached an expanded child)"


@pytest.mark.parametrize("zero_heads", [False, True], ids=["rand", "zero"])
def test_philox(zero_heads):
    check_oracle(fused(ez_fused_search(16, 20, zero_heads=zero_heads, fast=True, seed=4)))


# tests/test_gpu_fused.py's settings on the EfficientZero kernel (it has the weight-streaming form only), and the
# horizon's two ends: every leaf resets, none does (S + 5)
@pytest.mark.parametrize("A", [2, 3])
@pytest.mark.parametrize("settings", SETTINGS + [dict(horizon=1), dict(horizon=35)], ids=settings_id)
def test_one_launch_kernel_at_other_settings(settings, A):
    B, S = 16, 30
    r = check_tree_exact(B, S, A=A, H=64, Hl=128, seed=A, **settings)
    assert r["plan"]["kernel"] == "streaming", r["plan"]  # (ez_fused_search asserts last_path == "fused-mlp")
    rst = r["rec"]["is_reset"]
    if "horizon" in settings:
        assert rst.all() if settings["horizon"] == 1 else not rst.any()
    assert r["rec"]["search_len"].max() >= 3


def test_refused_width_takes_the_generic_path():
    """Hl 72 (no multiple of 16) is refused by lzm_search_mlp_ez_supported: the generic per-simulation path, the
    same oracle exactness, not an error"""
    r = ez_fused_search(16, 20, Hl=72, fused=False, seed=6)
    assert r["plan"] is None
    check_oracle(r)
