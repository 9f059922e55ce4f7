"""GPU: the one-launch Stochastic MuZero search (lzm_search_mlp_stoch: search_stoch_mlp_kernel<R, TL>) behind
StochasticMuZeroMCTSCtree with cfg.fused_search set, over StochasticMuZeroModelMLP.

Tree: the host restatement tests/stochastic_oracle.py, fed the decoded reward / value and the logits row the kernel
recorded, under the same Philox seeds — no tolerance. Network: float64 through the kind each row had, within
tests/mlp_numerics.py's bounds. Distinct, independently initialised branch networks with randomised BatchNorm
statistics (shared_dynamics=False) make a stale weight prefetch or a swapped head a network mismatch.
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mlp_numerics as mn  # noqa: E402
import stochastic_oracle as so  # noqa: E402
from test_gpu_stochastic import PB_C, bits  # noqa: E402

DEV = torch.device("cuda", 0)
SCALE = 10  # support 21
RAGGED = [[2, 0, 1], [1], [0, 3], [3, 1, 2, 0], [0, 1]]
# B, S, A, C, H and the options; R: roots per workgroup the plan must pick at that B on a 256-CU device
SHAPES = {
    "a2c2": dict(B=5, S=8, A=2, C=2),
    "a4c2_noise_ragged": dict(B=5, S=8, A=4, C=2, noise=True, legal=RAGGED),
    "a3c3_2p": dict(B=5, S=8, A=3, C=3, players=2),
    "a64c64_h64_hbm": dict(B=3, S=6, A=64, C=64, H=64, lds=False),
    "s1": dict(B=5, S=1, A=4, C=2),
    "s2": dict(B=5, S=2, A=4, C=2, legal=RAGGED),  # (the root with one legal action reaches a decision leaf)
    "b1_disc1_res": dict(B=1, S=8, A=4, C=2, disc=1.0, res=True),
    "b259_r2": dict(B=259, S=5, A=4, C=2, R=2),
    "b515_r4_noise": dict(B=515, S=5, A=3, C=3, R=4, noise=True),
    "b1027_r8_2p": dict(B=1027, S=5, A=4, C=2, R=8, players=2),
    "reserved_800_hbm": dict(B=5, S=8, A=4, C=2, reserve=800, lds=False),
    "a2c2_h128_v601": dict(B=5, S=8, A=2, C=2, H=128, scale=300),  # the zoo widths: the wide (in-register) decode
    "a2c2_shared": dict(B=5, S=8, A=2, C=2, shared=True),
    "b259_r2_shared_res": dict(B=259, S=5, A=4, C=2, R=2, shared=True, res=True),
}


def make_model(A, C, H, shared, res, seed, scale=SCALE):
    from lightzero_amd.model_mlp import StochasticMuZeroModelMLP
    torch.manual_seed(seed)
    m = StochasticMuZeroModelMLP(observation_shape=4, action_space_size=A, chance_space_size=C, latent_state_dim=H,
                                 reward_support_size=2 * scale + 1, value_support_size=2 * scale + 1,
                                 last_linear_layer_init_zero=False, res_connection_in_dynamics=res,
                                 shared_dynamics=shared)
    for bn in (x for x in m.modules() if isinstance(x, torch.nn.BatchNorm1d)):
        bn.running_mean.normal_(0.0, 0.3), bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5), bn.bias.data.normal_(0.0, 0.1)
    return m.to(DEV).eval()


def make_mcts(S, disc, fused, scale):
    from lightzero_amd import StochasticMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    cfg = dict(num_simulations=S, discount_factor=disc, device="cuda",
               model=EasyDict(support_scale=scale, categorical_distribution=True))
    if fused:
        cfg["fused_search"] = True
    mcts = StochasticMuZeroMCTSCtree(EasyDict(cfg))
    mcts.record = True
    return mcts


def search(model, fused, B, S, A, C, H=32, noise=False, legal=None, players=1, disc=0.997, reserve=None, seed=0,
           scale=SCALE, **_):
    """one recorded search through the driver; returns inputs, record, outputs, pool, path and plan"""
    from lightzero_amd.tree import DeviceTree
    rng = np.random.default_rng(seed)
    legal = legal or [list(range(A))] * B
    x = dict(legal=legal, lat=rng.normal(size=(B, H)).astype(np.float32),
             logits=rng.normal(size=(B, A)).astype(np.float32), reward=[0.0] * B,
             to_play=[1 + (i * 7) % 2 for i in range(B)] if players == 2 else [-1] * B,
             noises=[rng.dirichlet([0.3] * len(l)).astype(np.float32).tolist() for l in legal] if noise else None,
             seeds=torch.arange(21, 21 + S, dtype=torch.int32, device=DEV), disc=disc)
    mcts = make_mcts(S, disc, fused, scale)
    roots = mcts.roots(B, legal, C)
    if reserve:
        roots.tree = DeviceTree(B, A, reserve, fast_rng=True, device=DEV, chance=C)
    if noise:
        roots.prepare(0.25, x["noises"], x["reward"], x["logits"].tolist(), x["to_play"])
    else:
        roots.prepare_no_noise(x["reward"], x["logits"].tolist(), x["to_play"])
    mcts.search(roots, model, x["lat"], x["to_play"], seeds=x["seeds"])
    out = dict(x, rec=mcts.last_record.numpy(), is_chance=mcts.last_record.is_chance.cpu().numpy(),
               dist=so.pad(roots.get_distributions(), A), values=np.array(roots.get_values(), np.float32),
               traj=so.pad(roots.get_trajectories(), S + 1), mm=roots._last_minmax.cpu().numpy(),
               pool=mcts._buf.pool.cpu(), path=mcts.last_path, plan=getattr(mcts, "last_plan", None))
    roots.clear()
    return out


@functools.lru_cache(maxsize=None)
def fused_run(shape):
    s = SHAPES[shape]
    model = make_model(s["A"], s["C"], s.get("H", 32), s.get("shared", False), s.get("res", False), 3,
                       s.get("scale", SCALE))
    return dict(search(model, True, seed=sorted(SHAPES).index(shape), **s), model=model)


def expected_plan(s):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = next((r for r in (1, 2, 4) if (s["B"] + r - 1) // r <= cus), 8)
    return dict(roots_per_wg=R, kernel="streaming", mode=0, tree_in_lds=s.get("lds", True))


@pytest.mark.parametrize("shape", SHAPES)
def test_tree_matches_restatement_bit_for_bit(shape):
    s, r = SHAPES[shape], fused_run(shape)
    B, S, A, C, rec = s["B"], s["S"], s["A"], s["C"], r["rec"]
    assert r["path"] == "fused-mlp" and r["plan"] == expected_plan(s)
    assert r["plan"]["roots_per_wg"] == s.get("R", 1), "this B was chosen for that R on a 256-CU device"
    t, mms = so.Tree(r["legal"]), [so.MinMax(0.01) for _ in range(B)]
    t.prepare(0.25, r["noises"], r["reward"], r["logits"], r["to_play"])
    seeds = r["seeds"].cpu().numpy().view(np.uint32)
    for k in range(S):
        out = t.traverse(*PB_C, r["disc"], mms, r["to_play"], *so.philox_draws(seeds[k]))
        for name, got in (("x", rec["x"]), ("a", rec["action"]), ("len", rec["search_len"]), ("vtp", rec["vtp"]),
                          ("is_chance", r["is_chance"])):
            assert np.array_equal(got[k], np.asarray(out[name], np.int32)), (k, name)
        rows = [rec["policy_logits"][k, i, :C if out["is_chance"][i] else A] for i in range(B)]
        assert all(rec["decoded"][k, i, 0] == 0 for i in range(B) if out["is_chance"][i])
        t.backprop(k + 1, r["disc"], rec["decoded"][k, :, 0], rec["decoded"][k, :, 1], rows, mms, out["vtp"])
    assert np.array_equal(r["dist"], so.pad(t.distributions(), A))
    assert np.array_equal(r["traj"], so.pad(t.trajectories(), S + 1))
    assert np.array_equal(bits(r["values"]), bits(t.values()))
    assert np.array_equal(bits(r["mm"][:, 0]), bits([m.mx for m in mms]))
    assert np.array_equal(bits(r["mm"][:, 1]), bits([m.mn for m in mms]))
    assert np.array_equal(r["is_chance"], rec["search_len"] & 1) and (r["is_chance"][0] == 1).all()
    R = r["plan"]["roots_per_wg"]
    if R > 1:  # a mixed case: some workgroup holds both kinds in one simulation
        ch = np.pad(r["is_chance"], ((0, 0), (0, -B % R)), mode="edge").reshape(S, -1, R)
        assert (ch.min(axis=2) != ch.max(axis=2)).any()


def branch_scale(layers, dyn, pred, res, lat, act, A):
    """mlp_numerics.recurrent_scale for one branch of describe_stochastic's layers: (next latent, policy logits)"""
    lin = lambda x, l: F.linear(x, layers[l][0][0].double().abs().cpu(), layers[l][0][1].double().abs().cpu())
    nxt = lin(lin(torch.cat((lat.abs(), F.one_hot(act, A).double()), dim=1), dyn), dyn + 1)
    if res:
        nxt = nxt + lat.abs()
    return nxt, lin(lin(lin(lin(nxt, pred), pred + 1), pred + 4), pred + 5)


@pytest.mark.parametrize("shape", SHAPES)
def test_network_against_float64_through_each_rows_kind(shape):
    from lightzero_amd.fused import describe_stochastic
    s, r = SHAPES[shape], fused_run(shape)
    B, S, A, C, rec, pool = s["B"], s["S"], s["A"], s["C"], r["rec"], r["pool"]
    layers, dims = describe_stochastic(r["model"])
    nd, scale = 4 if dims["res"] else 2, s.get("scale", SCALE)
    m64, m32 = copy.deepcopy(r["model"]).cpu().double().eval(), copy.deepcopy(r["model"]).cpu().float().eval()
    kk, ii = np.nonzero(np.ones((S, B), bool))
    for chance in (1, 0):
        sel = r["is_chance"][kk, ii] == chance
        if not sel.any():
            assert S == 1 and not chance
            continue
        k, i, width = torch.from_numpy(kk[sel]), torch.from_numpy(ii[sel]), C if chance else A
        lat = pool[torch.from_numpy(rec["x"][kk[sel], ii[sel]]).long(), i]
        act = torch.from_numpy(rec["action"][kk[sel], ii[sel]]).long()
        with torch.no_grad():
            ref = m64.recurrent_inference(lat.double(), act, afterstate=not chance)
            f32 = m32.recurrent_inference(lat, act, afterstate=not chance)
        dyn = (0 if dims["shared"] else nd + 14) if chance else 0
        a_lat, a_pol = branch_scale(layers, dyn, nd + 8 if chance else nd + 2, dims["res"], lat.double(), act, A)
        mn.check_scaled(f"stoch {shape} chance={chance}", dict(
            latent=(pool[k + 1, i], ref.latent_state, a_lat, f32.latent_state),
            policy=(torch.from_numpy(rec["policy_logits"])[k, i, :width], ref.policy_logits, a_pol, f32.policy_logits)))
        dec = torch.from_numpy(rec["decoded"])[k, i]
        tol = dict(rtol=1e-4, atol=1e-5 * scale)  # mlp_numerics.check_search_network's
        torch.testing.assert_close(dec[:, 1], mn.inverse_scalar_transform64(ref.value, scale).float(), **tol)
        if not chance:
            torch.testing.assert_close(dec[:, 0], mn.inverse_scalar_transform64(ref.reward, scale).float(), **tol)


def assert_same_search(a, b):
    for n in ("x", "action", "search_len", "vtp"):
        assert np.array_equal(a["rec"][n], b["rec"][n]), n
    assert np.array_equal(a["is_chance"], b["is_chance"]) and np.array_equal(a["dist"], b["dist"])
    # tests/test_gpu_numerics.py's bound
    np.testing.assert_allclose(a["values"], b["values"], rtol=1e-5, atol=1e-5 * SCALE)


def test_one_launch_equals_generic_path():
    """(seed 0 of this shape: no near-tie that network rounding flips on either path)"""
    r = fused_run("a4c2_noise_ragged")
    g = search(r["model"], False, seed=sorted(SHAPES).index("a4c2_noise_ragged"), **SHAPES["a4c2_noise_ragged"])
    assert g["path"] == "generic"
    assert_same_search(r, g)


@pytest.mark.parametrize("why, kw", [("width not a multiple of 16", dict(H=24)), ("actions > hidden", dict(A=20, H=16))])
def test_refused_shapes_fall_back_to_the_generic_path(why, kw):
    s = dict(dict(B=4, S=4, A=4, C=2), **kw)
    model = make_model(s["A"], s["C"], s["H"], False, False, 5)
    f, g = search(model, True, **s), search(model, False, **s)
    assert f["path"] == "generic" and g["path"] == "generic"
    assert_same_search(f, g)
    assert np.array_equal(bits(f["values"]), bits(g["values"]))
