"""GPU: the one-launch Sampled EfficientZero search (lzm_search_mlp_sampled: search_sampled_mlp_kernel<R, TL>) behind
SampledEfficientZeroMCTSCtree with cfg.fused_search set, over the continuous SampledEfficientZeroModelMLP.

Tree: the host restatement tests/sampled_oracle.py, fed the decoded value prefix / value and the {mu, sigma} row the
kernel recorded, under the same Philox seeds — no tolerance, but one float32 ulp on the sampled actions (both sides
round a double result to float). Network: float64 on the recorded inputs within tests/mlp_numerics.py's
bounds; sigma, which passes through exp, within twice the float32 torch module's relative error on the same rows
(tests/test_gpu_split_range.py's margin).
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mlp_numerics as mn  # noqa: E402
import sampled_oracle as so  # noqa: E402
from test_gpu_sampled import bits, same_actions  # noqa: E402

DEV = torch.device("cuda", 0)
SCALE, ROOT_SEED = 10, 77  # support 21
# B, S, K, D and the options; lds: whether the reserved tree slice fits LDS; R: roots per workgroup the plan must pick at that B on a 256-CU device
SHAPES = {
    "k1_d1_deep": dict(B=5, S=12, K=1, D=1),
    "k2_d3_clamp": dict(B=5, S=12, K=2, D=3, clamp=True),
    "k20_d6_tanh_res": dict(B=5, S=12, K=20, D=6, tanh=True, res=True),
    "k64_d32": dict(B=5, S=12, K=64, D=32, H=64, lds=False),  # (the default reserve of 64 simulations x 64 slots)
    "s1": dict(B=5, S=1, K=20, D=6),
    "s2_fixed": dict(B=5, S=2, K=2, D=3, sigma="fixed"),
    "b1_disc1": dict(B=1, S=12, K=2, D=3, disc=1.0),
    "b259_r2_2p": dict(B=259, S=5, K=2, D=3, R=2, players=2),
    "b515_r4": dict(B=515, S=5, K=20, D=6, R=4, res=True, lds=False),  # (four roots' default reserve x 20 slots)
    "reserved_800_hbm": dict(B=5, S=12, K=20, D=6, reserve=800, lds=False),
    "zoo_256_v601": dict(B=5, S=8, K=20, D=4, H=256, Hl=256, res=True, scale=300),
}


def make_model(D, H=32, Hl=16, res=False, tanh=False, sigma="conditioned", clamp=False, scale=SCALE, seed=3,
               continuous=True, K=20):
    from lightzero_amd.model_mlp import SampledEfficientZeroModelMLP
    torch.manual_seed(seed)
    m = SampledEfficientZeroModelMLP(observation_shape=4, action_space_size=D, lstm_hidden_size=Hl, latent_state_dim=H,
                                     reward_support_size=2 * scale + 1, value_support_size=2 * scale + 1,
                                     last_linear_layer_init_zero=False, res_connection_in_dynamics=res,
                                     continuous_action_space=continuous, num_of_sampled_actions=K, sigma_type=sigma,
                                     bound_type="tanh" if tanh else None)
    for bn in (x for x in m.modules() if isinstance(x, torch.nn.BatchNorm1d)):
        bn.running_mean.normal_(0.0, 0.3), bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5), bn.bias.data.normal_(0.0, 0.1)
    if clamp:  # log_sigma of dimension 0 past the upper clamp end, of dimension 1 past the lower one, in every row
        m.prediction_network.fc_policy_head.log_sigma_layer.bias.data[:2] = torch.tensor([30.0, -30.0])
    return m.to(DEV).eval()


def search(model, fused, B, S, K, D, H=32, Hl=16, players=1, disc=so.DISC, reserve=None, seed=0, scale=SCALE,
           cont=True, graph=False, **_):
    """one search through the driver (recorded unless replayed as a graph); returns inputs, record, outputs, plan"""
    from lightzero_amd import SampledEfficientZeroMCTSCtree
    from lightzero_amd.tree import DeviceTree
    from lightzero_amd.utils import EasyDict
    rng = np.random.default_rng(seed)
    pol = (np.concatenate([rng.uniform(-1, 1, (B, D)), rng.uniform(0.2, 1.5, (B, D))], 1) if cont
           else rng.normal(size=(B, D))).astype(np.float32)
    x = dict(lat=rng.normal(size=(B, H)).astype(np.float32), pol=pol,
             hidden=tuple(rng.normal(0.0, 0.3, size=(1, B, Hl)).astype(np.float32) for _ in range(2)),
             to_play=[1 + (i * 7) % 2 for i in range(B)] if players == 2 else [-1] * B,
             seeds=torch.arange(21, 21 + S, dtype=torch.int32, device=DEV), disc=disc)
    cfg = dict(num_simulations=S, discount_factor=disc, device="cuda", lstm_horizon_len=so.HORIZON, use_hip_graph=graph,
               model=EasyDict(support_scale=scale, categorical_distribution=True, continuous_action_space=cont))
    if fused:
        cfg["fused_search"] = True
    mcts = SampledEfficientZeroMCTSCtree(EasyDict(cfg))
    mcts.record = not graph
    roots = mcts.roots(B, [[-1]] * B, D, K, cont)
    if reserve:
        roots.tree = DeviceTree(B, D, reserve, fast_rng=True, device=DEV, sampled=K, continuous=True)
    for _ in range(2 if graph else 1):  # (a graph: its capture's first replay, then a replay of the cached graph)
        roots.prepare_no_noise([0.0] * B, pol.tolist(), x["to_play"], seed=ROOT_SEED)
        mcts.search(roots, model, x["lat"], x["hidden"], x["to_play"], seeds=x["seeds"])
    out = dict(x, dist=np.array(roots.get_distributions(), np.int32), values=np.array(roots.get_values(), np.float32),
               traj=roots.get_trajectories(), sampled=np.array(roots.get_sampled_actions(), np.float32),
               mm=roots._last_minmax.cpu().numpy(), path=mcts.last_path, plan=getattr(mcts, "last_plan", None))
    if mcts.record:
        r = mcts.last_record
        out.update(rec=r.numpy(), is_reset=r.is_reset.cpu().numpy(), actions=r.last_actions.cpu().numpy(),
                   pool=mcts._buf.pool.cpu(), hpool=mcts._buf.extra[0].cpu(), cpool=mcts._buf.extra[1].cpu())
    roots.clear()
    return out


def model_of(s):
    return make_model(s["D"], s.get("H", 32), s.get("Hl", 16), s.get("res", False), s.get("tanh", False),
                      s.get("sigma", "conditioned"), s.get("clamp", False), s.get("scale", SCALE), K=s["K"])


@functools.lru_cache(maxsize=None)
def fused_run(shape):
    s = SHAPES[shape]
    model = model_of(s)
    return dict(search(model, True, seed=sorted(SHAPES).index(shape), **s), model=model)


@pytest.mark.parametrize("shape", SHAPES)
def test_tree_matches_restatement_bit_for_bit(shape, monkeypatch):
    s, r = SHAPES[shape], fused_run(shape)
    B, S, K, D, rec = s["B"], s["S"], s["K"], s["D"], r["rec"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = next((q for q in (1, 2) if (B + q - 1) // q <= cus), 4)
    assert r["path"] == "fused-mlp"
    assert r["plan"] == dict(roots_per_wg=R, kernel="streaming", mode=0, tree_in_lds=s.get("lds", True))
    assert R == s.get("R", 1), "this B was chosen for that R on a 256-CU device"
    mms = []
    monkeypatch.setattr(so, "DISC", r["disc"])
    monkeypatch.setattr(so, "MinMax", lambda delta, cls=so.MinMax: mms.append(cls(delta)) or mms[-1])
    seeds = r["seeds"].cpu().numpy().view(np.uint32)
    g = dict(to_play=np.array(r["to_play"], np.int32), root_vp=np.zeros(B, np.float32), root_policy=r["pol"],
             resp_vp=rec["decoded"][..., 0], resp_value=rec["decoded"][..., 1], resp_policy=rec["policy_logits"],
             meta=np.array([B, S, K, D, 1], np.int64))
    want = so.replay(g, lambda k: so.philox_draws(seeds[k]),
                     lambda k: so.philox_sampler(ROOT_SEED if k < 0 else seeds[k], K, True))
    for name, got in (("req_x", rec["x"]), ("req_slot", rec["action"]), ("req_len", rec["search_len"]),
                      ("out_dist", r["dist"])):
        assert np.array_equal(got, want[name]), name
    assert np.array_equal(r["is_reset"], (rec["search_len"] % so.HORIZON == 0).astype(np.int32))
    assert r["traj"] == want["traj"]
    assert np.array_equal(bits(r["values"]), bits(want["out_values"]))
    assert np.array_equal(bits(r["mm"][:, 0]), bits([m.mx for m in mms]))
    assert np.array_equal(bits(r["mm"][:, 1]), bits([m.mn for m in mms]))
    assert same_actions(r["actions"], want["req_action"], True)
    assert same_actions(r["sampled"], want["root_actions"], True)
    if K == 1:  # a path as deep as the search, the reset crossed
        assert rec["search_len"].max() == S and (r["is_reset"].any() and not r["is_reset"].all()) == (S > so.HORIZON)


def scales(layers, dims, lat, h0, c0, act):
    """A of (next latent, the cell, mu) for recurrent_inference(lat, (h0, c0), act) over describe_sampled's layers:
    every weight, bias and input by its absolute value, every activation the identity (tests/mlp_numerics.py)"""
    W = [(w.double().abs().cpu(), b.double().abs().cpu()) for (w, b), _ in layers]
    lin = lambda x, l: F.linear(x, W[l][0], W[l][1])
    nxt = lin(lin(torch.cat((lat.abs(), act.abs()), dim=1), 0), 1)
    o, xin = 2, nxt
    if dims["res"]:
        nxt = nxt + lat.abs()
        xin, o = lin(lin(nxt, 2), 3), 4
    cell = torch.stack(lin(torch.cat((xin, h0.abs()), dim=1), o).chunk(4, dim=1)).amax(dim=0) * (1 + c0.abs())
    main = lin(lin(lin(lin(nxt, o + 3), o + 4), o + 5)[:, dims["head_hidden"]:], o + 6)
    V, D = dims["support"], dims["dim"]
    return nxt, cell, lin(F.pad(main, (0, W[o + 7][0].shape[1] - main.shape[1])), o + 7)[:, V:V + D]


@pytest.mark.parametrize("shape", SHAPES)
def test_network_against_float64(shape):
    from lightzero_amd.fused import describe_sampled
    s, r = SHAPES[shape], fused_run(shape)
    B, S, D, rec, scale = s["B"], s["S"], s["D"], r["rec"], s.get("scale", SCALE)
    x, idx = torch.from_numpy(rec["x"]).long(), torch.arange(B)
    gat = lambda p: torch.stack([p[x[k], idx] for k in range(S)]).reshape(S * B, -1)
    lat, h0, c0 = gat(r["pool"]), gat(r["hpool"]), gat(r["cpool"])
    act = torch.from_numpy(r["actions"]).reshape(S * B, D)
    layers, dims = describe_sampled(r["model"])
    with torch.no_grad():
        m64, m32 = copy.deepcopy(r["model"]).cpu().double().eval(), copy.deepcopy(r["model"]).cpu().float().eval()
        ref = m64.recurrent_inference(lat.double(), (h0.double().unsqueeze(0), c0.double().unsqueeze(0)), act.double())
        f32 = m32.recurrent_inference(lat, (h0.unsqueeze(0), c0.unsqueeze(0)), act)
        a_lat, a_cell, a_mu = scales(layers, dims, lat.double(), h0.double(), c0.double(), act.double())
    keep = torch.from_numpy(r["is_reset"]).reshape(S * B) == 0
    h1, c1 = r["hpool"][1:S + 1].reshape(S * B, -1), r["cpool"][1:S + 1].reshape(S * B, -1)
    assert not h1[~keep].any() and not c1[~keep].any(), "reset rows of the state pools must be exactly 0"
    (rh, rc), (fh, fc) = (q.reward_hidden_state for q in (ref, f32))
    pol = torch.from_numpy(rec["policy_logits"]).reshape(S * B, 2 * D)
    mn.check_scaled(f"sampled {shape}", dict(
        latent=(r["pool"][1:S + 1].reshape(S * B, -1), ref.latent_state, a_lat, f32.latent_state),
        h1=(h1[keep], rh[0][keep], a_cell[keep], fh[0][keep]), c1=(c1[keep], rc[0][keep], a_cell[keep], fc[0][keep]),
        mu=(pol[:, :D], ref.policy_logits[:, :D], a_mu, f32.policy_logits[:, :D])))
    dec = torch.from_numpy(rec["decoded"]).reshape(S * B, 2)
    tol = dict(rtol=1e-4, atol=1e-5 * scale)  # mlp_numerics.check_search_network's
    torch.testing.assert_close(dec[:, 0], mn.inverse_scalar_transform64(ref.value_prefix, scale).float(), **tol)
    torch.testing.assert_close(dec[:, 1], mn.inverse_scalar_transform64(ref.value, scale).float(), **tol)
    sig = ref.policy_logits[:, D:]
    rel = lambda got: float(((got.double() - sig).abs() / sig).max())
    print(f"sampled {shape}: sigma max relative error, kernel {rel(pol[:, D:]):.3e} vs torch f32 "
          f"{rel(f32.policy_logits[:, D:]):.3e}")
    if s.get("sigma") == "fixed":
        # the module's row is the constant itself (error 0): the kernel's is exp of the float32 log of it, off by the
        # rounding of log(0.3) (|log| 2^-24 in the exponent) and one expf ulp: under 2^-22 relative
        assert rel(pol[:, D:]) <= 2.0 ** -22
    else:
        assert rel(pol[:, D:]) <= 2 * rel(f32.policy_logits[:, D:])
    if s.get("clamp"):
        assert np.allclose(sig[:, :2].numpy(), [np.exp(2.0), np.exp(-20.0)], rtol=1e-12)


def assert_same_search(a, b, requests=True):
    for n in ("x", "action", "search_len") if requests else ():
        assert np.array_equal(a["rec"][n], b["rec"][n]), n
    assert np.array_equal(a["dist"], b["dist"]) and a["traj"] == b["traj"]
    # tests/test_gpu_numerics.py's bound
    np.testing.assert_allclose(a["values"], b["values"], rtol=1e-5, atol=1e-5 * SCALE)


def test_one_launch_equals_generic_path():
    """(this model and seed: the generic path, eager and replayed as a graph, agrees with itself, so no near-tie
    that network rounding flips)"""
    name = "k20_d6_tanh_res"
    s, r = SHAPES[name], fused_run(name)
    kw = dict(s, seed=sorted(SHAPES).index(name))
    eager, graph = search(r["model"], False, **kw), search(r["model"], False, graph=True, **kw)
    assert eager["path"] == "generic" and graph["path"] == "generic" and r["path"] == "fused-mlp"
    assert_same_search(eager, graph, requests=False)
    assert np.array_equal(bits(eager["values"]), bits(graph["values"]))
    assert_same_search(r, eager)
    assert same_actions(r["sampled"], eager["sampled"], True)


@pytest.mark.parametrize("why, kw", [
    ("a discrete model", dict(D=6, K=3, cont=False)), ("sigma_type 'independent'", dict(sigma="independent")),
    ("an LSTM width of 24", dict(Hl=24)), ("D = 33", dict(D=33, H=48))])
def test_refusals_fall_back_to_the_generic_path(why, kw):
    s = dict(dict(B=4, S=4, K=3, D=3, H=32, Hl=16), **kw)
    if s["D"] > 32:  # (the tree refuses the handle itself: no path runs such a search)
        from lightzero_amd.fused import NotPackable, describe_sampled
        with pytest.raises(NotPackable, match="kSampledMaxDim"):
            describe_sampled(make_model(s["D"], s["H"], s["Hl"]))
        return
    model = make_model(s["D"], s["H"], s["Hl"], sigma=s.get("sigma", "conditioned"), continuous=s.get("cont", True),
                       K=s["K"], seed=5)
    f, g = search(model, True, **s), search(model, False, **s)
    assert f["path"] == "generic" and g["path"] == "generic"
    assert_same_search(f, g)
    assert np.array_equal(bits(f["values"]), bits(g["values"])) and np.array_equal(bits(f["sampled"]), bits(g["sampled"]))


def test_a_muzero_handle_is_refused_before_any_launch():
    from lightzero_amd import _lib
    from lightzero_amd.tree import DeviceTree
    t, z = DeviceTree(4, 3, 8, fast_rng=True, device=DEV), torch.zeros(4096, device=DEV)
    p = _lib.ptr(z)
    rc = _lib.load().lzm_search_mlp_sampled(t.h, 32, 16, 32, 21, 0, 0, p, 4, 5, 19652, 1.25, 0.997, p, p, p, p, p, p,
                                            *([None] * 7), None)
    assert rc == _lib.LZM_ERR_STATE
    t.close()
