"""GPU: the conv StochasticMuZeroModel's recurrent step as one launch per simulation (lzm_smz_conv_net_step:
smz_conv_step_kernel<NRES, P>) — against the module in float64 through each row's kind, its bits across batch
layouts, and behind StochasticMuZeroMCTSCtree with cfg.native_network against tests/stochastic_oracle.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

import stochastic_oracle as so  # noqa: E402
from test_gpu_stochastic import PB_C, bits  # noqa: E402
from test_stochastic_conv_pack import boards, make_model  # noqa: E402

DEV = torch.device("cuda", 0)
NAMES = ("latent", "value", "reward", "policy_d", "policy_c")


def inputs(m, net, B, seed=1):
    """B rows of alternating kinds (row 0 a chance leaf): non-negative latents, options, kinds"""
    kind = (torch.arange(B) + 1) % 2
    opt = torch.where(kind.bool(), torch.arange(B) % net.dims["A"], torch.arange(B) % net.dims["C"])
    with torch.no_grad():
        return m.representation_network(boards(B, seed)), opt, kind


def net_step(net, lat, opt, kind, P):
    """one step over the rows, read from pool slot 1; the outputs by name"""
    B = lat.shape[0]
    pool = torch.zeros(2, B, 64, 4, 4, device=DEV)
    pool[1] = lat.to(DEV)
    out = net.outputs(B)
    i32 = lambda t: t.to(device=DEV, dtype=torch.int32)
    net.step(pool, i32(torch.ones(B)), i32(opt), i32(kind), *out, positions=P)
    return dict(zip(NAMES, (o.cpu() for o in out)))


@pytest.mark.parametrize("A,C,V", [(4, 32, 601), (64, 2, 21)])
@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("P", [1, 2])
def test_step_matches_torch_float64(P, nres, A, C, V):
    """B = 5 rows of alternating kinds (P = 2: mixed workgroups and a ragged last one) against a float64 copy of the
    module on the CPU, per row through its kind: |got - ref| <= 2e-5 + 2e-4 |ref|, and the maximum / 99th-percentile
    absolute error at most 4x / 2x those of the same module on the CPU in float32 (floor 2e-5).
    Measured on an MI355X, worst row over the parametrisation, |err| p99 / max (the float32 module beside it):
      next latent 1.888e-07 / 4.609e-07 (1.084e-07 / 2.144e-07), value 4.952e-08 / 6.867e-08 (3.889e-08 / 4.686e-08),
      reward 4.656e-08 / 7.805e-08 (2.803e-08 / 3.857e-08), policy [A] 6.763e-08 / 7.767e-08 (4.841e-08 / 4.872e-08),
      chance logits [C] 6.333e-08 / 7.243e-08 (3.473e-08 / 3.601e-08)."""
    from lightzero_amd.conv_infer import StochasticConvNet
    m = make_model(nres, A, C, V)
    net = StochasticConvNet(m, DEV)
    lat, opt, kind = inputs(m, net, 5)
    got = net_step(net, lat, opt, kind, P)
    m64 = copy.deepcopy(m).double()
    for i in range(5):
        ch = bool(kind[i])
        with torch.no_grad():
            want = m64.recurrent_inference(lat[i:i + 1].double(), opt[i:i + 1], afterstate=not ch)
            f32 = m.recurrent_inference(lat[i:i + 1], opt[i:i + 1], afterstate=not ch)
        rows = [("latent", "latent_state"), ("value", "value"), ("policy_c" if ch else "policy_d", "policy_logits")]
        for name, attr in rows + ([] if ch else [("reward", "reward")]):
            w = getattr(want, attr).reshape(-1)
            err, e32 = (got[name][i].double().reshape(-1) - w).abs(), (getattr(f32, attr).double().reshape(-1) - w).abs()
            q = [float(torch.quantile(err, z)) for z in (0.99, 1.0)]
            q32 = [float(torch.quantile(e32, z)) for z in (0.99, 1.0)]
            print(f"smz conv P {P} nres {nres} row {i} {name}: |err| p99 / max = {q[0]:.3e} / {q[1]:.3e} "
                  f"(torch CPU float32: {q32[0]:.3e} / {q32[1]:.3e}); max |ref| {float(w.abs().max()):.3e}")
            assert torch.isfinite(got[name][i]).all()
            assert bool((err <= 2e-5 + 2e-4 * w.abs()).all()), (i, name, float((err - 2e-4 * w.abs()).max()))
            assert q[1] <= max(2e-5, 4 * q32[1]) and q[0] <= max(2e-5, 2 * q32[0]), (i, name, q, q32)


@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("P", [1, 2])
def test_step_bits_do_not_depend_on_the_batch(P, nres):
    """five rows alone, then as rows 0, 3, 10, 21 and 36 of a B = 37 call (first and second position of a P = 2
    workgroup, the ragged last one), each beside a neighbour of the other kind, with P and with the other P:
    byte-identical"""
    from lightzero_amd.conv_infer import StochasticConvNet
    m = make_model(nres, 4, 32, 21)
    net = StochasticConvNet(m, DEV)
    lat, opt, kind = inputs(m, net, 5)
    alone = net_step(net, lat, opt, kind, P)
    blat, bopt, bkind = inputs(m, net, 37, seed=9)
    at = torch.tensor([0, 3, 10, 21, 36])
    blat[at], bopt[at], bkind[at] = lat, opt, kind
    bkind[at[:4] ^ 1] = 1 - kind[:4]
    bopt[at[:4] ^ 1] = 0
    for big in (net_step(net, blat, bopt, bkind, P), net_step(net, blat, bopt, bkind, 3 - P)):
        for name in NAMES:
            rows = [i for i in range(5) if name in ("latent", "value") or bool(kind[i]) == (name == "policy_c")]
            assert rows and torch.equal(big[name][at[rows]].view(torch.int32), alone[name][rows].view(torch.int32)), name


def search(m, B, S, A, C, graph, native=True, scale=10):
    from lightzero_amd import StochasticMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    rng = np.random.default_rng(B)
    legal = [list(range(A))] * B
    x = dict(legal=legal, logits=rng.normal(size=(B, A)).astype(np.float32), reward=[0.0] * B,
             to_play=[1 + (i * 7) % 2 for i in range(B)],
             noises=[rng.dirichlet([0.3] * A).astype(np.float32).tolist() for _ in legal],
             seeds=torch.arange(21, 21 + S, dtype=torch.int32, device=DEV))
    mcts = StochasticMuZeroMCTSCtree(EasyDict(dict(
        num_simulations=S, discount_factor=0.997, device="cuda", native_network=native, use_hip_graph=graph,
        model=EasyDict(support_scale=scale, categorical_distribution=True))))
    mcts.record = not graph
    roots = mcts.roots(B, legal, C)
    roots.prepare(0.25, x["noises"], x["reward"], x["logits"].tolist(), x["to_play"])
    with torch.no_grad():
        lat = m.representation_network(boards(B, 5).to(DEV))
    mcts.search(roots, m, lat, x["to_play"], seeds=x["seeds"])
    out = dict(x, dist=so.pad(roots.get_distributions(), A), values=np.array(roots.get_values(), np.float32),
               traj=so.pad(roots.get_trajectories(), S + 1), mm=roots._last_minmax.cpu().numpy(), path=mcts.last_path)
    if mcts.record:
        out.update(rec=mcts.last_record.numpy(), is_chance=mcts.last_record.is_chance.cpu().numpy())
    roots.clear()
    return out


@pytest.mark.parametrize("A,C", [(4, 32), (3, 5)])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nres", [1, 2])
@pytest.mark.parametrize("P", [1, 2])
def test_search_matches_restatement_bit_for_bit(monkeypatch, P, nres, B, A, C):
    """cfg.native_network, S = 12, two players, root noise: requests, leaf kinds, visit counts, trajectories and
    root-value bits against tests/stochastic_oracle.py fed the recorded decoded scalars and policy rows; eager and
    one HIP graph give identical arrays; both kinds occur among the leaves"""
    monkeypatch.setenv("LZM_SMZ_CONV_POSITIONS", str(P))
    S, m = 12, make_model(nres, A, C, 21, seed=2).to(DEV)
    r = search(m, B, S, A, C, graph=False)
    assert r["path"] == "native-conv"
    rec = r["rec"]
    t, mms = so.Tree(r["legal"]), [so.MinMax(0.01) for _ in range(B)]
    t.prepare(0.25, r["noises"], r["reward"], r["logits"], r["to_play"])
    seeds = r["seeds"].cpu().numpy().view(np.uint32)
    for k in range(S):
        out = t.traverse(*PB_C, 0.997, mms, r["to_play"], *so.philox_draws(seeds[k]))
        for name, got in (("x", rec["x"]), ("a", rec["action"]), ("len", rec["search_len"]), ("vtp", rec["vtp"]),
                          ("is_chance", r["is_chance"])):
            assert np.array_equal(got[k], np.asarray(out[name], np.int32)), (k, name)
        rows = [rec["policy_logits"][k, i, :C if out["is_chance"][i] else A] for i in range(B)]
        assert all(not rec["policy_logits"][k, i, len(rows[i]):].any() for i in range(B))
        t.backprop(k + 1, 0.997, rec["decoded"][k, :, 0], rec["decoded"][k, :, 1], rows, mms, out["vtp"])
    assert set(np.unique(r["is_chance"])) == {0, 1}
    assert np.array_equal(r["dist"], so.pad(t.distributions(), A))
    assert np.array_equal(r["traj"], so.pad(t.trajectories(), S + 1))
    assert np.array_equal(bits(r["values"]), bits(t.values()))
    g = search(m, B, S, A, C, graph=True)
    assert g["path"] == "native-conv"
    for name in ("dist", "traj", "values", "mm"):
        assert np.array_equal(bits(g[name]) if g[name].dtype == np.float32 else g[name],
                              bits(r[name]) if r[name].dtype == np.float32 else r[name]), name


def test_refused_model_takes_the_generic_path():
    m = make_model(1, 4, 32, 21, num_channels=32).to(DEV)  # (a width the kernel does not take)
    assert search(m, 2, 3, 4, 32, graph=False)["path"] == "generic"
