"""CPU: EfficientZeroModelMLP and its packer for the one-launch search (lightzero_amd/fused.py describe_ez /
pack_efficientzero_mlp, lzm_search_mlp_ez).

1. The module against a plain restatement built from its own tensors (F.linear, eval BatchNorm, ReLU,
   nn.LSTMCell with the LSTM's weights) in float64: 1e-12.
2. describe_ez's folded layers — BatchNorm folded, the LSTM as one dense gate layer over [x ; h_prev] with the two
   biases summed — evaluated in float64 numpy against the module: 1e-12.
3. The packed size is the library's (lzm_mlp_ez_packed_floats); what the packer refuses; the shape query.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from lightzero_amd import _lib
from lightzero_amd.fused import NotPackable, describe_ez, pack_efficientzero_mlp
from lightzero_amd.model_mlp import (EfficientZeroModelMLP, MuZeroModelMLP, cartpole_efficientzero_model)

TOL = 1e-12
H, HL, A, V, FH = 48, 32, 3, 21, 16  # LSTM width != latent width


def make_model(res, seed=0, **kw):
    torch.manual_seed(seed)
    args = dict(observation_shape=4, action_space_size=A, lstm_hidden_size=HL, latent_state_dim=H,
                fc_reward_layers=(FH,), fc_value_layers=(FH,), fc_policy_layers=(FH,), reward_support_size=V,
                value_support_size=V, last_linear_layer_init_zero=False, res_connection_in_dynamics=res)
    args.update(kw)
    m = EfficientZeroModelMLP(**args)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm1d):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.double().eval()


def inputs(n=7, seed=3):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(n, H, generator=g, dtype=torch.float64)
    h0 = torch.randn(1, n, HL, generator=g, dtype=torch.float64) * 0.5
    c0 = torch.randn(1, n, HL, generator=g, dtype=torch.float64) * 0.5
    act = torch.randint(0, A, (n,), generator=g)
    return lat, (h0, c0), act


def plain_seq(seq, x):
    for m in seq:
        if isinstance(m, nn.Linear):
            x = F.linear(x, m.weight, m.bias)
        elif isinstance(m, nn.BatchNorm1d):
            x = (x - m.running_mean) / torch.sqrt(m.running_var + m.eps) * m.weight + m.bias
        else:
            assert isinstance(m, nn.ReLU), type(m)
            x = torch.relu(x)
    return x


@pytest.mark.parametrize("res", [False, True])
def test_module_matches_lstmcell_restatement(res):
    m = make_model(res)
    lat, (h0, c0), act = inputs()
    dyn, pred = m.dynamics_network, m.prediction_network
    with torch.no_grad():
        out = m.recurrent_inference(lat, (h0, c0), act)
        x = torch.cat((lat, F.one_hot(act, A).double()), dim=1)
        if res:
            nxt = plain_seq(dyn.fc_dynamics_1, x) + lat
            xin = plain_seq(dyn.fc_dynamics_2, nxt)
        else:
            nxt = xin = plain_seq(dyn.fc_dynamics, x)
        cell = nn.LSTMCell(H, HL).double()
        cell.weight_ih.copy_(dyn.lstm.weight_ih_l0)
        cell.weight_hh.copy_(dyn.lstm.weight_hh_l0)
        cell.bias_ih.copy_(dyn.lstm.bias_ih_l0)
        cell.bias_hh.copy_(dyn.lstm.bias_hh_l0)
        h1, c1 = cell(xin, (h0[0], c0[0]))
        vp = plain_seq(dyn.fc_reward_head, h1)
        p = plain_seq(pred.fc_prediction_common, nxt)
        value, policy = plain_seq(pred.fc_value_head, p), plain_seq(pred.fc_policy_head, p)
    for got, ref in ((out.latent_state, nxt), (out.value_prefix, vp), (out.value, value), (out.policy_logits, policy),
                     (out.reward_hidden_state[0][0], h1), (out.reward_hidden_state[1][0], c1)):
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= TOL
    assert out.reward_hidden_state[0].shape == (1, lat.shape[0], HL)


def test_initial_inference_state_and_value_prefix():
    m = make_model(False)
    with torch.no_grad():
        out = m.initial_inference(torch.randn(5, 4, dtype=torch.float64))
    assert out.value_prefix == [0.] * 5
    for s in out.reward_hidden_state:
        assert s.shape == (1, 5, HL) and not s.any()
    assert out.latent_state.shape == (5, H) and out.policy_logits.shape == (5, A) and out.value.shape == (5, V)


def test_cartpole_model_is_the_zoo_config():
    m = cartpole_efficientzero_model()
    _, dims = describe_ez(m.eval())
    assert dims == dict(hidden=128, actions=2, head_hidden=32, support=601, res=False, lstm_hidden=128)
    assert m.representation_network.fc_representation[0].in_features == 4
    assert m.dynamics_network.fc_reward_head[-1].weight.abs().sum() > 0  # random_heads
    assert cartpole_efficientzero_model(random_heads=False).prediction_network.fc_value_head[-1].weight.abs().sum() == 0


@pytest.mark.parametrize("res", [False, True])
def test_packed_layers_match_module(res):
    m = make_model(res)
    lat, (h0, c0), act = inputs()
    layers, dims = describe_ez(m, dtype=torch.float64)
    assert dims == dict(hidden=H, actions=A, head_hidden=FH, support=V, res=res, lstm_hidden=HL)
    L = [(w.numpy(), b.numpy(), relu) for (w, b), relu in layers]
    assert len(L) == (13 if res else 11)

    def dense(x, l):
        w, b, relu = L[l]
        y = x @ w.T + b
        return np.maximum(y, 0.0) if relu else y
    x = np.concatenate((lat.numpy(), np.eye(A)[act.numpy()]), axis=1)
    nxt = dense(dense(x, 0), 1)
    o = 2
    xin = nxt
    if res:
        nxt = nxt + lat.numpy()
        xin = dense(dense(nxt, 2), 3)
        o = 4
    w, b, relu = L[o]
    assert w.shape == (4 * HL, H + HL) and b.shape == (4 * HL,) and not relu
    gates = dense(np.concatenate((xin, h0[0].numpy()), axis=1), o)
    gi, gf, gg, go = np.split(gates, 4, axis=1)  # nn.LSTM's order
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    c1 = sig(gf) * c0[0].numpy() + sig(gi) * np.tanh(gg)
    h1 = sig(go) * np.tanh(c1)
    vp = dense(dense(h1, o + 1), o + 2)
    p = dense(dense(nxt, o + 3), o + 4)
    value, policy = dense(dense(p, o + 5), o + 6), dense(dense(p, o + 7), o + 8)
    with torch.no_grad():
        out = m.recurrent_inference(lat, (h0, c0), act)
    for got, ref in ((nxt, out.latent_state), (vp, out.value_prefix), (value, out.value), (policy, out.policy_logits),
                     (h1, out.reward_hidden_state[0][0]), (c1, out.reward_hidden_state[1][0])):
        assert np.abs(got - ref.numpy()).max() <= TOL
    # the summed bias is the float64 sum of the two, then cast (what the float32 packer files)
    lstm = m.dynamics_network.lstm
    b32 = describe_ez(m)[0][o][0][1]
    assert b32.dtype == torch.float32
    assert torch.equal(b32, (lstm.bias_ih_l0.double() + lstm.bias_hh_l0.double()).float())


@pytest.mark.parametrize("res", [False, True])
def test_packed_size_is_the_librarys(res):
    m = make_model(res).float()
    flat, dims = pack_efficientzero_mlp(m, torch.device("cpu"))
    n = _lib.load().lzm_mlp_ez_packed_floats(H, HL, A, FH, V, int(res))
    assert flat.dtype == torch.float32 and flat.numel() == n
    layers, _ = describe_ez(m)
    assert n == sum(w.numel() + b.numel() for (w, b), _ in layers)
    assert _lib.load().lzm_mlp_ez_kernel_floats(H, HL, A, FH, V, int(res)) >= n
    # the first layer as packed: W[K][N] (torch's weight transposed), then its bias
    (w0, b0), _ = layers[0]
    assert torch.equal(flat[:w0.numel()].reshape(H + A, H), w0.t())
    assert torch.equal(flat[w0.numel():w0.numel() + H], b0)


def test_refusals():
    with pytest.raises(NotPackable):
        describe_ez(make_model(False, state_norm=True))
    with pytest.raises(NotPackable):
        describe_ez(make_model(False, discrete_action_encoding_type='not_one_hot'))
    two = make_model(False)
    two.dynamics_network.lstm = nn.LSTM(H, HL, num_layers=2).double()
    with pytest.raises(NotPackable):
        describe_ez(two)
    bi = make_model(False)
    bi.dynamics_network.lstm = nn.LSTM(H, HL, bidirectional=True).double()
    with pytest.raises(NotPackable):
        describe_ez(bi)
    nob = make_model(False)
    nob.dynamics_network.lstm = nn.LSTM(H, HL, bias=False).double()
    with pytest.raises(NotPackable):
        describe_ez(nob)
    with pytest.raises(NotPackable):
        describe_ez(make_model(False).train())
    with pytest.raises(NotPackable):
        describe_ez(MuZeroModelMLP(observation_shape=4, action_space_size=A, latent_state_dim=H).eval())
    with pytest.raises(NotPackable):  # a width the kernel refuses (the library is asked)
        pack_efficientzero_mlp(make_model(False, lstm_hidden_size=72).float(), torch.device("cpu"))


def test_shape_query():
    L = _lib.load()
    assert L.lzm_search_mlp_ez_supported(2, 128, 128, 32, 601) == 1   # the zoo config
    assert L.lzm_search_mlp_ez_supported(6, 256, 512, 32, 601) == 1   # the model's defaults
    assert L.lzm_search_mlp_ez_supported(2, 128, 72, 32, 601) == 0    # not a multiple of 16
    assert L.lzm_search_mlp_ez_supported(24, 128, 128, 32, 1001) == 0  # support + actions > 1024
    assert L.lzm_search_mlp_ez_supported(2, 128, 1024, 32, 601) == 0  # past four gate column rounds
    assert L.lzm_mlp_ez_packed_floats(0, 128, 2, 32, 601, 0) == -1
