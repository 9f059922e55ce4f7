"""CPU: fused.describe_sampled / pack_sampled_efficientzero_mlp over the continuous SampledEfficientZeroModelMLP — the
packed size against the library's, the merged tail's layer order, the fixed sigma, the refusals with their reasons,
and the restated model against a hand-written float64 forward of the same parameters (host only)."""
import math

import pytest
import torch
import torch.nn.functional as F

from lightzero_amd import _lib
from lightzero_amd.fused import NotPackable, describe_sampled, pack_sampled_efficientzero_mlp
from lightzero_amd.model_mlp import SampledEfficientZeroModelMLP


def model(D=3, H=32, Hl=16, V=21, **kw):
    torch.manual_seed(1)
    kw = dict(dict(continuous_action_space=True, last_linear_layer_init_zero=False), **kw)
    return SampledEfficientZeroModelMLP(observation_shape=5, action_space_size=D, lstm_hidden_size=Hl,
                                        latent_state_dim=H, reward_support_size=V, value_support_size=V, **kw).eval()


@pytest.mark.parametrize("res, H, F_", [(False, 32, 32), (True, 32, 32), (False, 16, 32), (True, 64, 16)])
def test_packed_size_matches_the_library(res, H, F_):
    m = model(H=H, res_connection_in_dynamics=res, fc_value_layers=(F_,), fc_reward_layers=(F_,), bound_type="tanh")
    flat, dims = pack_sampled_efficientzero_mlp(m, "cpu")
    assert dims == dict(hidden=H, lstm_hidden=16, dim=3, head_hidden=F_, support=21, res=res, tanh=True)
    assert flat.numel() == _lib.load().lzm_mlp_sampled_packed_floats(H, 16, 3, F_, 21, int(res))
    assert _lib.load().lzm_mlp_sampled_kernel_floats(H, 16, 3, F_, 21, int(res)) >= flat.numel()


def test_layer_order_of_the_merged_tail():
    """H = 16 < F = 32: mu / log_sigma read 16 of the output layer's 32 input columns, the rest are zeros"""
    m = model(H=16, norm_type=None)
    layers, dims = describe_sampled(m)
    pred, head = m.prediction_network, m.prediction_network.fc_policy_head
    assert [tuple(w.shape) for (w, _), _ in layers] == [
        (16, 19), (16, 16), (64, 32), (32, 16), (21, 32), (16, 16), (16, 16), (48, 16), (16, 16), (27, 32)]
    assert [relu for _, relu in layers] == [True, True, False, True, False, True, True, True, True, False]
    (wh, bh), (wm, _), (wo, bo) = (layers[i][0] for i in (7, 8, 9))
    assert torch.equal(wh, torch.cat((pred.fc_value_head[0].weight, head.main[0].weight)))
    assert torch.equal(bh, torch.cat((pred.fc_value_head[0].bias, head.main[0].bias)))
    assert torch.equal(wm, head.main[2].weight)
    assert torch.equal(wo[:21], pred.fc_value_head[2].weight)
    assert torch.equal(wo[21:24, :16], head.mu.weight) and torch.equal(wo[24:, :16], head.log_sigma_layer.weight)
    assert not wo[21:, 16:].any()
    assert torch.equal(bo, torch.cat((pred.fc_value_head[2].bias, head.mu.bias, head.log_sigma_layer.bias)))


def test_fixed_sigma_reproduces_the_constant_row_through_exp():
    m = model(sigma_type="fixed", fixed_sigma_value=0.3)
    (w, b), _ = describe_sampled(m)[0][-1]
    assert not w[24:].any() and torch.equal(b[24:], torch.full((3,), math.log(0.3)))
    out = m.prediction_network(torch.randn(4, 32))[0]
    torch.testing.assert_close(torch.exp(b[24:]).expand(4, 3), out[:, 3:], rtol=1e-6, atol=0)


@pytest.mark.parametrize("why, make", [
    ("discrete action space", lambda: model(continuous_action_space=False)),
    ("sigma_type 'independent'", lambda: model(sigma_type="independent")),
    ("fixed_sigma_value 8.0 outside", lambda: model(sigma_type="fixed", fixed_sigma_value=8.0)),
    ("kSampledMaxDim", lambda: model(D=33, H=48)),
    ("state_norm", lambda: model(state_norm=True)),
    ("BatchNorm in training mode", lambda: model().train()),
])
def test_refusals_carry_their_reasons(why, make):
    with pytest.raises(NotPackable, match=why):
        describe_sampled(make())


def test_library_shape_limits_refuse_with_the_shape():
    ok = _lib.load().lzm_search_mlp_sampled_supported  # (dim, hidden, lstm_hidden, head_hidden, support)
    assert ok(3, 128, 128, 32, 601) == 1 and ok(4, 256, 256, 32, 601) == 1 and ok(32, 64, 16, 32, 21) == 1
    assert ok(33, 128, 128, 32, 21) == 0 and ok(3, 128, 24, 32, 21) == 0 and ok(17, 32, 16, 32, 21) == 0
    with pytest.raises(NotPackable, match="outside the search kernels' range"):
        pack_sampled_efficientzero_mlp(model(Hl=24), "cpu")


@pytest.mark.parametrize("res, bound", [(False, None), (True, "tanh")])
def test_recurrent_inference_equals_a_hand_written_float64_forward(res, bound):
    m = model(res_connection_in_dynamics=res, bound_type=bound).double()
    for bn in (x for x in m.modules() if isinstance(x, torch.nn.BatchNorm1d)):
        bn.running_mean.normal_(0.0, 0.3), bn.running_var.uniform_(0.5, 1.5)
    p = dict(m.named_parameters()) | dict(m.named_buffers())

    def block(x, name, n, last_plain):  # mlp(): Linear, BatchNorm (eval), ReLU per layer; the last one plain or not
        for j in range(n):
            i = 3 * j
            x = F.linear(x, p[f"{name}.{i}.weight"], p[f"{name}.{i}.bias"])
            if j + 1 < n or not last_plain:
                x = (x - p[f"{name}.{i + 1}.running_mean"]) / torch.sqrt(p[f"{name}.{i + 1}.running_var"] + 1e-5)
                x = torch.relu(x * p[f"{name}.{i + 1}.weight"] + p[f"{name}.{i + 1}.bias"])
        return x
    lat, act = torch.randn(6, 32, dtype=torch.float64), torch.rand(6, 3, dtype=torch.float64) * 2 - 1
    h0, c0 = torch.randn(2, 1, 6, 16, dtype=torch.float64) * 0.3
    x = torch.cat((lat, act), dim=1)
    if res:
        nxt = block(x, "dynamics_network.fc_dynamics_1", 2, False) + lat
        xin = block(nxt, "dynamics_network.fc_dynamics_2", 2, False)
    else:
        nxt = xin = block(x, "dynamics_network.fc_dynamics", 2, False)
    q = "dynamics_network.lstm."
    gates = F.linear(xin, p[q + "weight_ih_l0"], p[q + "bias_ih_l0"]) + F.linear(h0[0], p[q + "weight_hh_l0"],
                                                                                 p[q + "bias_hh_l0"])
    gi, gf, gg, go = gates.chunk(4, dim=1)
    c1 = torch.sigmoid(gf) * c0[0] + torch.sigmoid(gi) * torch.tanh(gg)
    h1 = torch.sigmoid(go) * torch.tanh(c1)
    vp = block(h1, "dynamics_network.fc_reward_head", 2, True)
    com = block(nxt, "prediction_network.fc_prediction_common", 2, False)
    value = block(com, "prediction_network.fc_value_head", 2, True)
    q = "prediction_network.fc_policy_head."
    y = torch.relu(F.linear(com, p[q + "main.0.weight"], p[q + "main.0.bias"]))
    y = torch.relu(F.linear(y, p[q + "main.2.weight"], p[q + "main.2.bias"]))
    mu = F.linear(y, p[q + "mu.weight"], p[q + "mu.bias"])
    mu = torch.tanh(mu) if bound else mu
    sigma = torch.exp(F.linear(y, p[q + "log_sigma_layer.weight"], p[q + "log_sigma_layer.bias"]).clamp(-20, 2))
    with torch.no_grad():
        out = m.recurrent_inference(lat, (h0, c0), act)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(out.latent_state, nxt, **tol)
    torch.testing.assert_close(out.reward_hidden_state[0][0], h1, **tol)
    torch.testing.assert_close(out.reward_hidden_state[1][0], c1, **tol)
    torch.testing.assert_close(out.value_prefix, vp, **tol)
    torch.testing.assert_close(out.value, value, **tol)
    torch.testing.assert_close(out.policy_logits, torch.cat((mu, sigma), dim=1), **tol)
