"""CPU: fused.describe_stochastic / pack_stochastic_mlp over StochasticMuZeroModelMLP — the packed sizes against the
library's, the refusals, and the library's shape limits (host only)."""
import pytest
import torch
import torch.nn as nn

from lightzero_amd import _lib
from lightzero_amd.fused import NotPackable, describe_stochastic, pack_stochastic_mlp
from lightzero_amd.model_mlp import StochasticMuZeroModelMLP


def model(A=4, C=2, H=32, V=21, **kw):
    return StochasticMuZeroModelMLP(observation_shape=5, action_space_size=A, chance_space_size=C, latent_state_dim=H,
                                    reward_support_size=V, value_support_size=V, **kw).eval()


@pytest.mark.parametrize("res", [False, True])
def test_packed_size_matches_the_library_and_sharing_saves_one_dynamics_network(res):
    L, n = _lib.load(), {}
    for shared in (True, False):
        flat, dims = pack_stochastic_mlp(model(res_connection_in_dynamics=res, shared_dynamics=shared), "cpu")
        assert dims == dict(hidden=32, actions=4, chance=2, head_hidden=32, support=21, res=res, shared=shared)
        n[shared] = flat.numel()
        assert n[shared] == L.lzm_mlp_stoch_packed_floats(32, 4, 2, 32, 21, int(res), int(shared))
    # the dynamics layers of one DynamicsNetwork: [H + A -> H], then H -> H (three more with the residual block)
    assert n[False] - n[True] == (36 * 32 + 32) + (3 if res else 1) * (32 * 32 + 32)


def test_branch_order_of_the_packed_layers():
    """unshared: the last layers are afterstate_dynamics_network's; shared: dynamics_network's come first, once"""
    m = model(norm_type=None, shared_dynamics=False)
    layers, _ = describe_stochastic(m)
    assert len(layers) == 2 + 2 + 6 + 6 + 2
    assert layers[9][0][0].shape[0] == 4 and layers[15][0][0].shape[0] == 2  # policy rows: A, then C
    assert torch.equal(layers[0][0][0], m.dynamics_network.fc_dynamics[0].weight)
    assert torch.equal(layers[16][0][0], m.afterstate_dynamics_network.fc_dynamics[0].weight)
    assert len(describe_stochastic(model(shared_dynamics=True))[0]) == 16


@pytest.mark.parametrize("why, make", [
    ("chance > actions", lambda: _wider_chance()),
    ("activation", lambda: _with(lambda m: setattr(m.prediction_network.fc_value_head, "2", nn.Tanh()))),
    ("BatchNorm in training mode", lambda: _with(lambda m: m.afterstate_prediction_network.train())),
    ("state_norm", lambda: model(state_norm=True)),
])
def test_refusals(why, make):
    with pytest.raises(NotPackable, match=why if why != "chance > actions" else "chance space"):
        describe_stochastic(make())


def _with(change):
    m = model()
    change(m)
    return m


def _wider_chance():
    m = model(A=4, C=4)
    m.afterstate_prediction_network = type(m.prediction_network)(6, 32, output_support_size=21).eval()
    return m


def test_shape_limits_on_the_host():
    ok = _lib.load().lzm_search_mlp_stoch_supported  # (actions, chance, hidden, head_hidden, support)
    assert ok(2, 2, 128, 32, 601) == 1 and ok(64, 64, 64, 32, 21) == 1 and ok(4, 2, 16, 16, 21) == 1
    assert ok(65, 2, 128, 32, 21) == 0 and ok(4, 5, 128, 32, 21) == 0 and ok(4, 0, 128, 32, 21) == 0
    assert ok(33, 2, 32, 32, 21) == 0 and ok(2, 2, 100, 32, 21) == 0 and ok(2, 2, 64, 24, 21) == 0
