"""MuZeroModelMLP restated for PyTorch-ROCm (the network the CartPole search calls every simulation).

Reference: /root/reference/lzero/model/muzero_model_mlp.py:12-204 (model, ``initial_inference``,
``recurrent_inference``), ``DynamicsNetwork`` :327-440, and lzero/model/common.py
(``RepresentationNetworkMLP`` :467-517, ``PredictionNetworkMLP`` :883-971, ``SimNorm`` :53-91).
Every block there is built by DI-engine's ``MLP`` (not installed here); its construction is
restated in ``mlp()``: ``layer_num`` Linear layers with widths [in] + [hidden]*(layer_num-1) +
[out]; each hidden Linear is followed by BatchNorm1d then the activation; the last Linear is
followed by BatchNorm only if ``output_norm`` and the activation only if ``output_activation``;
``last_linear_layer_init_zero`` zeroes the last Linear's weight and bias.

Parity note: DI-engine is absent, so the network's numerics are not pinned to reference
outputs; the architecture, widths, init rules and forward order are.
"""
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class MZNetworkOutput:  # lzero/model/common.py:45-50
    value: torch.Tensor
    reward: torch.Tensor
    policy_logits: torch.Tensor
    latent_state: torch.Tensor


def mlp(in_channels: int, hidden_channels: int, out_channels: int, layer_num: int, activation: nn.Module,
        norm_type: Optional[str] = 'BN', output_activation: bool = True, output_norm: bool = True,
        last_linear_layer_init_zero: bool = False) -> nn.Sequential:
    channels = [in_channels] + [hidden_channels] * (layer_num - 1) + [out_channels]
    layers = []
    for i in range(layer_num - 1):
        layers.append(nn.Linear(channels[i], channels[i + 1]))
        if norm_type == 'BN':
            layers.append(nn.BatchNorm1d(channels[i + 1]))
        elif norm_type == 'LN':
            layers.append(nn.LayerNorm(channels[i + 1]))
        layers.append(activation)
    last = nn.Linear(channels[-2], channels[-1])
    layers.append(last)
    if output_norm and norm_type == 'BN':
        layers.append(nn.BatchNorm1d(channels[-1]))
    elif output_norm and norm_type == 'LN':
        layers.append(nn.LayerNorm(channels[-1]))
    if output_activation:
        layers.append(activation)
    if last_linear_layer_init_zero:
        nn.init.zeros_(last.weight)
        nn.init.zeros_(last.bias)
    return nn.Sequential(*layers)


class SimNorm(nn.Module):
    """Softmax over consecutive groups of ``dim`` features (common.py:53-91)."""

    def __init__(self, simnorm_dim: int) -> None:
        super().__init__()
        self.dim = simnorm_dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shp = x.shape
        if shp[1] == 0:
            return x
        return F.softmax(x.view(*shp[:-1], -1, self.dim), dim=-1).view(*shp)


class RepresentationNetworkMLP(nn.Module):
    def __init__(self, observation_shape: int, hidden_channels: int = 64, layer_num: int = 2,
                 activation: nn.Module = nn.GELU(approximate='tanh'), norm_type: Optional[str] = 'BN',
                 group_size: int = 8):
        super().__init__()
        self.fc_representation = mlp(observation_shape, hidden_channels, hidden_channels, layer_num, activation,
                                     norm_type, output_activation=False, output_norm=False,
                                     last_linear_layer_init_zero=True)
        self.sim_norm = SimNorm(group_size)

    def forward(self, x):
        return self.sim_norm(self.fc_representation(x))


class PredictionNetworkMLP(nn.Module):
    def __init__(self, action_space_size: int, num_channels: int, common_layer_num: int = 2,
                 fc_value_layers: Sequence[int] = (32,), fc_policy_layers: Sequence[int] = (32,),
                 output_support_size: int = 601, last_linear_layer_init_zero: bool = True,
                 activation: nn.Module = nn.ReLU(inplace=True), norm_type: Optional[str] = 'BN'):
        super().__init__()
        self.fc_prediction_common = mlp(num_channels, num_channels, num_channels, common_layer_num, activation,
                                        norm_type, output_activation=True, output_norm=True)
        self.fc_value_head = mlp(num_channels, fc_value_layers[0], output_support_size, len(fc_value_layers) + 1,
                                 activation, norm_type, output_activation=False, output_norm=False,
                                 last_linear_layer_init_zero=last_linear_layer_init_zero)
        self.fc_policy_head = mlp(num_channels, fc_policy_layers[0], action_space_size, len(fc_policy_layers) + 1,
                                  activation, norm_type, output_activation=False, output_norm=False,
                                  last_linear_layer_init_zero=last_linear_layer_init_zero)

    def forward(self, latent_state):
        x = self.fc_prediction_common(latent_state)
        return self.fc_policy_head(x), self.fc_value_head(x)


class DynamicsNetwork(nn.Module):
    def __init__(self, action_encoding_dim: int = 2, num_channels: int = 64, common_layer_num: int = 2,
                 fc_reward_layers: Sequence[int] = (32,), output_support_size: int = 601,
                 last_linear_layer_init_zero: bool = True, activation: nn.Module = nn.ReLU(inplace=True),
                 norm_type: Optional[str] = 'BN', res_connection_in_dynamics: bool = False):
        super().__init__()
        self.action_encoding_dim = action_encoding_dim
        self.latent_state_dim = num_channels - action_encoding_dim
        self.res_connection_in_dynamics = res_connection_in_dynamics
        H = self.latent_state_dim
        if res_connection_in_dynamics:
            self.fc_dynamics_1 = mlp(num_channels, H, H, common_layer_num, activation, norm_type, True, True)
            self.fc_dynamics_2 = mlp(H, H, H, common_layer_num, activation, norm_type, True, True)
        else:
            self.fc_dynamics = mlp(num_channels, H, H, common_layer_num, activation, norm_type, True, True)
        self.fc_reward_head = mlp(H, fc_reward_layers[0], output_support_size, 2, activation, norm_type,
                                  output_activation=False, output_norm=False,
                                  last_linear_layer_init_zero=last_linear_layer_init_zero)

    def forward(self, state_action_encoding):
        if self.res_connection_in_dynamics:
            latent_state = state_action_encoding[:, :-self.action_encoding_dim]
            next_latent_state = self.fc_dynamics_1(state_action_encoding) + latent_state
            enc = self.fc_dynamics_2(next_latent_state)
        else:
            next_latent_state = self.fc_dynamics(state_action_encoding)
            enc = next_latent_state
        return next_latent_state, self.fc_reward_head(enc)


class MuZeroModelMLP(nn.Module):
    """MuZero for vector observations (muzero_model_mlp.py:12-204), discrete one-hot actions."""

    def __init__(self, observation_shape: int = 2, action_space_size: int = 6, latent_state_dim: int = 256,
                 fc_reward_layers=(32,), fc_value_layers=(32,), fc_policy_layers=(32,),
                 reward_support_size: int = 601, value_support_size: int = 601,
                 categorical_distribution: bool = True, last_linear_layer_init_zero: bool = True,
                 norm_type: Optional[str] = 'BN', res_connection_in_dynamics: bool = False, **kwargs):
        super().__init__()
        self.categorical_distribution = categorical_distribution
        self.reward_support_size = reward_support_size if categorical_distribution else 1
        self.value_support_size = value_support_size if categorical_distribution else 1
        self.action_space_size = action_space_size
        self.latent_state_dim = latent_state_dim
        self.representation_network = RepresentationNetworkMLP(observation_shape, latent_state_dim,
                                                               norm_type=norm_type)
        self.dynamics_network = DynamicsNetwork(action_space_size, latent_state_dim + action_space_size, 2,
                                                fc_reward_layers, self.reward_support_size,
                                                last_linear_layer_init_zero, norm_type=norm_type,
                                                res_connection_in_dynamics=res_connection_in_dynamics)
        self.prediction_network = PredictionNetworkMLP(action_space_size, latent_state_dim,
                                                       fc_value_layers=fc_value_layers,
                                                       fc_policy_layers=fc_policy_layers,
                                                       output_support_size=self.value_support_size,
                                                       last_linear_layer_init_zero=last_linear_layer_init_zero,
                                                       norm_type=norm_type)

    def initial_inference(self, obs: torch.Tensor) -> MZNetworkOutput:
        latent_state = self.representation_network(obs)
        policy_logits, value = self.prediction_network(latent_state)
        return MZNetworkOutput(value, [0. for _ in range(obs.size(0))], policy_logits, latent_state)

    def recurrent_inference(self, latent_state: torch.Tensor, action: torch.Tensor) -> MZNetworkOutput:
        a = action.long().reshape(-1, 1)
        one_hot = torch.zeros(a.shape[0], self.action_space_size, device=latent_state.device)
        one_hot.scatter_(1, a, 1)
        next_latent_state, reward = self.dynamics_network(torch.cat((latent_state, one_hot), dim=1))
        policy_logits, value = self.prediction_network(next_latent_state)
        return MZNetworkOutput(value, reward, policy_logits, next_latent_state)


class DynamicsNetworkMLP(nn.Module):
    """EfficientZero's MLP dynamics with the reward LSTM (efficientzero_model_mlp.py:341-475): the dynamics
    layers, one ``nn.LSTM`` step on their output, the value-prefix head on the LSTM's output."""

    def __init__(self, action_encoding_dim: int = 2, num_channels: int = 64, common_layer_num: int = 2,
                 fc_reward_layers: Sequence[int] = (32,), output_support_size: int = 601,
                 lstm_hidden_size: int = 512, last_linear_layer_init_zero: bool = True,
                 activation: nn.Module = nn.ReLU(inplace=True), norm_type: Optional[str] = 'BN',
                 res_connection_in_dynamics: bool = False):
        super().__init__()
        assert num_channels > action_encoding_dim, (num_channels, action_encoding_dim)
        self.num_channels = num_channels
        self.action_encoding_dim = action_encoding_dim
        self.latent_state_dim = num_channels - action_encoding_dim
        self.lstm_hidden_size = lstm_hidden_size
        self.activation = activation
        self.res_connection_in_dynamics = res_connection_in_dynamics
        H = self.latent_state_dim
        if res_connection_in_dynamics:
            self.fc_dynamics_1 = mlp(num_channels, H, H, common_layer_num, activation, norm_type, True, True)
            self.fc_dynamics_2 = mlp(H, H, H, common_layer_num, activation, norm_type, True, True)
        else:
            self.fc_dynamics = mlp(num_channels, H, H, common_layer_num, activation, norm_type, True, True)
        self.lstm = nn.LSTM(input_size=H, hidden_size=lstm_hidden_size)
        self.fc_reward_head = mlp(lstm_hidden_size, fc_reward_layers[0], output_support_size, 2, activation,
                                  norm_type, output_activation=False, output_norm=False,
                                  last_linear_layer_init_zero=last_linear_layer_init_zero)

    def forward(self, state_action_encoding, reward_hidden_state):
        if self.res_connection_in_dynamics:
            latent_state = state_action_encoding[:, :-self.action_encoding_dim]
            next_latent_state = self.fc_dynamics_1(state_action_encoding) + latent_state
            lstm_in = self.fc_dynamics_2(next_latent_state)  # the LSTM's input; the filed latent is x + latent
        else:
            next_latent_state = self.fc_dynamics(state_action_encoding)
            lstm_in = next_latent_state
        value_prefix, next_reward_hidden_state = self.lstm(lstm_in.unsqueeze(0), reward_hidden_state)
        value_prefix = self.fc_reward_head(value_prefix.squeeze(0))
        return next_latent_state, next_reward_hidden_state, value_prefix


class EfficientZeroModelMLP(nn.Module):
    """EfficientZero for vector observations (efficientzero_model_mlp.py:14-338), discrete actions. The
    projection / prediction heads of the self-supervised loss (training only) are not restated."""

    def __init__(self, observation_shape: int = 2, action_space_size: int = 6, lstm_hidden_size: int = 512,
                 latent_state_dim: int = 256, fc_reward_layers=(32,), fc_value_layers=(32,), fc_policy_layers=(32,),
                 reward_support_size: int = 601, value_support_size: int = 601,
                 categorical_distribution: bool = True, last_linear_layer_init_zero: bool = True,
                 state_norm: bool = False, norm_type: Optional[str] = 'BN',
                 discrete_action_encoding_type: str = 'one_hot', res_connection_in_dynamics: bool = False,
                 **kwargs):
        super().__init__()
        self.categorical_distribution = categorical_distribution
        self.reward_support_size = reward_support_size if categorical_distribution else 1
        self.value_support_size = value_support_size if categorical_distribution else 1
        self.action_space_size = action_space_size
        assert discrete_action_encoding_type in ('one_hot', 'not_one_hot'), discrete_action_encoding_type
        self.discrete_action_encoding_type = discrete_action_encoding_type
        self.action_encoding_dim = action_space_size if discrete_action_encoding_type == 'one_hot' else 1
        self.lstm_hidden_size = lstm_hidden_size
        self.latent_state_dim = latent_state_dim
        self.last_linear_layer_init_zero = last_linear_layer_init_zero
        self.state_norm = state_norm
        self.res_connection_in_dynamics = res_connection_in_dynamics
        self.representation_network = RepresentationNetworkMLP(observation_shape, latent_state_dim,
                                                               norm_type=norm_type)
        self.dynamics_network = DynamicsNetworkMLP(self.action_encoding_dim,
                                                   latent_state_dim + self.action_encoding_dim, 2,
                                                   lstm_hidden_size=lstm_hidden_size,
                                                   fc_reward_layers=fc_reward_layers,
                                                   output_support_size=self.reward_support_size,
                                                   last_linear_layer_init_zero=last_linear_layer_init_zero,
                                                   norm_type=norm_type,
                                                   res_connection_in_dynamics=res_connection_in_dynamics)
        self.prediction_network = PredictionNetworkMLP(action_space_size, latent_state_dim,
                                                       fc_value_layers=fc_value_layers,
                                                       fc_policy_layers=fc_policy_layers,
                                                       output_support_size=self.value_support_size,
                                                       last_linear_layer_init_zero=last_linear_layer_init_zero,
                                                       norm_type=norm_type)

    @staticmethod
    def _renormalize(x):  # lzero/model/utils.py:103-120 renormalize: min-max over the features
        lo, hi = x.min(1, keepdim=True).values, x.max(1, keepdim=True).values
        return (x - lo) / (hi - lo)

    def initial_inference(self, obs: torch.Tensor):
        from .model_conv import EZNetworkOutput  # (model_conv imports this module)
        B = obs.size(0)
        latent_state = self.representation_network(obs)
        if self.state_norm:
            latent_state = self._renormalize(latent_state)
        policy_logits, value = self.prediction_network(latent_state)
        hidden = (torch.zeros(1, B, self.lstm_hidden_size, device=obs.device),
                  torch.zeros(1, B, self.lstm_hidden_size, device=obs.device))
        return EZNetworkOutput(value, [0. for _ in range(B)], policy_logits, latent_state, hidden)

    def recurrent_inference(self, latent_state: torch.Tensor, reward_hidden_state, action: torch.Tensor):
        from .model_conv import EZNetworkOutput
        if self.discrete_action_encoding_type == 'one_hot':
            a = action.long().reshape(-1, 1)
            enc = torch.zeros(a.shape[0], self.action_space_size, device=latent_state.device,
                              dtype=latent_state.dtype)
            enc.scatter_(1, a, 1)
        else:
            enc = (action / self.action_space_size).reshape(-1, 1).to(latent_state)
        next_latent_state, hidden, value_prefix = self.dynamics_network(torch.cat((latent_state, enc), dim=1),
                                                                        reward_hidden_state)
        if self.state_norm:
            next_latent_state = self._renormalize(next_latent_state)
        policy_logits, value = self.prediction_network(next_latent_state)
        return EZNetworkOutput(value, value_prefix, policy_logits, next_latent_state, hidden)


class ReparameterizationHead(nn.Module):
    """DI-engine's ``ding.model.common.head.ReparameterizationHead`` (not installed here), restated from its source
    as remembered — submodule names, forward order and constants; not checked against an installed DI-engine:
    ``main`` = ``layer_num`` Linear(H, H) + activation layers without norm, ``mu = Linear(H, D)``, and by
    ``sigma_type``: 'conditioned' ``log_sigma_layer = Linear(H, D)`` with sigma = exp(clamp(log_sigma, -20, 2));
    'independent' a parameter ``log_sigma_param`` [1, D] with sigma = exp(log_sigma_param); 'fixed' a constant row of
    ``fixed_sigma_value``. ``bound_type='tanh'`` applies tanh to mu. Returns {'mu', 'sigma'}."""

    def __init__(self, input_size: int, output_size: int, layer_num: int = 2, sigma_type: str = 'conditioned',
                 fixed_sigma_value: float = 1.0, activation: nn.Module = nn.ReLU(), norm_type: Optional[str] = None,
                 bound_type: Optional[str] = None):
        super().__init__()
        assert sigma_type in ('fixed', 'independent', 'conditioned'), sigma_type
        assert bound_type in ('tanh', None), bound_type
        assert norm_type is None, "the Sampled EfficientZero models build this head without a norm"
        self.sigma_type, self.bound_type, self.fixed_sigma_value = sigma_type, bound_type, float(fixed_sigma_value)
        layers = []
        for _ in range(layer_num):
            layers += [nn.Linear(input_size, input_size), activation]
        self.main = nn.Sequential(*layers)
        self.mu = nn.Linear(input_size, output_size)
        if sigma_type == 'fixed':
            self.register_buffer('sigma', torch.full((1, output_size), float(fixed_sigma_value)), persistent=False)
        elif sigma_type == 'independent':
            self.log_sigma_param = nn.Parameter(torch.zeros(1, output_size))
        else:
            self.log_sigma_layer = nn.Linear(input_size, output_size)

    def forward(self, x):
        x = self.main(x)
        mu = self.mu(x)
        if self.bound_type == 'tanh':
            mu = torch.tanh(mu)
        if self.sigma_type == 'fixed':
            sigma = self.sigma.to(mu) + torch.zeros_like(mu)
        elif self.sigma_type == 'independent':
            sigma = torch.exp(self.log_sigma_param + torch.zeros_like(mu))
        else:
            sigma = torch.exp(torch.clamp(self.log_sigma_layer(x), -20, 2))
        return {'mu': mu, 'sigma': sigma}


class SampledPredictionNetworkMLP(nn.Module):
    """sampled_efficientzero_model_mlp.py:386-521: fc_prediction_common, fc_value_head and, for a continuous action
    space, a ReparameterizationHead as fc_policy_head (policy = cat(mu, sigma)); an MLP head otherwise."""

    def __init__(self, continuous_action_space: bool, action_space_size: int, num_channels: int,
                 fc_value_layers: Sequence[int] = (32,), fc_policy_layers: Sequence[int] = (32,),
                 output_support_size: int = 601, last_linear_layer_init_zero: bool = True,
                 activation: nn.Module = nn.ReLU(inplace=True), norm_type: Optional[str] = 'BN',
                 sigma_type: str = 'conditioned', fixed_sigma_value: float = 0.3, bound_type: Optional[str] = None):
        super().__init__()
        self.continuous_action_space = continuous_action_space
        self.fc_prediction_common = mlp(num_channels, num_channels, num_channels, 2, activation, norm_type,
                                        output_activation=True, output_norm=True)
        self.fc_value_head = mlp(num_channels, fc_value_layers[0], output_support_size, 2, activation, norm_type,
                                 output_activation=False, output_norm=False,
                                 last_linear_layer_init_zero=last_linear_layer_init_zero)
        if continuous_action_space:
            self.fc_policy_head = ReparameterizationHead(num_channels, action_space_size, 2, sigma_type,
                                                         fixed_sigma_value, nn.ReLU(), None, bound_type)
        else:
            self.fc_policy_head = mlp(num_channels, fc_policy_layers[0], action_space_size, 2, activation, norm_type,
                                      output_activation=False, output_norm=False,
                                      last_linear_layer_init_zero=last_linear_layer_init_zero)

    def forward(self, latent_state):
        x = self.fc_prediction_common(latent_state)
        value = self.fc_value_head(x)
        policy = self.fc_policy_head(x)
        if self.continuous_action_space:
            policy = torch.cat([policy['mu'], policy['sigma']], dim=-1)
        return policy, value


class SampledEfficientZeroModelMLP(nn.Module):
    """Sampled EfficientZero for vector observations (sampled_efficientzero_model_mlp.py:14-384): EfficientZeroModelMLP
    with, for ``continuous_action_space=True``, the dynamics input [latent ; action] (the action as D floats,
    ``action_encoding_dim = D``) and DI-engine's ReparameterizationHead as the policy head, ``policy_logits =
    cat(mu, sigma)``; a discrete space keeps EfficientZeroModelMLP's encodings and MLP policy head. The constructor
    keywords, ``initial_inference`` / ``recurrent_inference`` and the EZNetworkOutput fields are
    EfficientZeroModelMLP's. The projection / prediction heads of the self-supervised loss are not restated."""

    def __init__(self, observation_shape: int = 2, action_space_size: int = 6, lstm_hidden_size: int = 512,
                 latent_state_dim: int = 256, fc_reward_layers=(32,), fc_value_layers=(32,), fc_policy_layers=(32,),
                 reward_support_size: int = 601, value_support_size: int = 601,
                 categorical_distribution: bool = True, last_linear_layer_init_zero: bool = True,
                 state_norm: bool = False, norm_type: Optional[str] = 'BN',
                 discrete_action_encoding_type: str = 'one_hot', res_connection_in_dynamics: bool = False,
                 continuous_action_space: bool = False, num_of_sampled_actions: int = 6,
                 sigma_type: str = 'conditioned', fixed_sigma_value: float = 0.3, bound_type: Optional[str] = None,
                 **kwargs):
        super().__init__()
        self.categorical_distribution = categorical_distribution
        self.reward_support_size = reward_support_size if categorical_distribution else 1
        self.value_support_size = value_support_size if categorical_distribution else 1
        self.continuous_action_space = continuous_action_space
        self.action_space_size = action_space_size
        self.num_of_sampled_actions = num_of_sampled_actions
        assert discrete_action_encoding_type in ('one_hot', 'not_one_hot'), discrete_action_encoding_type
        self.discrete_action_encoding_type = discrete_action_encoding_type
        self.action_encoding_dim = action_space_size if (
            continuous_action_space or discrete_action_encoding_type == 'one_hot') else 1
        self.lstm_hidden_size = lstm_hidden_size
        self.latent_state_dim = latent_state_dim
        self.state_norm = state_norm
        self.res_connection_in_dynamics = res_connection_in_dynamics
        self.sigma_type, self.fixed_sigma_value, self.bound_type = sigma_type, fixed_sigma_value, bound_type
        self.representation_network = RepresentationNetworkMLP(observation_shape, latent_state_dim,
                                                               norm_type=norm_type)
        self.dynamics_network = DynamicsNetworkMLP(self.action_encoding_dim,
                                                   latent_state_dim + self.action_encoding_dim, 2,
                                                   lstm_hidden_size=lstm_hidden_size,
                                                   fc_reward_layers=fc_reward_layers,
                                                   output_support_size=self.reward_support_size,
                                                   last_linear_layer_init_zero=last_linear_layer_init_zero,
                                                   norm_type=norm_type,
                                                   res_connection_in_dynamics=res_connection_in_dynamics)
        self.prediction_network = SampledPredictionNetworkMLP(
            continuous_action_space, action_space_size, latent_state_dim, fc_value_layers=fc_value_layers,
            fc_policy_layers=fc_policy_layers, output_support_size=self.value_support_size,
            last_linear_layer_init_zero=last_linear_layer_init_zero, norm_type=norm_type, sigma_type=sigma_type,
            fixed_sigma_value=fixed_sigma_value, bound_type=bound_type)

    _renormalize = staticmethod(EfficientZeroModelMLP._renormalize)
    initial_inference = EfficientZeroModelMLP.initial_inference

    def recurrent_inference(self, latent_state: torch.Tensor, reward_hidden_state, action: torch.Tensor):
        if not self.continuous_action_space:
            return EfficientZeroModelMLP.recurrent_inference(self, latent_state, reward_hidden_state, action)
        from .model_conv import EZNetworkOutput
        if action.dim() == 1:  # (batch,) -> (batch, 1); (batch, D, 1) -> (batch, D)  (:332-339)
            action = action.unsqueeze(-1)
        elif action.dim() == 3:
            action = action.squeeze(-1)
        next_latent_state, hidden, value_prefix = self.dynamics_network(
            torch.cat((latent_state, action.to(latent_state)), dim=1), reward_hidden_state)
        if self.state_norm:
            next_latent_state = EfficientZeroModelMLP._renormalize(next_latent_state)
        policy_logits, value = self.prediction_network(next_latent_state)
        return EZNetworkOutput(value, value_prefix, policy_logits, next_latent_state, hidden)


class StochasticMuZeroModelMLP(nn.Module):
    """Stochastic MuZero for vector observations (stochastic_muzero_model_mlp.py:14-350, ``initial_inference`` and
    ``recurrent_inference`` of stochastic_muzero_model.py:201-273), discrete one-hot options. Attribute names and
    ``state_dict`` keys are the reference's. Not restated: the chance encoder and the self-supervised heads
    (training only; load such a checkpoint with ``strict=False``).

    Restated as the reference behaves: ``_afterstate_dynamics`` calls ``dynamics_network`` (line 277), so
    ``afterstate_dynamics_network`` holds parameters nothing reads, and both branches one-hot their option over
    ``action_space_size``, so ``chance_space_size <= action_space_size``. ``shared_dynamics=False`` (not in the
    reference) makes ``_afterstate_dynamics`` call ``afterstate_dynamics_network``."""

    def __init__(self, observation_shape: int = 2, action_space_size: int = 6, chance_space_size: int = 2,
                 latent_state_dim: int = 256, fc_reward_layers=(32,), fc_value_layers=(32,), fc_policy_layers=(32,),
                 reward_support_size: int = 601, value_support_size: int = 601,
                 categorical_distribution: bool = True, last_linear_layer_init_zero: bool = True,
                 state_norm: bool = False, norm_type: Optional[str] = 'BN', res_connection_in_dynamics: bool = False,
                 shared_dynamics: bool = True, **kwargs):
        super().__init__()
        assert chance_space_size <= action_space_size, "an outcome is one-hot encoded over the action space"
        self.categorical_distribution = categorical_distribution
        self.reward_support_size = reward_support_size if categorical_distribution else 1
        self.value_support_size = value_support_size if categorical_distribution else 1
        self.action_space_size = action_space_size
        self.chance_space_size = chance_space_size
        self.discrete_action_encoding_type = 'one_hot'
        self.action_encoding_dim = action_space_size
        self.latent_state_dim = latent_state_dim
        self.state_norm = state_norm
        self.res_connection_in_dynamics = res_connection_in_dynamics
        self.shared_dynamics = shared_dynamics
        dyn = dict(action_encoding_dim=action_space_size, num_channels=latent_state_dim + action_space_size,
                   common_layer_num=2, fc_reward_layers=fc_reward_layers, output_support_size=self.reward_support_size,
                   last_linear_layer_init_zero=last_linear_layer_init_zero, norm_type=norm_type,
                   res_connection_in_dynamics=res_connection_in_dynamics)
        pred = dict(num_channels=latent_state_dim, fc_value_layers=fc_value_layers, fc_policy_layers=fc_policy_layers,
                    output_support_size=self.value_support_size,
                    last_linear_layer_init_zero=last_linear_layer_init_zero, norm_type=norm_type)
        self.representation_network = RepresentationNetworkMLP(observation_shape, latent_state_dim,
                                                               norm_type=norm_type)
        self.dynamics_network = DynamicsNetwork(**dyn)
        self.prediction_network = PredictionNetworkMLP(action_space_size, **pred)
        self.afterstate_dynamics_network = DynamicsNetwork(**dyn)
        self.afterstate_prediction_network = PredictionNetworkMLP(chance_space_size, **pred)

    def initial_inference(self, obs: torch.Tensor) -> MZNetworkOutput:
        latent_state = self.representation_network(obs)
        if self.state_norm:
            latent_state = EfficientZeroModelMLP._renormalize(latent_state)
        policy_logits, value = self.prediction_network(latent_state)
        return MZNetworkOutput(value, [0. for _ in range(obs.size(0))], policy_logits, latent_state)

    def _step(self, network, state, option):
        a = option.long().reshape(-1, 1)
        one_hot = torch.zeros(a.shape[0], self.action_space_size, device=state.device, dtype=state.dtype)
        one_hot.scatter_(1, a, 1)
        next_state, reward = network(torch.cat((state, one_hot), dim=1))
        return (EfficientZeroModelMLP._renormalize(next_state) if self.state_norm else next_state), reward

    def _dynamics(self, latent_state, action):
        return self._step(self.dynamics_network, latent_state, action)

    def _afterstate_dynamics(self, latent_state, action):
        return self._step(self.dynamics_network if self.shared_dynamics else self.afterstate_dynamics_network,
                          latent_state, action)

    def recurrent_inference(self, state: torch.Tensor, option: torch.Tensor,
                            afterstate: bool = False) -> MZNetworkOutput:
        if afterstate:  # state is an afterstate, option a chance outcome
            next_state, reward = self._dynamics(state, option)
            policy_logits, value = self.prediction_network(next_state)
        else:  # state is a latent state, option an action
            next_state, reward = self._afterstate_dynamics(state, option)
            policy_logits, value = self.afterstate_prediction_network(next_state)
        return MZNetworkOutput(value, reward, policy_logits, next_state)


def cartpole_efficientzero_model(random_heads: bool = True) -> EfficientZeroModelMLP:
    """The CartPole-v0 EfficientZero network (cartpole_efficientzero_config.py:29-38 over efficientzero.py's
    defaults: latent 128, LSTM 128, one-hot actions, BN, no residual, support 601). ``random_heads`` as in
    cartpole_muzero_model."""
    return EfficientZeroModelMLP(observation_shape=4, action_space_size=2, lstm_hidden_size=128,
                                 latent_state_dim=128, categorical_distribution=True,
                                 last_linear_layer_init_zero=not random_heads, norm_type='BN',
                                 res_connection_in_dynamics=False)


def cartpole_muzero_model(random_heads: bool = True) -> MuZeroModelMLP:
    """The CartPole-v0 MuZero network (cartpole_muzero_config.py:31-39 over muzero.py defaults:
    latent 128, one-hot actions, BN, residual dynamics, support 601). ``random_heads`` keeps the
    last linear layers random instead of zero (a trained-net stand-in: zero heads make every
    simulation a tie)."""
    return MuZeroModelMLP(observation_shape=4, action_space_size=2, latent_state_dim=128,
                          categorical_distribution=True, last_linear_layer_init_zero=not random_heads,
                          norm_type='BN', res_connection_in_dynamics=True)
