"""SampledEfficientZeroModel's recurrent_inference(latent, (c, h), action [B, D] float or [B] long) in small."""
from types import SimpleNamespace

import torch
from torch import nn


class SampledNet(nn.Module):
    def __init__(self, latent=16, dim=3, continuous=True, support=21, hidden=32, lstm=8):
        super().__init__()
        self.dim, self.continuous = dim, continuous
        self.dynamics = nn.Sequential(nn.Linear(latent + dim, hidden), nn.ReLU(), nn.Linear(hidden, latent))
        self.gates = nn.Linear(latent + lstm, 4 * lstm)  # the value-prefix LSTM cell, written out
        self.value_prefix, self.value = nn.Linear(lstm, support), nn.Linear(latent, support)
        self.policy = nn.Linear(latent, 2 * dim if continuous else dim)

    def recurrent_inference(self, state, reward_hidden_state, action):
        B = state.shape[0]
        a = (action.to(state.dtype).reshape(B, self.dim) if self.continuous
             else nn.functional.one_hot(action.long().reshape(B), self.dim).to(state.dtype))
        s = self.dynamics(torch.cat([state, a], dim=1))
        c, h = (x.reshape(B, -1) for x in reward_hidden_state)
        i, f, g, o = self.gates(torch.cat([s, h], dim=1)).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        p = self.policy(s)
        if self.continuous:  # {mu, sigma > 0}
            p = torch.cat([p[:, :self.dim], nn.functional.softplus(p[:, self.dim:]) + 0.1], dim=1)
        return SimpleNamespace(value=self.value(s), value_prefix=self.value_prefix(h), policy_logits=p, latent_state=s,
                               reward_hidden_state=(c.unsqueeze(0), h.unsqueeze(0)))
