"""A small two-branch network with StochasticMuZeroModel's recurrent_inference(state, option, afterstate)
(stochastic_muzero_model.py:233-273), for the stochastic search's tests and tools/stochastic_search_time.py."""
from types import SimpleNamespace

import torch
from torch import nn


class TwoBranchNet(nn.Module):
    def __init__(self, latent=16, actions=4, chance=32, support=21, hidden=32):
        super().__init__()
        self.A, self.C = actions, chance
        mlp = lambda i: nn.Sequential(nn.Linear(i, hidden), nn.ReLU(), nn.Linear(hidden, latent))
        self.afterstate_dynamics, self.dynamics = mlp(latent + actions), mlp(latent + chance)
        self.reward = nn.Linear(latent, support)
        self.afterstate_value, self.afterstate_policy = nn.Linear(latent, support), nn.Linear(latent, chance)
        self.value, self.policy = nn.Linear(latent, support), nn.Linear(latent, actions)

    def recurrent_inference(self, state, option, afterstate=False):
        """afterstate=False: state + action -> afterstate, its value and the chance logits (a chance leaf);
        afterstate=True: afterstate + outcome -> next state, reward, value and the policy logits (a decision leaf)"""
        hot = nn.functional.one_hot(option.long(), self.C if afterstate else self.A).to(state.dtype)
        x = torch.cat([state, hot], dim=1)
        if not afterstate:
            s = self.afterstate_dynamics(x)
            return SimpleNamespace(value=self.afterstate_value(s), reward=torch.zeros_like(self.reward(s)),
                                   policy_logits=self.afterstate_policy(s), latent_state=s)
        s = self.dynamics(x)
        return SimpleNamespace(value=self.value(s), reward=self.reward(s), policy_logits=self.policy(s), latent_state=s)
