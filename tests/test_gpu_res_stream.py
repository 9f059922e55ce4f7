"""GPU: the resident search kernel's weight schedule (lzm_search_res.h, the simulation loop's stream
buffer P): fc_dynamics_2[0] staged from LDS behind the tie draw, fc_prediction_common[1] and the
value support refilled slot by slot behind the layer that frees each register.

The tree tests take the kernel's recorded network outputs as given, so a layer fed another layer's
weights on one control path would pass them. Here every simulation's network outputs — the filed next
latent pool[k + 1], the policy logits and the decoded reward and value — are pinned to the torch module's
recurrent_inference on the recorded (x, action), at test_fused_network_matches_torch_module's tolerances,
and the same run's tree to the oracle, on every path that reaches the staged layer: the late draw and the
draw before the dynamics (LZM_RES_LATE=0), simulations without a draw, a root resumed after a tie between
visited children (status 2 / 3), selection modes 1, 4 and 5, glibc and Philox, one root (no look-back)
and a tie at the root through its legal list.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_gpu_fused as tf  # noqa: E402
from tests.test_gpu_fused import DEV, check_tree_exact, fused_search  # noqa: E402
from tests.test_gpu_numerics import torch_inverse_scalar_transform  # noqa: E402
from tests.test_gpu_res_handoff import RAGGED, environ, ragged_roots  # noqa: E402
from tests.test_gpu_walk_regs import assert_both_endings, last_linear, oracle_mismatch  # noqa: E402

A, H, SCALE = 2, 128, 300
make_model = tf.make_model  # (the case below replaces tf.make_model)


def check_network(r):
    """every simulation's recorded network outputs against model.recurrent_inference(pool[x], action)"""
    rec, pool, model = r["rec"], r["pool"], r["model"]
    S, B = rec["x"].shape
    idx = torch.arange(B, device=DEV)
    with torch.no_grad():
        for k in range(S):
            x = torch.from_numpy(rec["x"][k]).long().to(DEV)
            out = model.recurrent_inference(pool[x, idx], torch.from_numpy(rec["action"][k]).long().to(DEV))
            torch.testing.assert_close(pool[k + 1], out.latent_state, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(torch.from_numpy(rec["policy_logits"][k]).to(DEV), out.policy_logits,
                                       rtol=1e-4, atol=1e-5)
            dec = torch.from_numpy(rec["decoded"][k]).to(DEV)
            torch.testing.assert_close(dec[:, 0], torch_inverse_scalar_transform(out.reward, SCALE).squeeze(1),
                                       rtol=1e-4, atol=1e-5 * SCALE)
            torch.testing.assert_close(dec[:, 1], torch_inverse_scalar_transform(out.value, SCALE).squeeze(1),
                                       rtol=1e-4, atol=1e-5 * SCALE)


def pinned(case, **env):
    """the search of case under env: its tree equal to the oracle, its network outputs to the module"""
    with environ(**env):
        r = check_tree_exact(case)
    check_network(r)
    return r


@pytest.mark.parametrize("players", [1, 2])
@pytest.mark.parametrize("env", [{}, {"LZM_RES_LATE": "0"}, {"LZM_RES_SELECT": "1"}, {"LZM_RES_SELECT": "4"}],
                         ids=["default", "late0", "select1", "select4"])
def test_glibc_both_walk_endings(env, players):
    r = pinned((8, 25, A, H, False, players, False), **env)
    assert_both_endings(r["rec"])  # (simulations with a leaf tie's draw and simulations without one)


def test_philox():
    pinned((8, 25, A, H, False, 1, True))


def test_one_root():
    pinned((1, 10, A, H, False, 1, False))


def test_root_tie_through_the_legal_list(monkeypatch):
    B, S = 3, 2
    ragged_roots(monkeypatch, RAGGED)
    r = fused_search(B, S, A, H, False, 1, False, seed=B + S + A)
    assert r["diag"][0] == 0 and r["diag"][3] == 0
    assert oracle_mismatch(r, B, S, legal=RAGGED) is None
    check_network(r)


def action_blind_model(*args, **kw):
    """make_model's network with the dynamics blind to the action and a constant policy: siblings get
    bit-identical latents, rewards, values and equal priors, so two visited siblings tie exactly (status
    2 / 3), while every head output still depends on the hidden layers."""
    m = make_model(*args, **kw)
    first = [q for q in m.dynamics_network.fc_dynamics_1.modules() if isinstance(q, torch.nn.Linear)][0]
    last = last_linear(m.prediction_network.fc_policy_head)
    with torch.no_grad():
        assert first.weight.shape[1] == H + A
        first.weight[:, H:].zero_()
        last.weight.zero_()
        last.bias.zero_()
    return m


def test_resumed_roots_with_live_heads(monkeypatch):
    monkeypatch.setattr(tf, "make_model", action_blind_model)
    r = pinned((8, 25, A, H, False, 1, False))
    assert r["diag"][2] > 0, "no tie between visited children was resolved through depth speculation"
    assert r["diag"][0] == 0 and r["diag"][3] == 0
    dec = r["rec"]["decoded"]
    assert np.abs(dec).max() > 0 and np.ptp(dec[:, :, 1]) > 0, "the heads are not live"
