"""GPU: Gumbel MuZero collection on the device, from the root-output kernel to MuZeroCollector.collect().

Nothing here has a tolerance but two bounds taken from the files that own them: the next root's Dirichlet noise to
1 float32 ulp (tests/test_gpu_collect_rng.py: the device's log / cos / pow against numpy's) and the CartPole replay
through oracle/cartpole.py (tests/test_gpu_collector.py: rtol 1e-4, atol 1e-5 on the float32 observations). The
Gumbel tree is bit-exact against tests/gumbel_oracle.py, and everything above it is selection, copying and one
float32 mean.

"The plain API" below is the sequence a caller without the device step runs: initial inference -> the root values
through InverseScalarTransform -> the 6-argument Roots.prepare (Python lists) -> GumbelMuZeroMCTSCtree.search ->
the tree's four getters. Its initial inference is the step's own (DeviceSearchStep.initial: the one-launch
initial inference where the model has one, else the model), so both sides search from the same latents; its search
config is the step's (cfg.fused_search on), so both sides run the same network arithmetic.
"""
import functools

import numpy as np
import pytest
import torch

import bench
import gumbel_oracle as go
import test_gpu_gumbel as tg
import test_gpu_gumbel_fused as tf
from oracle import cartpole
from oracle import collect_rng as cr
from tests.test_collect_rng import GPU_COUNTERS, GPU_SEED
from tests.test_gpu_collect import _model as cartpole_model
from tests.test_gpu_collect_rng import RESET_ATOL, _check_noise

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PERM6 = [[5, 4, 3, 2, 1, 0], [5, 2], [3, 0, 4, 1, 2], [4], [0, 1, 2, 3, 4, 5]]  # ragged, not ascending (PERM9's kind)


def mask_of(legal, A):
    m = np.zeros((len(legal), A), bool)
    for i, l in enumerate(legal):
        m[i, l] = True
    return m


def first_argmax_masked(policy, mask):
    """the reference's action: np.argmax([v for v in np.where(action_mask == 1, improved_policy_probs, 0)])"""
    return np.array([int(np.argmax([v for v in np.where(mask[i], policy[i], 0.0)])) for i in range(len(policy))])


def collect_outputs(t, disc, count=None):
    out = t.collect_outputs(disc, count=count)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_against_siblings(r, A, count=None):
    """lzm_gumbel_collect_outputs == the four getters (children values with the mask applied), bit for bit, and the
    action the first maximum of the masked policy"""
    t, disc = r["roots"].tree, r["disc"]
    got = collect_outputs(t, disc, count)
    sib = tg.device_outputs(r["roots"], disc, A, 1)
    mask = mask_of(r["legal"], A)
    assert np.array_equal(got["distributions"], sib["dist"])
    assert tg.same_bits(got["values"], sib["values"])
    assert tg.same_bits(got["improved_policy"], sib["policies"])
    assert np.array_equal(np.isneginf(sib["children"]), ~mask)
    assert tg.same_bits(got["completed_q"], np.where(mask, sib["children"], np.float32(0)))
    assert (got["improved_policy"][~mask] == 0).all()
    assert np.array_equal(got["action"], first_argmax_masked(sib["policies"], mask))
    assert got["action"].dtype == np.int32 and mask[np.arange(len(mask)), got["action"]].all()
    return got


# ------------------------------------------------------------------------------------------- 1. the root outputs
def test_collect_outputs_match_getters_and_oracle():
    B, A, S, m = 5, 6, 16, 4
    r = tg.run_search(tg.mlp_model(A, seed=3), B, A, S, m, legal=PERM6, noise=True, seed=4)
    tg.assert_matches_restatement(r, A, S, m)  # the getters == gumbel_oracle replayed from the record
    got = check_against_siblings(r, A)
    assert (got["distributions"].clip(0).sum(1) == S).all()
    # ... and so the new kernel against the oracle directly
    rec, legal = r["rec"], r["legal"]
    ot = go.GumbelTree(legal, A)
    ot.prepare(0.25, [r["noises"][i, :len(legal[i])] for i in range(B)], np.zeros(B, np.float32), r["root_value"],
               r["logits0"], r["to_play"])
    for k in range(S):
        ot.traverse(S, m, r["disc"], r["to_play"])
        ot.backprop(k + 1, r["disc"], rec["decoded"][k][:, 0], rec["decoded"][k][:, 1], rec["policy_logits"][k],
                    r["to_play"])
    mask = mask_of(legal, A)
    assert tg.same_bits(got["improved_policy"], ot.policies(r["disc"]))
    assert tg.same_bits(got["completed_q"], np.where(mask, ot.children_values(r["disc"]), np.float32(0)))
    assert np.array_equal(got["action"], first_argmax_masked(ot.policies(r["disc"]), mask))
    # the step counter: advanced by exactly 1 when passed, untouched when null
    count = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    again = collect_outputs(r["roots"].tree, r["disc"], count)
    assert int(count.item()) == 42
    collect_outputs(r["roots"].tree, r["disc"], None)
    assert int(count.item()) == 42
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
    r["roots"].clear()


def test_collect_outputs_lane_limit_and_single_legal_action():
    """A = 64: every lane is an action; one root's only legal action is the last lane"""
    A, S, m = 64, 12, 8
    legal = [list(range(64)), [63], list(range(63, -1, -1)), [7, 63]]
    r = tg.run_search(tg.mlp_model(A, H=64, seed=5), 4, A, S, m, legal=legal, noise=True, seed=6)
    tg.assert_matches_restatement(r, A, S, m)
    got = check_against_siblings(r, A)
    assert got["action"][1] == 63 and got["improved_policy"][1, 63] == 1.0
    assert (got["improved_policy"][1, :63] == 0).all()
    assert got["distributions"][1].tolist() == [S] + [-1] * 63
    r["roots"].clear()


def test_collect_outputs_ties_take_the_first_legal_action():
    """zero-initialised last layers, no noise, full legal lists: equal priors and equal completed Q, so the policy
    row is uniform and the action is the first maximum, action 0"""
    B, A, S, m = 6, 5, 10, 5
    r = tg.run_search(tg.mlp_model(A, zero_heads=True, seed=7), B, A, S, m, noise=False, seed=8)
    got = check_against_siblings(r, A)
    assert (got["improved_policy"] == got["improved_policy"][:, :1]).all()
    assert (got["action"] == 0).all()
    r["roots"].clear()


def test_collect_outputs_refuse_a_muzero_handle():
    from lightzero_amd._lib import LZM_ERR_STATE, LzmError, load, ptr
    from lightzero_amd.tree import DeviceTree
    t = DeviceTree(3, 4, 8, device=DEV)
    f = lambda *s: torch.full(s, 7.0, device=DEV)
    i = lambda *s: torch.full(s, 7, dtype=torch.int32, device=DEV)
    dist, values, cq, pol, act = i(3, 4), f(3), f(3, 4), f(3, 4), i(3)
    count = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    rc = load().lzm_gumbel_collect_outputs(t.h, 0.997, ptr(dist), ptr(values), ptr(cq), ptr(pol), ptr(act), ptr(count),
                                           None)
    torch.cuda.synchronize()
    assert rc == LZM_ERR_STATE
    with pytest.raises(LzmError):
        t.collect_outputs(0.997)
    # refused before any launch: nothing written, the counter untouched
    assert int(count.item()) == 5 and (dist == 7).all() and (values == 7).all() and (act == 7).all()
    t.close()


# ------------------------------------------------------------------------------------------- 2. the raw env steps
def cq_mean(cq):
    """the kernel's float32 mean: the row added up in action order, then divided by A"""
    s = np.zeros(len(cq), np.float32)
    for a in range(cq.shape[1]):
        s = (s + cq[:, a]).astype(np.float32)
    return (s / np.float32(cq.shape[1])).astype(np.float32)


def given_outputs(n, A, seed):
    rng = np.random.default_rng(seed)
    policy = rng.dirichlet([0.5] * A, size=n).astype(np.float32)
    cq = (rng.random((n, A)) * 6).astype(np.float32)
    cq[rng.random((n, A)) < 0.25] = 0  # masked entries
    action = rng.integers(0, A, n).astype(np.int32)  # given, NOT the argmax: the kernel must take it as it is
    visits = rng.integers(0, 9, (n, A)).astype(np.int32)
    value = rng.normal(size=n).astype(np.float32)
    return policy, cq, action, visits, value


@pytest.mark.parametrize("key", GPU_COUNTERS)
def test_cartpole_gumbel_step(key):
    from lightzero_amd._lib import call, ptr, stream_ptr
    n, A, T, E = 7, 2, 2, 1
    policy, cq, action, visits, value = given_outputs(n, A, 11)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    z = functools.partial(torch.zeros, device=DEV)
    rng = np.random.default_rng(12)
    s0 = rng.uniform(-0.05, 0.05, (n, 4))
    s0[5] = [2.4 - 1e-9, 1.0, 0.0, 0.0]  # ends in this step whatever the action: reset from the purpose-3 draw
    state, obs = d(s0), d(s0.astype(np.float32))
    steps, noises = z(n, dtype=torch.int32), z((n, A))
    rec_obs, rec_action = z((n, E, T + 1, 4)), torch.full((n, E, T), -7, dtype=torch.int32, device=DEV)
    rec_reward, rec_visits, rec_value = z((n, E, T)), z((n, E, T, A), dtype=torch.int32), z((n, E, T))
    rec_policy, rec_cq = z((n, E, T, A)), z((n, E, T))
    ep_len, ep_count, ep_return = z((n, E), dtype=torch.int32), z(n, dtype=torch.int32), z((n, E))
    counter = torch.full((1,), int(key), dtype=torch.int64, device=DEV)
    v_d, val_d, a_d, p_d, q_d = d(visits), d(value), d(action), d(policy), d(cq)  # (alive across the launch)
    call("lzm_cartpole_collect_step_gumbel", n, A, T, E, ptr(v_d), ptr(val_d), None, ptr(a_d), ptr(p_d), ptr(q_d),
         ptr(state), ptr(steps), ptr(obs), ptr(noises), 0.3, ptr(rec_obs), ptr(rec_action),
         ptr(rec_reward), ptr(rec_visits), ptr(rec_value), None, ptr(rec_policy), ptr(rec_cq), ptr(ep_len),
         ptr(ep_count), ptr(ep_return), T, GPU_SEED, ptr(counter), stream_ptr())
    torch.cuda.synchronize()
    assert int(counter.item()) == key  # only read
    assert np.array_equal(rec_action[:, 0, 0].cpu().numpy(), action)
    assert np.array_equal(rec_policy[:, 0, 0].cpu().numpy(), policy)
    assert np.array_equal(rec_cq[:, 0, 0].cpu().numpy(), cq_mean(cq))
    assert np.array_equal(rec_visits[:, 0, 0].cpu().numpy(), visits)
    assert np.array_equal(rec_value[:, 0, 0].cpu().numpy(), value)
    assert np.array_equal(rec_obs[:, 0, 0].cpu().numpy(), s0.astype(np.float32))
    assert (rec_action[:, 0, 1] == -7).all() and (rec_policy[:, 0, 1] == 0).all()
    got = state.cpu().numpy()
    done = np.zeros(n, bool)
    for i in range(n):
        want, done[i] = cartpole.step(s0[i], int(action[i]))
        if not done[i]:
            np.testing.assert_allclose(got[i], want, rtol=1e-12, atol=1e-14)
        else:
            np.testing.assert_allclose(rec_obs[i, 0, 1].cpu().numpy(), want.astype(np.float32), rtol=1e-6, atol=1e-9)
    assert done.tolist() == [i == 5 for i in range(n)]
    restated = cr.cartpole_reset(GPU_SEED, n, step=key)
    assert np.abs(got[done] - restated[done]).max() <= RESET_ATOL
    assert np.array_equal(ep_count.cpu().numpy(), done.astype(np.int32))
    assert np.array_equal(steps.cpu().numpy(), (~done).astype(np.int32))
    assert ep_len[5, 0].item() == 1 and ep_return[5, 0].item() == 1.0
    assert np.array_equal(obs.cpu().numpy(), got.astype(np.float32))
    _check_noise(noises, GPU_SEED, n, key, A, 0.3, f"cartpole gumbel key={key}")


@pytest.mark.parametrize("key", GPU_COUNTERS)
def test_breakout_gumbel_step(key):
    from lightzero_amd._lib import call, ptr, stream_ptr
    from tests.test_gpu_collect_rng import _Atari, _first_step
    n, A = 3, 4
    k = _Atari("breakout", n)
    want0 = cr.breakout_reset(GPU_SEED, n)
    assert np.array_equal(k.reset(), want0)
    policy, cq, _, visits, value = given_outputs(n, A, 13)
    action = np.array([1, 3, 2], np.int32)  # FIRE (serves: the purpose-6 draw), LEFT, RIGHT
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rec_policy, rec_cq = torch.zeros((n, k.E, k.T, A), device=DEV), torch.zeros((n, k.E, k.T), device=DEV)
    v_d, val_d, a_d, p_d, q_d = d(visits), d(value), d(action), d(policy), d(cq)  # (alive across the launches)

    def step(max_steps):
        k.counter.fill_(int(key))
        call("lzm_atari_collect_step_gumbel", n, A, k.T, k.E, ptr(v_d), ptr(val_d), None, ptr(a_d), ptr(p_d), ptr(q_d),
             ptr(k.state), ptr(k.steps), ptr(k.cur), ptr(k.obs), ptr(k.noises), 0.3,
             ptr(k.rec_frames), ptr(k.rec_action), ptr(k.rec_reward), ptr(k.rec_visits), ptr(k.rec_value), None,
             ptr(rec_policy), ptr(rec_cq), ptr(k.ep_len), ptr(k.ep_count), None, int(max_steps), GPU_SEED,
             ptr(k.counter), stream_ptr())
        torch.cuda.synchronize()

    step(100)
    assert np.array_equal(k.rec_action[:, 0, 0].cpu().numpy(), action)
    assert np.array_equal(rec_policy[:, 0, 0].cpu().numpy(), policy)
    assert np.array_equal(rec_cq[:, 0, 0].cpu().numpy(), cq_mean(cq))
    assert np.array_equal(k.rec_visits[:, 0, 0].cpu().numpy(), visits)
    assert np.array_equal(k.state.cpu().numpy(), _first_step("breakout", want0, action, GPU_SEED, key)[0])
    _check_noise(k.noises, GPU_SEED, n, key, A, 0.3, f"breakout gumbel key={key}")
    # the in-step reset (max_steps = 1: every episode ends in this step): purpose 3 at the step's key
    k.reset()
    step(1)
    assert np.array_equal(k.state.cpu().numpy(), cr.breakout_reset(GPU_SEED, n, step=key))
    assert (k.ep_count.cpu().numpy() == 1).all() and (k.ep_len.cpu().numpy() == 1).all()


def test_gumbel_steps_refuse_missing_arrays():
    from lightzero_amd._lib import LZM_ERR_ARG, load
    L = load()
    # (null arrays: refused before any launch)
    tail = [0.3] + [None] * 11 + [2, 0, None, None]
    assert L.lzm_cartpole_collect_step_gumbel(*([4, 2, 2, 1] + [None] * 10 + tail)) == LZM_ERR_ARG
    assert L.lzm_atari_collect_step_gumbel(*([4, 4, 2, 1] + [None] * 11 + tail)) == LZM_ERR_ARG


# ------------------------------------------------------------------------------------------- the plain API
def plain_step(model, initial, obs, noises, legal, S, m, scale, fused=True):
    """the module docstring's sequence over one batch -> (dict of the five outputs, the path the search took)"""
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    from lightzero_amd.scaling_transform import InverseScalarTransform
    from lightzero_amd.utils import EasyDict
    B, A = len(legal), noises.shape[1]
    cfg = EasyDict(dict(num_simulations=S, max_num_considered_actions=m, discount_factor=0.997, device=DEV,
                        fused_search=fused, model=dict(support_scale=scale, categorical_distribution=True)))
    mcts = GumbelMuZeroMCTSCtree(cfg)
    with torch.no_grad():
        out = (initial or model).initial_inference(obs)
        pred = InverseScalarTransform(scale, DEV, True)(out.value).detach().cpu().numpy()
        roots = GumbelMuZeroMCTSCtree.roots(B, legal)
        nz = noises.cpu().numpy()
        roots.prepare(0.25, [nz[i, :len(l)].tolist() for i, l in enumerate(legal)], [0.0] * B, list(pred),
                      out.policy_logits.cpu().numpy().tolist(), [-1] * B)
        mcts.search(roots, model, out.latent_state, [-1] * B)
    disc = mcts._discount()
    o = tg.device_outputs(roots, disc, A, 1)
    mask = mask_of(legal, A)
    res = dict(distributions=o["dist"], values=o["values"], improved_policy=o["policies"],
               completed_q=np.where(mask, o["children"], np.float32(0)),
               action=first_argmax_masked(o["policies"], mask))
    roots.clear()
    return res, mcts.last_path


def same_step(got, want, what):
    assert np.array_equal(got["distributions"], want["distributions"]), what
    for k in ("values", "improved_policy", "completed_q"):
        assert tg.same_bits(got[k], want[k]), (what, k)
    assert np.array_equal(got["action"], want["action"]), what


# ------------------------------------------------------------------------------------------- 3. DeviceSearchStep
@pytest.mark.parametrize("F,path", [(16, "fused-mlp"), (24, "generic")])  # head width 24: no multiple of 16, refused
def test_device_search_step_gumbel(F, path):
    from lightzero_amd.collect import DeviceSearchStep
    A, n, S, m, scale = 3, 6, 8, 2, 10
    model = tf.wide_model(A, 32, F, scale, seed=2)
    legal = [[0, 1, 2], [2, 0], [1], [0, 1, 2], [1, 2], [2, 1, 0]]
    rng = np.random.default_rng(0)
    obs_list = [torch.from_numpy(rng.normal(size=(n, 4)).astype(np.float32)).to(DEV) for _ in range(3)]
    nz_list = []
    for _ in range(3):
        nz = np.zeros((n, A), np.float32)
        for i, l in enumerate(legal):
            nz[i, :len(l)] = rng.dirichlet([0.3] * len(l))
        nz_list.append(torch.from_numpy(nz).to(DEV))
    steps = {g: DeviceSearchStep(model, n, S, legal, (4,), DEV, graph=g, support_scale=scale, algo="gumbel",
                                 max_num_considered_actions=m) for g in (True, False)}
    keys = ("distributions", "values", "improved_policy", "completed_q", "action")
    for k, (obs, nz) in enumerate(zip(obs_list, nz_list)):
        outs = {}
        for g, step in steps.items():
            step.set_inputs(obs=obs, noises=nz)
            out = step.step()
            torch.cuda.synchronize()
            outs[g] = {key: out[key].cpu().numpy() for key in keys}
            assert step.mcts.last_path == path
            assert int(step.step_counter.item()) == k + 1
            assert set(out) >= {"distributions", "values", "latent_state", "policy_logits", "value_logits", *keys}
        same_step(outs[True], outs[False], f"step {k}: graph against eager")
        want, took = plain_step(model, steps[True].initial, obs, nz, legal, S, m, scale)
        assert took == path
        same_step(outs[True], want, f"step {k}: against the plain API")
        assert (outs[True]["distributions"].clip(0).sum(1) == S).all()
    assert steps[True].graph is not None and steps[False].graph is None


def test_device_search_step_gumbel_refuses_efficientzero_and_unknown_algo():
    from lightzero_amd.collect import DeviceSearchStep
    from lightzero_amd.model_mlp import EfficientZeroModelMLP
    ez = EfficientZeroModelMLP(observation_shape=4, action_space_size=2).to(DEV).eval()
    with pytest.raises(ValueError):
        DeviceSearchStep(ez, 2, 4, [[0, 1]] * 2, (4,), DEV, algo="gumbel")
    with pytest.raises(ValueError):
        DeviceSearchStep(cartpole_model(), 2, 4, [[0, 1]] * 2, (4,), DEV, algo="sampled")


def test_device_search_step_gumbel_refresh_weights():
    """a changed network is re-packed for the captured one-launch Gumbel search (its _fused takes S)"""
    from lightzero_amd.collect import DeviceSearchStep
    A, n, S, m, scale = 3, 4, 8, 2, 10
    model = tf.wide_model(A, 32, 16, scale, seed=4)
    legal = [list(range(A))] * n
    step = DeviceSearchStep(model, n, S, legal, (4,), DEV, graph=True, support_scale=scale, algo="gumbel",
                            max_num_considered_actions=m)
    rng = np.random.default_rng(1)
    obs = torch.from_numpy(rng.normal(size=(n, 4)).astype(np.float32)).to(DEV)
    nz = torch.from_numpy(rng.dirichlet([0.3] * A, size=n).astype(np.float32)).to(DEV)
    step.set_inputs(obs=obs, noises=nz)
    step.step()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.25)
    out = step.step()
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in ("distributions", "values", "improved_policy", "completed_q", "action")}
    want, took = plain_step(model, step.initial, obs, nz, legal, S, m, scale)
    assert took == "fused-mlp" and step.mcts.last_path == "fused-mlp"
    same_step(got, want, "after the weight change")


# ------------------------------------------------------------------------------------------- 4. DeviceCollector
@functools.lru_cache(maxsize=None)
def cartpole_run():
    """One eager Gumbel collector run on CartPole, shared by the tests below: 4 envs, 8 simulations, m = 2, episodes
    of at most 6 steps, 4 slots, 8 steps (every env finishes an episode at step 6 at the latest). The device's own
    inputs are snapshotted before each step (graph=False, so a step is a Python call): the observation and the
    noise the search is about to read, the running slot and step of every env."""
    from lightzero_amd.collector import DeviceCollector
    n, S, m = 4, 8, 2
    model = cartpole_model(3)
    col = DeviceCollector(model, n, S, device=DEV, max_episode_steps=6, episode_slots=4, seed=9, graph=False,
                          algo="gumbel", max_num_considered_actions=m)
    snaps = []
    for _ in range(8):
        snap = dict(obs=col.search.obs.clone(), noises=col.search.noises.clone(),
                    slot=col.ep_count.cpu().numpy() % col.E, t=col.env.steps.cpu().numpy().copy())
        col.step()
        torch.cuda.synchronize()
        snap["key"] = int(col.search.step_counter.item())
        snaps.append(snap)
    rec = {k: getattr(col, k).cpu().numpy().copy() for k in ("rec_action", "rec_visits", "rec_value", "rec_policy",
                                                             "rec_cq", "rec_frames", "ep_len")}
    block = col.pack_new()
    from lightzero_amd.trajectory import unpack_episodes
    return dict(col=col, model=model, snaps=snaps, rec=rec, block=block, episodes=unpack_episodes(block, col.A), n=n,
                S=S, m=m)


def test_device_collector_gumbel_cartpole_episodes():
    r = cartpole_run()
    eps = r["episodes"]
    assert len(eps) >= 4 and {e["env_id"] for e in eps} == set(range(r["n"]))
    from lightzero_amd.trajectory import LAYOUT_GUMBEL
    assert r["block"].layout == LAYOUT_GUMBEL and r["block"].scalars.shape[1] == 4 + 2 * 2
    for e in eps:
        L = len(e["action_segment"])
        assert 1 <= L <= 6 and e["improved_policy_segment"].shape == (L, 2) and e["visits"].shape == (L, 2)
        assert (e["visits"].sum(1) == r["S"]).all()
        assert np.array_equal(e["action_segment"], np.argmax(e["improved_policy_segment"], axis=1))
        # the actions replayed through the numpy CartPole from o_0 (test_gpu_collector.py's bound for this replay)
        s = e["obs_segment"][0].astype(np.float64)
        for t in range(L):
            s, _ = cartpole.step(s, int(e["action_segment"][t]))
            np.testing.assert_allclose(s.astype(np.float32), e["obs_segment"][t + 1], rtol=1e-4, atol=1e-5)
    # the packed columns are the recorded arrays
    seen = {}
    for e in eps:
        i = e["env_id"]
        k = seen.get(i, 0)
        seen[i] = k + 1
        L = len(e["action_segment"])
        assert r["rec"]["ep_len"][i, k] == L
        assert np.array_equal(e["improved_policy_segment"], r["rec"]["rec_policy"][i, k, :L])
        assert np.array_equal(e["completed_value_segment"], r["rec"]["rec_cq"][i, k, :L])
        assert e["completed_value"] == float(np.mean(r["rec"]["rec_cq"][i, k, :L].astype(np.float64)))


def test_device_collector_gumbel_steps_recompute_with_the_plain_api():
    """every recorded step against the plain API on the DEVICE'S OWN observation and noise (the snapshots): visits,
    value, policy and the mean completed Q bit for bit, the same action. The snapshotted noise of step n + 1 is the
    one the env kernel drew at key n + 1, equal to the restatement (oracle.collect_rng) to 1 float32 ulp."""
    r = cartpole_run()
    col, rec, n = r["col"], r["rec"], r["n"]
    env = np.arange(n)
    for g, snap in enumerate(r["snaps"]):
        want, took = plain_step(r["model"], col.search.initial, snap["obs"], snap["noises"], [[0, 1]] * n, r["S"],
                                r["m"], 300)
        assert took == "fused-mlp"
        at = (env, snap["slot"], snap["t"])
        assert np.array_equal(rec["rec_visits"][at], want["distributions"]), g
        assert tg.same_bits(rec["rec_value"][at], want["values"]), g
        assert tg.same_bits(rec["rec_policy"][at], want["improved_policy"]), g
        assert tg.same_bits(rec["rec_cq"][at], cq_mean(want["completed_q"])), g
        assert np.array_equal(rec["rec_action"][at], want["action"]), g
        assert np.array_equal(rec["rec_frames"][at], snap["obs"].cpu().numpy()), g
        assert snap["key"] == g + 1
        if g:  # the noise this step searched with was drawn by the previous step's env kernel, at its key
            _check_noise(snap["noises"], col.seed, n, r["snaps"][g - 1]["key"], col.A, col.noise_alpha, f"step {g}")
    assert col.search.mcts.last_path == "fused-mlp"


def test_device_collector_gumbel_set_temperature_keeps_the_graph():
    from lightzero_amd.collector import DeviceCollector
    col = DeviceCollector(cartpole_model(3), 4, 8, device=DEV, max_episode_steps=6, episode_slots=4, seed=9,
                          graph=True, algo="gumbel", max_num_considered_actions=2)
    graph = col.search.graph
    assert graph is not None
    col.step()
    state = col.env.state.clone()
    col.set_temperature(0.25, deterministic=True)
    assert col.search.graph is graph and torch.equal(col.env.state, state) and col._epoch == 0


def test_device_collector_gumbel_graph_equals_eager():
    from lightzero_amd.collector import DeviceCollector
    got = {}
    for graph in (True, False):
        col = DeviceCollector(cartpole_model(3), 4, 8, device=DEV, max_episode_steps=6, episode_slots=4, seed=9,
                              graph=graph, algo="gumbel", max_num_considered_actions=2)
        for _ in range(8):
            col.step()
        torch.cuda.synchronize()
        got[graph] = {k: getattr(col, k).cpu().numpy() for k in ("rec_action", "rec_visits", "rec_value",
                                                                  "rec_policy", "rec_cq", "ep_len", "ep_count")}
    for k in got[True]:
        assert np.array_equal(got[True][k], got[False][k]), k
    # the eager run is cartpole_run()'s: same seed, same model
    assert np.array_equal(got[False]["rec_policy"], cartpole_run()["rec"]["rec_policy"])


def test_device_collector_gumbel_breakout():
    from lightzero_amd.collector import DeviceCollector
    col = DeviceCollector(bench.build_conv_model(DEV, seed=3), 2, 4, device=DEV, seed=3, graph=True, poll_every=3,
                          episode_slots=4, max_episode_steps=3, env="breakout", algo="gumbel",
                          max_num_considered_actions=2)
    assert col.search.graph is not None
    episodes, stats = col.collect(2)
    assert col.search.mcts.last_path == "generic"  # the per-simulation loop, captured in the step's graph
    assert len(episodes) >= 2
    for e in episodes:
        L = len(e["action_segment"])
        assert L == 3 and e["obs_segment"].shape == (L + 1, 1, 64, 64)
        p = e["improved_policy_segment"]
        assert p.shape == (L, 4) and p.dtype == np.float32
        assert np.abs(p.astype(np.float64).sum(1) - 1.0).max() <= 1e-6 and (p != 0).all()  # every action legal
        assert np.array_equal(e["action_segment"], np.argmax(p, axis=1))
        assert (e["visits"].sum(1) == 4).all() and np.isfinite(e["completed_value"])


def test_device_collector_gumbel_refuses_pong():
    from lightzero_amd.collector import DeviceCollector
    with pytest.raises(ValueError):
        DeviceCollector(bench.build_ez_model(DEV, seed=3), 2, 4, device=DEV, env="pong", algo="gumbel")


# ------------------------------------------------------------------------------------------- 5. MuZeroCollector
def test_muzero_collector_device_path_with_a_gumbel_policy():
    from lightzero_amd.envs import DeviceCartPoleEnvManager
    from lightzero_amd.policy import GumbelMuZeroCollectPolicy, gumbel_policy_config
    from lightzero_amd.worker import MuZeroCollector
    n, gsl = 4, 3
    cfg = gumbel_policy_config(num_simulations=8, max_num_considered_actions=2, game_segment_length=gsl, device=DEV,
                               num_unroll_steps=1, td_steps=1, n_episode=n, device_episode_slots=4,
                               device_poll_every=2)
    col = MuZeroCollector(env=DeviceCartPoleEnvManager(n, seed=9, max_episode_steps=6),
                          policy=GumbelMuZeroCollectPolicy(cfg, cartpole_model(3)), policy_config=cfg)
    segs, meta = col.collect(n_episode=n, policy_kwargs=dict(temperature=1.0, epsilon=0.0))
    assert col._device is not None and col._device.gumbel and col._device.search.mcts.last_path == "fused-mlp"
    played = col.last_schedule.played
    assert sum(len(p) for p in played) == n
    # the segments' improved policies: each counted episode's policies cut at game_segment_length and padded with
    # the next segment's first num_unroll_steps + td_steps ones, like the root values
    want = []
    for i, eps in enumerate(played):
        for e in eps:
            pol, L = e["improved_policy_segment"], len(e["action_segment"])
            for s in range(0, L, gsl):
                body, nxt = pol[s:s + gsl], pol[s + gsl:s + gsl + 2]
                padded = s + gsl < L or L % gsl == 0
                want.append((i, np.concatenate([body, nxt]) if padded else body))
    assert len(segs) == len(want)
    got = sorted((tuple(np.asarray(s.improved_policy_probs).reshape(-1).tolist()) for s in segs))
    assert got == sorted(tuple(w.reshape(-1).tolist()) for _, w in want)
    for s in segs:
        p = np.asarray(s.improved_policy_probs)
        assert p.shape == (len(s.root_value_segment), 2) and p.shape[0] >= len(s.action_segment)
    # completed_value: in every episode's info, the mean of its recorded step values
    infos = col._episode_info
    assert len(infos) == n and all('completed_value' in d for d in infos)
    means = sorted(float(np.mean(e["completed_value_segment"].astype(np.float64))) for eps in played for e in eps)
    assert sorted(d['completed_value'] for d in infos) == means


# ------------------------------------------------------------------------------------------- 6. the host policy
@pytest.mark.parametrize("mode", ["collect", "eval"])
def test_gumbel_policy_forward_matches_oracle(mode):
    from lightzero_amd.policy import GumbelMuZeroCollectPolicy, gumbel_policy_config
    A, S, m = 3, 8, 2
    masks = [np.array(x) for x in ([1, 1, 1], [0, 1, 1], [1, 0, 0], [1, 1, 0])]
    B = len(masks)
    cfg = gumbel_policy_config(num_simulations=S, max_num_considered_actions=m, device=DEV,
                               model=dict(action_space_size=A, support_scale=10))
    policy = GumbelMuZeroCollectPolicy(cfg, tg.mlp_model(A, seed=6))
    policy.record = True
    rng = np.random.default_rng(5)
    data = torch.from_numpy(rng.normal(size=(B, 4)).astype(np.float32)).to(DEV)
    np.random.seed(77)
    if mode == "collect":
        out = policy.forward(data, masks, temperature=1.0, to_play=[-1] * B)
        keys = ['action', 'visit_count_distributions', 'visit_count_distribution_entropy', 'searched_value',
                'roots_completed_value', 'improved_policy_probs', 'predicted_value', 'predicted_policy_logits']
    else:
        out = policy.eval_mode.forward(data, masks, to_play=[-1] * B)
        keys = ['action', 'visit_count_distributions', 'visit_count_distribution_entropy', 'searched_value',
                'predicted_value', 'predicted_policy_logits']
    assert sorted(out) == list(range(B)) and all(list(out[i].keys()) == keys for i in range(B))
    rec = policy.records[-1]
    assert rec["mode"] == mode and (rec["noises"] is not None) == (mode == "collect")
    legal, sr = rec["legal"], rec["search"]
    assert legal == [[0, 1, 2], [1, 2], [0], [0, 1]]
    disc = np.float32(cfg.discount_factor)
    ot = go.GumbelTree(legal, A)
    ot.prepare(cfg.root_noise_weight, rec["noises"], np.asarray(rec["reward_roots"], np.float32),
               rec["pred_values"].reshape(-1), rec["root_logits"], rec["to_play"])
    for k in range(S):
        x, _, a, _, ln = ot.traverse(S, m, disc, rec["to_play"])
        assert x == sr["x"][k].tolist() and a == sr["action"][k].tolist() and ln == sr["search_len"][k].tolist(), k
        ot.backprop(k + 1, disc, sr["decoded"][k][:, 0], sr["decoded"][k][:, 1], sr["policy_logits"][k], rec["to_play"])
    pol, cv, vals = ot.policies(disc), ot.children_values(disc), ot.values()
    mask = np.array(masks) == 1
    want_action = first_argmax_masked(pol, mask)
    for i in range(B):
        o = out[i]
        assert int(o["action"]) == want_action[i] and mask[i, int(o["action"])]
        assert o["visit_count_distributions"] == ot.distributions()[i]
        assert tg.same_bits(o["searched_value"], vals[i])
        if mode == "collect":
            assert tg.same_bits(o["improved_policy_probs"], pol[i])
            assert tg.same_bits(o["roots_completed_value"], np.where(mask[i], cv[i], np.float32(0)))
    assert tg.same_bits(rec["policies"], pol)
