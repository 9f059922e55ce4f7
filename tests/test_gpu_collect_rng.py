"""GPU: the collect kernels' random layer equals its host restatement (oracle/collect_rng.py) in every row.

The restatement is checked against the Dirichlet, categorical and uniform laws on the CPU
(tests/test_collect_rng.py, which also caps the decision margins of the inputs used here at 1e-9, so a
few double ulps between the device's and numpy's log / cos / pow cannot move a branch). Here the device
must agree with it draw for draw: the sampled action exactly, the Dirichlet noise to 1 float32 ulp per
entry, the reset states and the serve directions, for cartpole_collect_kernel and both templates of
atari_collect_kernel at raw calls (counter values 0, 1 and 2^32 + 5: the counter's high word reaches the
key), and inside DeviceCollector's loop (graph and eager: step n uses key n + 1, the counter advances by one
per step and survives the re-capture after set_temperature).
"""
import functools

import numpy as np
import pytest
import torch

import bench
from oracle import collect_rng as cr
from tests.test_collect_rng import (GPU_ATARI, GPU_ATARI_N, GPU_CARTPOLE_A, GPU_CARTPOLE_ALPHAS, GPU_CARTPOLE_N,
                                    GPU_COUNTERS, GPU_SEED, MARGIN_MIN, TEMPERATURES, tie_rows, visit_rows)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RESET_ATOL = 2e-17  # -0.05 + 0.1 u may be contracted to an fma on the device

_rows = functools.lru_cache(maxsize=None)(visit_rows)
_ties = functools.lru_cache(maxsize=None)(tie_rows)
_not_bit_equal = dict(entries=0, off=0)


def _check_noise(got, seed, n, key, A, alpha, what):
    """device noise == restated Dirichlet to 1 float32 ulp per entry; rows sum to 1, entries >= 0"""
    got = got.cpu().numpy()
    want = cr.dirichlet_noise(seed, n, key, A, alpha)
    assert got.shape == want.shape == (n, A) and got.dtype == np.float32
    assert (got >= 0).all(), what
    assert np.abs(got.astype(np.float64).sum(1) - 1.0).max() <= 1e-6, what
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    _not_bit_equal["entries"] += ulps.size
    _not_bit_equal["off"] += int((ulps != 0).sum())
    bad = np.argwhere(ulps > 1)
    assert len(bad) == 0, f"{what}: {len(bad)} of {ulps.size} noise entries differ by more than 1 ulp; first " \
                          f"(env, action) {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    print(f"{what}: noise entries not bit-equal {int((ulps != 0).sum())} of {ulps.size} "
          f"(running total {_not_bit_equal['off']} of {_not_bit_equal['entries']})")
    return got


# ---------------------------------------------------------------- raw calls: the CartPole kernel
class _CartPole:
    """buffers of one lzm_cartpole_collect_step call (the pattern of test_gpu_collector._raw_step, small T/E)"""

    def __init__(self, n, A, T=2, E=1):
        self.n, self.A, self.T, self.E = n, A, T, E
        z = functools.partial(torch.zeros, device=DEV)
        self.state = z((n, 4), dtype=torch.float64)
        self.steps = z(n, dtype=torch.int32)
        self.obs = z((n, 4))
        self.noises = z((n, A))
        self.value = z(n)
        self.rec_obs = z((n, E, T + 1, 4))
        self.rec_action = z((n, E, T), dtype=torch.int32)
        self.rec_reward = z((n, E, T))
        self.rec_visits = z((n, E, T, A), dtype=torch.int32)
        self.rec_value = z((n, E, T))
        self.ep_len = z((n, E), dtype=torch.int32)
        self.ep_count = z(n, dtype=torch.int32)
        self.counter = z(1, dtype=torch.int64)

    def fresh(self, state=None):
        for t in (self.state, self.steps, self.obs, self.ep_len, self.ep_count, self.rec_action):
            t.zero_()
        self.rec_action.fill_(-7)
        self.noises.fill_(-1.0)
        if state is not None:
            self.state.copy_(torch.from_numpy(state))
            self.obs.copy_(self.state.float())

    def step(self, visits, key, temperature=1.0, deterministic=0, alpha=0.3, max_steps=None, seed=GPU_SEED):
        from lightzero_amd._lib import call, ptr, stream_ptr
        v = torch.from_numpy(np.ascontiguousarray(visits, np.int32)).to(DEV)
        self.counter.fill_(int(key))
        call("lzm_cartpole_collect_step", self.n, self.A, self.T, self.E, ptr(v), ptr(self.value), None,
             ptr(self.state), ptr(self.steps), ptr(self.obs), ptr(self.noises), float(alpha), float(temperature),
             int(deterministic), ptr(self.rec_obs), ptr(self.rec_action), ptr(self.rec_reward), ptr(self.rec_visits),
             ptr(self.rec_value), None, ptr(self.ep_len), ptr(self.ep_count), None,
             self.T if max_steps is None else int(max_steps), seed, ptr(self.counter), stream_ptr())
        torch.cuda.synchronize()
        return self.rec_action[:, 0, 0].cpu().numpy()


@pytest.mark.parametrize("key", GPU_COUNTERS)
@pytest.mark.parametrize("A", GPU_CARTPOLE_A)
def test_cartpole_kernel_actions_and_noise(A, key):
    n = GPU_CARTPOLE_N
    k = _CartPole(n, A)
    v = _rows(A, n)
    for T in TEMPERATURES:
        k.fresh()
        got = k.step(v, key, temperature=T)
        want, margin = cr.select_action(v, T, False, GPU_SEED, key)
        assert margin.min() >= MARGIN_MIN
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"A={A} key={key} T={T}: {len(bad)} of {n} actions differ; first env {bad[0]}: " \
                              f"{got[bad[0]]} != {want[bad[0]]} for visits {v[bad[0]].tolist()}"
        assert np.array_equal(k.rec_visits[:, 0, 0].cpu().numpy(), v)
    _check_noise(k.noises, GPU_SEED, n, key, A, 0.3, f"cartpole A={A} key={key}")
    # deterministic mode: the first maximum on rows with ties
    t = _ties(A, n)
    k.fresh()
    got = k.step(t, key, deterministic=1)
    assert np.array_equal(got, np.argmax(t, axis=1))
    assert np.array_equal(got, cr.select_action(t, 1.0, True, GPU_SEED, key)[0])
    for alpha in GPU_CARTPOLE_ALPHAS.get(A, ())[1:]:  # the alpha < 1 boundary and a no-boost alpha
        k.fresh()
        k.step(t, key, deterministic=1, alpha=alpha)
        _check_noise(k.noises, GPU_SEED, n, key, A, alpha, f"cartpole A={A} key={key} alpha={alpha}")


def test_cartpole_streams_differ_between_steps_and_purposes():
    """what a frozen or truncated counter would break: the draws of keys 0, 1, 2^32 + 0 and 2^32 + 1 all differ"""
    n, A = 512, 6
    k = _CartPole(n, A)
    v = np.tile(np.array([8, 9, 8, 9, 8, 8], np.int32), (n, 1))
    acts, noises = [], []
    for key in (0, 1, 2 ** 32, 2 ** 32 + 1):
        k.fresh()
        acts.append(k.step(v, key))
        noises.append(k.noises.cpu().numpy().copy())
        assert np.array_equal(acts[-1], cr.select_action(v, 1.0, False, GPU_SEED, key)[0])
    for i in range(4):
        for j in range(i + 1, 4):
            assert (acts[i] != acts[j]).mean() > 0.5 and (noises[i] != noises[j]).any(axis=1).all()


@pytest.mark.parametrize("seed", [GPU_SEED, (GPU_SEED + 0x9E3779B9 * 2) & 0xffffffff])
def test_cartpole_reset_entry_point(seed):
    from lightzero_amd._lib import call, ptr, stream_ptr
    n = GPU_CARTPOLE_N
    k = _CartPole(n, 2)
    k.steps.fill_(9)
    call("lzm_cartpole_reset", n, ptr(k.state), ptr(k.steps), ptr(k.obs), seed, stream_ptr())
    torch.cuda.synchronize()
    state = k.state.cpu().numpy()
    assert np.abs(state - cr.cartpole_reset(seed, n)).max() <= RESET_ATOL
    assert np.array_equal(k.obs.cpu().numpy(), state.astype(np.float32))
    assert (k.steps.cpu().numpy() == 0).all()


@pytest.mark.parametrize("key", GPU_COUNTERS)
def test_cartpole_in_step_reset(key):
    """envs that terminate in a collect step (placed just inside the x threshold, moving out) restart from the
    restated purpose-3 draw at the step's key; the others keep their episode"""
    n = GPU_CARTPOLE_N
    k = _CartPole(n, 2)
    out = np.arange(n) % 4 != 2  # both ends of the 128-thread blocks among them
    s0 = np.zeros((n, 4))
    s0[out] = [2.4 - 1e-9, 1.0, 0.0, 0.0]
    k.fresh(s0)
    k.step(np.tile(np.array([25, 25], np.int32), (n, 1)), key)
    state, obs = k.state.cpu().numpy(), k.obs.cpu().numpy()
    want = cr.cartpole_reset(GPU_SEED, n, step=key)
    assert np.abs(state[out] - want[out]).max() <= RESET_ATOL
    assert np.array_equal(obs, state.astype(np.float32))
    assert np.array_equal(k.ep_count.cpu().numpy(), out.astype(np.int32))
    assert np.array_equal(k.steps.cpu().numpy(), (~out).astype(np.int32))
    assert (k.ep_len.cpu().numpy()[out, 0] == 1).all()
    assert (np.abs(state[~out][:, 0]) < 1e-12).all()  # (x = 0 + tau * 0: not reset)
    # the final observation of the finished episode is beyond the threshold
    assert (k.rec_obs[:, 0, 1, 0].cpu().numpy()[out] > 2.4).all()


# ---------------------------------------------------------------- raw calls: the Atari kernel's two templates
class _Atari:
    def __init__(self, game, n, T=2, E=1):
        self.game, self.n, self.A, self.T, self.E = game, n, GPU_ATARI[game], T, E
        self.prefix = "lzm_atari" if game == "breakout" else "lzm_pong"
        A = self.A
        z = functools.partial(torch.zeros, device=DEV)
        self.state = z((n, 16), dtype=torch.int32)
        self.steps = z(n, dtype=torch.int32)
        self.cur = z((n, 64 * 64), dtype=torch.uint8)
        self.obs = z((n, 4, 64, 64))
        self.noises = z((n, A))
        self.value = z(n)
        self.rec_frames = z((n, E, T + 1, 64 * 64), dtype=torch.uint8)
        self.rec_action = z((n, E, T), dtype=torch.int32)
        self.rec_reward = z((n, E, T))
        self.rec_visits = z((n, E, T, A), dtype=torch.int32)
        self.rec_value = z((n, E, T))
        self.ep_len = z((n, E), dtype=torch.int32)
        self.ep_count = z(n, dtype=torch.int32)
        self.counter = z(1, dtype=torch.int64)

    def reset(self, seed=GPU_SEED):
        from lightzero_amd._lib import call, ptr, stream_ptr
        self.state.fill_(77)
        self.steps.fill_(9)
        self.ep_count.zero_()
        self.ep_len.zero_()
        self.rec_action.fill_(-7)
        self.noises.fill_(-1.0)
        call(self.prefix + "_reset", self.n, ptr(self.state), ptr(self.steps), ptr(self.cur), ptr(self.obs), seed,
             stream_ptr())
        torch.cuda.synchronize()
        assert (self.steps.cpu().numpy() == 0).all()
        return self.state.cpu().numpy()

    def step(self, visits, key, temperature=1.0, deterministic=0, alpha=0.3, max_steps=100, seed=GPU_SEED):
        from lightzero_amd._lib import call, ptr, stream_ptr
        v = torch.from_numpy(np.ascontiguousarray(visits, np.int32)).to(DEV)
        self.counter.fill_(int(key))
        call(self.prefix + "_collect_step", self.n, self.A, self.T, self.E, ptr(v), ptr(self.value), None,
             ptr(self.state), ptr(self.steps), ptr(self.cur), ptr(self.obs), ptr(self.noises), float(alpha),
             float(temperature), int(deterministic), ptr(self.rec_frames), ptr(self.rec_action), ptr(self.rec_reward),
             ptr(self.rec_visits), ptr(self.rec_value), None, ptr(self.ep_len), ptr(self.ep_count), None,
             int(max_steps), seed, ptr(self.counter), stream_ptr())
        torch.cuda.synchronize()
        return self.rec_action[:, 0, 0].cpu().numpy(), self.state.cpu().numpy()


def _restated_reset(game, seed, n, step=None):
    return (cr.breakout_reset if game == "breakout" else cr.pong_reset)(seed, n, step)


def _first_step(game, s0, action, seed, key):
    """the state after one step from a fresh reset (nothing in play yet): the paddle moves, FIRE serves the
    ball in the direction of the restated purpose-6 bits, anything else idles (at_step / pg_step's first branch)"""
    n = len(s0)
    s = s0.copy()
    b0, b1 = cr.serve_bits(seed, n, key)
    if game == "breakout":
        s[:, 0] = np.clip(s0[:, 0] + 3 * (action == 2) - 3 * (action == 3), 2, 54)
        fire = action == 1
        s[fire, 1], s[fire, 2] = s[fire, 0] + 3, 50
        s[fire, 3], s[fire, 4] = np.where(b0[fire], 1, -1), -1
    else:
        up, down = (action == 2) | (action == 4), (action == 3) | (action == 5)
        s[:, 0] = np.clip(s0[:, 0] - 3 * up + 3 * down, 2, 54)
        fire = (action == 1) | (action == 4) | (action == 5)
        s[fire, 1], s[fire, 2] = 31, 31
        s[fire, 3], s[fire, 4] = np.where(b0[fire], 1, -1), np.where(b1[fire], 1, -1)
    s[fire, 5] = 1
    s[~fire, 10] = 1  # an idle step counted
    return s, fire


@pytest.mark.parametrize("key", GPU_COUNTERS)
@pytest.mark.parametrize("game", list(GPU_ATARI))
def test_atari_kernel_draws(game, key):
    n, A = GPU_ATARI_N, GPU_ATARI[game]
    k = _Atari(game, n)
    want0 = _restated_reset(game, GPU_SEED, n)
    # ---- the reset entry point: paddle words as restated, every other word as at_reset / pg_reset set it
    assert np.array_equal(k.reset(), want0)
    # ---- FIRE from a fresh reset: the serve follows the purpose-6 bits, both directions occur
    fire_actions = np.array([1] if game == "breakout" else [1, 4, 5])[np.arange(n) % (1 if game == "breakout" else 3)]
    v = np.zeros((n, A), np.int32)
    v[np.arange(n), fire_actions] = 50
    act, state = k.step(v, key, deterministic=1)
    assert np.array_equal(act, fire_actions)
    want, fire = _first_step(game, want0, act, GPU_SEED, key)
    assert fire.all() and np.array_equal(state, want)
    for word in ((3,) if game == "breakout" else (3, 4)):
        assert set(np.unique(state[:, word])) == {-1, 1}
    _check_noise(k.noises, GPU_SEED, n, key, A, 0.3, f"{game} key={key}")
    # ---- sampled actions at three temperatures (and whatever they serve)
    v = _rows(A, n)
    for T in TEMPERATURES:
        assert np.array_equal(k.reset(), want0)
        act, state = k.step(v, key, temperature=T)
        want_act, margin = cr.select_action(v, T, False, GPU_SEED, key)
        assert margin.min() >= MARGIN_MIN
        bad = np.flatnonzero(act != want_act)
        assert len(bad) == 0, f"{game} key={key} T={T}: {len(bad)} of {n} actions differ; first env {bad[0]}: " \
                              f"{act[bad[0]]} != {want_act[bad[0]]} for visits {v[bad[0]].tolist()}"
        assert np.array_equal(state, _first_step(game, want0, act, GPU_SEED, key)[0])
        _check_noise(k.noises, GPU_SEED, n, key, A, 0.3, f"{game} key={key} T={T}")
    # ---- deterministic mode with ties
    t = _ties(A, n)
    k.reset()
    act, _ = k.step(t, key, deterministic=1)
    assert np.array_equal(act, np.argmax(t, axis=1))
    # ---- the in-loop reset (max_steps = 1: every env's episode ends in this step): purpose 3 at the step's key
    k.reset()
    _, state = k.step(t, key, deterministic=1, max_steps=1)
    want3 = _restated_reset(game, GPU_SEED, n, step=key)
    assert np.array_equal(state, want3)
    assert not np.array_equal(want3[:, 0], want0[:, 0])
    assert (k.ep_count.cpu().numpy() == 1).all() and (k.steps.cpu().numpy() == 0).all()
    assert (k.ep_len.cpu().numpy() == 1).all()


def test_atari_reset_entry_point_other_seed():
    seed = (GPU_SEED + 0x9E3779B9) & 0xffffffff
    for game in GPU_ATARI:
        k = _Atari(game, GPU_ATARI_N)
        assert np.array_equal(k.reset(seed), _restated_reset(game, seed, GPU_ATARI_N))


# ---------------------------------------------------------------- in the loop
def _loop_check(col, steps, reset_fn, temperature):
    """`steps` single step() calls: the counter advances by one per step; with key = its new value, the
    recorded action, the next root's noise and the restarted envs' states are the restatement's at that key"""
    n, A, E, seed = col.n, col.A, col.E, col.seed
    ended = 0
    last_noise = col.search.noises.cpu().numpy().copy()
    for _ in range(steps):
        count0 = int(col.search.step_counter.item())
        ep0, t0 = col.ep_count.cpu().numpy().copy(), col.env.steps.cpu().numpy().copy()
        col.step()
        torch.cuda.synchronize()
        key = int(col.search.step_counter.item())
        assert key == count0 + 1
        slot = ep0 % E
        env = np.arange(n)
        visits = col.rec_visits.cpu().numpy()[env, slot, t0]
        assert (visits.sum(1) == col.S).all()
        want, margin = cr.select_action(visits, temperature, False, seed, key)
        assert margin.min() >= MARGIN_MIN  # (a condition on the inputs: change the seed if it ever fails)
        got = col.rec_action.cpu().numpy()[env, slot, t0]
        assert np.array_equal(got, want), (key, got.tolist(), want.tolist(), visits.tolist())
        noise = _check_noise(col.search.noises, seed, n, key, A, col.noise_alpha, f"loop key={key}")
        assert (noise != last_noise).any(axis=1).all(), f"key {key}: the noise of consecutive steps is the same"
        last_noise = noise.copy()
        done = col.ep_count.cpu().numpy() != ep0
        if done.any():
            state = col.env.state.cpu().numpy()
            restated = reset_fn(seed, n, step=key)
            if state.dtype == np.float64:
                assert np.abs(state[done] - restated[done]).max() <= RESET_ATOL
            else:
                assert np.array_equal(state[done], restated[done])
            assert (col.env.steps.cpu().numpy()[done] == 0).all()
        ended += int(done.sum())
    return ended


def _set_temperature_check(col, graph, reset_fn):
    """set_temperature re-captures the graph: the counter survives it, the envs restart from the epoch's seed
    (graph mode; eager mode has nothing to re-capture and the episodes go on), the next step samples at the
    new temperature with the next key"""
    count = int(col.search.step_counter.item())
    before = col.env.state.cpu().numpy().copy()
    col.set_temperature(0.5)
    torch.cuda.synchronize()
    assert int(col.search.step_counter.item()) == count
    state = col.env.state.cpu().numpy()
    if graph:
        assert col._epoch == 1
        restated = reset_fn((col.seed + 0x9E3779B9 * col._epoch) & 0xffffffff, col.n)
        if state.dtype == np.float64:
            assert np.abs(state - restated).max() <= RESET_ATOL
        else:
            assert np.array_equal(state, restated)
        assert (col.ep_count.cpu().numpy() == 0).all() and (col.env.steps.cpu().numpy() == 0).all()
    else:
        assert np.array_equal(state, before)
    _loop_check(col, 2, reset_fn, 0.5)
    assert int(col.search.step_counter.item()) == count + 2


@pytest.mark.parametrize("graph", [True, False])
def test_cartpole_loop_follows_the_restatement(graph):
    from lightzero_amd.collector import DeviceCollector
    from tests.test_gpu_collect import _model
    col = DeviceCollector(_model(), 16, 12, device=DEV, seed=9, graph=graph, poll_every=2)
    assert int(col.search.step_counter.item()) == 0
    state = col.env.state.cpu().numpy()
    assert np.abs(state - cr.cartpole_reset(col.seed, col.n)).max() <= RESET_ATOL
    ended = _loop_check(col, 40, cr.cartpole_reset, 1.0)
    assert int(col.search.step_counter.item()) == 40
    assert ended >= 1, "no CartPole episode ended within 40 steps"
    _set_temperature_check(col, graph, cr.cartpole_reset)


@pytest.mark.parametrize("graph", [True, False])
def test_breakout_loop_follows_the_restatement(graph):
    from lightzero_amd.collector import DeviceCollector
    col = DeviceCollector(bench.build_conv_model(DEV, seed=3), 8, 8, device=DEV, seed=3, graph=graph, poll_every=4,
                          episode_slots=8, max_episode_steps=5, env="breakout")
    assert np.array_equal(col.env.state.cpu().numpy(), cr.breakout_reset(col.seed, col.n))
    ended = _loop_check(col, 12, cr.breakout_reset, 1.0)
    assert int(col.search.step_counter.item()) == 12
    assert ended >= 2 * col.n  # max_episode_steps = 5: every env restarted at steps 5 and 10
    _set_temperature_check(col, graph, cr.breakout_reset)
