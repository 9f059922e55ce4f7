"""GPU: the collect kernels at the game and recording edges play never reaches.

atari_collect_kernel<GAME, GUMBEL> (csrc/lzm_atari.h) and cartpole_collect_kernel<GUMBEL> (csrc/lzm_collect.h)
write every trajectory the learner sees. The random layer is pinned draw for draw by test_gpu_collect_rng.py; the
game rules were checked only along what a randomly initialised network happens to play. Here the state is
written directly (int32[n][16], or double[n][4]), the action is chosen by one-hot visits with deterministic = 1
(or by the Gumbel entry's action[n]), and every buffer of the launch is compared as a whole, by bits, with a numpy
restatement of the step: the restated game (oracle/breakout_synth.py, oracle/pong_synth.py, oracle/cartpole.py),
the restated serve and reset draws (oracle/collect_rng.py) and the record step restated below. The buffers start
filled with canaries, so a write outside the step's own elements shows as well.

 1. One launch per game and entry point with env i holding case i of tests/env_cases.py (the CPU test
    tests/test_env_cases.py asserts that each case shows the edge it is named for).
 2. Two lockstep runs that record nothing (T = 2, max_steps large): 300 steps of a ball-tracking Breakout policy
    and 1,400 steps of uniform Pong actions, long enough for a 21-point finish; all state words after every step.
 3. The recording guards of the three kernels through their five entry points: the slot after a wrap, t < T,
    the final frame's nt <= T, the nullable arrays, the Gumbel action clamp and records, refused arguments.

Every comparison is exact: integers, bytes and float bit patterns. The next root's noise is compared (to 1 ulp)
by test_gpu_collect_rng.py; here it only has to be written.
"""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import cartpole
from oracle import collect_rng as cr
from tests import env_cases as ec
from tests.test_gpu_collect_rng import _Atari

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
KEY = 2 ** 32 + 77  # the step key of the single launches (its high word reaches the Philox counter)
CANARY = dict(rec_frames=0xA5, rec_action=-7, rec_reward=-9.5, rec_visits=-3, rec_value=-8.25, rec_pred=-6.5,
              rec_policy=-4.5, rec_cq=-2.5, ep_len=-5, ep_return=-77.5, noises=-1.0, rec_obs=-11.5)
COMPARED = ("state", "steps", "cur", "obs", "rec_frames", "rec_action", "rec_reward", "rec_visits", "rec_value",
            "rec_pred", "rec_policy", "rec_cq", "ep_len", "ep_count", "ep_return")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _assert_same(got, want, what):
    """whole buffers, by bits"""
    for name in want:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(_bits(g) != _bits(w))
        assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} elements; first at {bad[0].tolist()}: " \
                              f"{g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


def cq_mean(row):
    """the float32 sum in action order, divided by A (record_gumbel)"""
    s = np.float32(0.0)
    for v in row:
        s = np.float32(s + np.float32(v))
    return np.float32(s / np.float32(len(row)))


# ------------------------------------------------------------------------------------------ the Atari kernels
class _Edge(_Atari):
    """_Atari's buffers plus the nullable and Gumbel ones, every record buffer filled with its canary"""

    def __init__(self, game, n, T, E):
        super().__init__(game, n, T=T, E=E)
        f = functools.partial(torch.zeros, device=DEV)
        self.ep_return, self.rec_pred, self.rec_cq = f((n, E)), f((n, E, T)), f((n, E, T))
        self.rec_policy = f((n, E, T, self.A))
        for name, v in CANARY.items():
            if hasattr(self, name):
                getattr(self, name).fill_(v)

    def put(self, words, steps, ep_count, rng):
        """the states, their restated render as the newest frame, four different known frames in the stack"""
        render = ec.synth(self.game).render
        self.state.copy_(_dev(np.asarray(words, np.int32)))
        self.steps.copy_(_dev(np.asarray(steps, np.int32)))
        self.ep_count.copy_(_dev(np.asarray(ep_count, np.int32)))
        cur = np.stack([render(ec.state_of(self.game, w)[0]).reshape(-1) for w in words])
        self.cur.copy_(_dev(cur))
        self.obs.copy_(_dev(rng.random((self.n, 4, 64, 64), dtype=np.float32)))

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in COMPARED}

    def launch(self, visits, value, key, max_steps, pred=None, ret=True, gumbel=None):
        """one collect step; gumbel = (action, policy, completed_q) takes the Gumbel entry point"""
        from lightzero_amd._lib import call, ptr, stream_ptr
        keep = [_dev(visits), _dev(value), None if pred is None else _dev(pred)]
        self.counter.fill_(int(key))
        head = [self.n, self.A, self.T, self.E, ptr(keep[0]), ptr(keep[1]), ptr(keep[2])]
        tail = [ptr(self.ep_len), ptr(self.ep_count), ptr(self.ep_return) if ret else None, int(max_steps), SEED,
                ptr(self.counter), stream_ptr()]
        env = [ptr(self.state), ptr(self.steps), ptr(self.cur), ptr(self.obs), ptr(self.noises), 0.3]
        rec = [ptr(self.rec_frames), ptr(self.rec_action), ptr(self.rec_reward), ptr(self.rec_visits),
               ptr(self.rec_value), None if pred is None else ptr(self.rec_pred)]
        if gumbel is None:
            call(self.prefix + "_collect_step", *head, *env, 1.0, 1, *rec, *tail)
        else:
            keep += [_dev(np.asarray(g)) for g in gumbel]
            call("lzm_atari_collect_step_gumbel", *head, *[ptr(g) for g in keep[3:]], *env, *rec, ptr(self.rec_policy),
                 ptr(self.rec_cq), *tail)
        torch.cuda.synchronize()
        assert int(self.counter.item()) == key  # only read


def restate_atari_step(game, h, action, visits, value, key, T, E, max_steps, pred=None, ret=True, gumbel=None):
    """the collect step on host copies `h` of the buffers (in place): record the transition into slot
    ep_count % E while t < T, step the restated game under the restated serve draw, and either go on (the stack
    shifts by one frame) or end the episode (length, return, the final frame while nt <= T, the restated reset)"""
    game_mod = ec.synth(game)
    n = len(action)
    b0, b1 = cr.serve_bits(SEED, n, key)
    reset = (cr.breakout_reset if game == "breakout" else cr.pong_reset)(SEED, n, step=key)
    sc = np.float32(1.0 / 255.0)  # a product with the rounded reciprocal, not a division
    dones = np.zeros(n, bool)
    for i in range(n):
        s0, score = ec.state_of(game, h["state"][i])
        a = int(action[i])
        s1, pts, term = game_mod.step(s0, a, ec.draw_from_bits(game, b0[i], b1[i]))
        e, t = int(h["ep_count"][i]) % E, int(h["steps"][i])
        if t < T:
            h["rec_action"][i, e, t] = a
            h["rec_visits"][i, e, t] = visits[i]
            h["rec_value"][i, e, t] = value[i]
            h["rec_reward"][i, e, t] = np.sign(pts)
            h["rec_frames"][i, e, t] = h["cur"][i]
            if pred is not None:
                h["rec_pred"][i, e, t] = pred[i]
            if gumbel is not None:
                h["rec_policy"][i, e, t] = gumbel[1][i]
                h["rec_cq"][i, e, t] = cq_mean(gumbel[2][i])
        nt = t + 1
        score += int(pts)
        dones[i] = term or nt >= max_steps
        if dones[i]:
            h["ep_len"][i, e] = nt
            if ret:
                h["ep_return"][i, e] = np.float32(score)
            h["ep_count"][i] += 1
            if nt <= T:
                h["rec_frames"][i, e, nt] = game_mod.render(s1).reshape(-1)
            h["state"][i], h["steps"][i] = reset[i], 0
            frame = game_mod.render(ec.state_of(game, reset[i])[0]).reshape(-1)
            h["obs"][i, :] = (frame.astype(np.float32) * sc).reshape(64, 64)
        else:
            h["state"][i], h["steps"][i] = ec.words(game, s1, score), nt
            frame = game_mod.render(s1).reshape(-1)
            h["obs"][i, :3] = h["obs"][i, 1:].copy()
            h["obs"][i, 3] = (frame.astype(np.float32) * sc).reshape(64, 64)
        h["cur"][i] = frame
    return dones


def _one_hot(action, A, other=False):
    """visits whose first maximum is `action` (other: some different action, for the Gumbel entry)"""
    v = np.full((len(action), A), 2, np.int32)
    v[np.arange(len(action)), (np.asarray(action) + (1 if other else 0)) % A] = 50
    return v


@pytest.mark.parametrize("game,entry", [("breakout", "plain"), ("breakout", "gumbel"), ("pong", "plain")])
def test_case_table_on_the_device(game, entry):
    """env i holds case i: state, cur, obs, steps, ep_count before; every buffer after"""
    cases = ec.CASES[game]
    n, T, E = len(cases), ec.MAX_STEPS, 2
    rng = np.random.default_rng(3)
    k = _Edge(game, n, T, E)
    A = k.A
    k.put([ec.words(game, c.state, c.score) for c in cases], [c.steps for c in cases], [c.ep_count for c in cases], rng)
    action = np.array([c.action for c in cases], np.int32)
    value = rng.normal(size=n).astype(np.float32)
    gumbel, pred = None, None
    if entry == "gumbel":  # the visits' argmax is another action: the kernel must obey action[n]
        visits = _one_hot(action, A, other=True)
        gumbel = (action, rng.dirichlet([0.5] * A, size=n).astype(np.float32), (rng.random((n, A)) * 6).astype(np.float32))
    else:
        visits = _one_hot(action, A)
        pred = rng.normal(size=n).astype(np.float32)
    want = k.host()
    dones = restate_atari_step(game, want, action, visits, value, KEY, T, E, ec.MAX_STEPS, pred=pred, gumbel=gumbel)
    # the restatement's results are the ones the CPU test pins (the device's serve draw among its draws)
    b0, b1 = cr.serve_bits(SEED, n, KEY)
    served = set()
    for i, c in enumerate(cases):
        d = ec.draw_from_bits(game, b0[i], b1[i])
        _, _, term = ec.check_case(game, c, d)
        assert dones[i] == ec.done(c, term)
        if ec.serves(game, c.state, c.action):
            served.add(d)
    assert served == set(ec.draws(game)), "the launch does not see every value of the serve draw"
    assert 3 <= dones.sum() < n
    k.launch(visits, value, KEY, ec.MAX_STEPS, pred=pred, gumbel=gumbel)
    got = k.host()
    for i in np.argwhere(_bits(got["state"]) != _bits(want["state"]))[:, 0][:1]:  # name the case
        raise AssertionError(f"{game} {entry}: case {cases[i].name}: state {got['state'][i].tolist()} != "
                             f"{want['state'][i].tolist()}")
    _assert_same(got, want, f"{game} {entry}")
    assert (k.noises.cpu().numpy() >= 0).all()


def _lockstep(game, n, steps, policy):
    """`steps` launches that record nothing (T = 2, the step counts run past it): all state words after every step"""
    ref = ec.run_restated(game, n, steps, policy, seed=SEED, max_steps=10 ** 6)
    k = _Atari(game, n, T=2, E=1)
    first = k.reset(SEED)
    assert np.array_equal(first, ref["first_words"])
    A = k.A
    t0 = time.perf_counter()
    for t in range(steps):
        _, state = k.step(_one_hot(ref["actions"][t], A), 1 + t, deterministic=1, max_steps=10 ** 6, seed=SEED)
        if not np.array_equal(state, ref["words"][t]):
            i = int(np.argwhere(state != ref["words"][t])[0, 0])
            raise AssertionError(f"{game} lockstep: step {t} env {i} action {ref['actions'][t, i]}: "
                                 f"{state[i].tolist()} != {ref['words'][t, i].tolist()}")
    torch.cuda.synchronize()
    print(f"{game} lockstep: {steps} steps of {n} envs in {time.perf_counter() - t0:.2f} s; met " +
          ", ".join(f"{m} {ref[m]}" for m in ("terminated", "score_ends", "points", "upper_rows", "agent_points")))
    assert np.array_equal(k.steps.cpu().numpy(), ref["steps"][-1])
    return ref


def test_breakout_lockstep_with_a_ball_tracking_policy():
    ref = _lockstep("breakout", 8, 300, ec.BreakoutTracker(8, seed=7))
    assert ref["terminated"] >= 8 and ref["upper_rows"] >= 1


def test_pong_lockstep_reaches_a_21_point_finish():
    acts = ec.pong_actions(8, 1400)
    ref = _lockstep("pong", 8, 1400, lambda t, states: acts[t])
    assert ref["score_ends"] >= 1, "no env's episode terminates by score"


# ------------------------------------------------------------------------------------------ recording edges
REC_T, REC_MAX = 4, 9


def _rec_envs(game, E):
    """(words, steps, ep_count, action) of the recording launch: idle envs in every slot, at the steps around T,
    and envs whose episode ends with nt == T, nt == T + 1 and at the truncation"""
    if game == "breakout":
        idle, lost = ec._idle(30, 2), ec._bk(bx=20, by=62, vx=1, vy=1)
    else:
        idle = ec._pg(in_play=0, idle=2, bx=0, by=0, vx=0, vy=0)
        lost = ec._pg(paddle=2, bx=62, by=50, vx=1, vy=1, me=4, them=20)
    rows = [(idle, 0, c) for c in (0, E - 1, E, 2 * E + 1)]
    rows += [(idle, s, 1) for s in (0, 3, 4, 7, 8)]          # 8: truncated with nt == 9 > T
    rows += [(lost, 3, c) for c in (0, 2 * E + 1)]            # nt == T: the final frame goes to row T
    rows += [(lost, 4, 1), (lost, 7, E)]                      # nt == T + 1 and later: not written; ep_len all the same
    rows += [(lost, 0, 0), (idle, 2, E + 1)]
    score = 3 if game == "breakout" else -16
    return ([ec.words(game, s, score) for s, _, _ in rows], [t for _, t, _ in rows], [c for _, _, c in rows],
            np.full(len(rows), ec.NOOP, np.int32))


@pytest.mark.parametrize("pred,ret", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("E", [3, 1])
@pytest.mark.parametrize("game,entry", [("breakout", "plain"), ("breakout", "gumbel"), ("pong", "plain")])
def test_atari_recording_edges(game, entry, E, pred, ret):
    words, steps, counts, action = _rec_envs(game, E)
    rng = np.random.default_rng(17)
    gumbel = None
    if entry == "gumbel":  # five more envs: action ids outside the set are clamped, recorded and executed clamped
        given = np.array([-1, 0, 3, 4, 9], np.int32)
        words += [ec.words(game, ec._idle(30, 2))] * 5
        steps, counts = steps + [1] * 5, counts + [0] * 5
        action = np.concatenate([action, np.clip(given, 0, 3)])
    n = len(words)
    k = _Edge(game, n, REC_T, E)
    A = k.A
    k.put(words, steps, counts, rng)
    value = rng.normal(size=n).astype(np.float32)
    pv = rng.normal(size=n).astype(np.float32) if pred else None
    if entry == "gumbel":
        raw = np.concatenate([action[:n - 5], given])
        cq = (rng.random((n, A)) * 6).astype(np.float32)
        cq[0], cq[1] = [1e8, 1, -1e8, 1], [1, 1e8, 1, -1e8]  # the order of the float32 sum matters
        assert cq_mean(cq[0]) == 0.25 and cq_mean(cq[1]) == 0.0 and np.float32(cq[0].astype(np.float64).mean()) == 0.5
        gumbel = (raw, rng.dirichlet([0.5] * A, size=n).astype(np.float32), cq)
        visits = _one_hot(action, A, other=True)
    else:
        visits = _one_hot(action, A)
    want = k.host()
    dones = restate_atari_step(game, want, action, visits, value, KEY + 1, REC_T, E, REC_MAX, pred=pv, ret=ret,
                               gumbel=gumbel)
    assert dones.sum() == 6
    k.launch(visits, value, KEY + 1, REC_MAX, pred=pv, ret=ret, gumbel=gumbel)
    got = k.host()
    _assert_same(got, want, f"{game} {entry} E={E}")
    # what the restatement must have produced for the named edges
    assert got["ep_len"][11, 1 % E] == 5 and (got["rec_frames"][11, 1 % E] == CANARY["rec_frames"]).all()  # nt == T + 1
    assert got["ep_len"][9, 0] == 4 and (got["rec_frames"][9, 0, REC_T] != CANARY["rec_frames"]).any()     # nt == T
    assert got["ep_len"][8, 1 % E] == 9 and (got["rec_action"][8] == CANARY["rec_action"]).all()           # truncated
    assert (got["ep_return"] != np.float32(CANARY["ep_return"])).sum() == (6 if ret else 0)
    assert (got["rec_pred"] != np.float32(CANARY["rec_pred"])).sum() == (sum(s < REC_T for s in steps) if pred else 0)
    if entry == "gumbel":
        assert got["rec_action"][n - 5:, 0, 1].tolist() == [0, 0, 3, 3, 3]
        assert got["state"][n - 5:, 0].tolist() == [30, 30, 27, 27, 27]  # LEFT moved the paddle: the clamped id ran


# ---- CartPole: one thread per env; theta = theta_dot = 0 keeps the restated physics in exact arithmetic
class _Cart:
    def __init__(self, n, A, T, E):
        self.n, self.A, self.T, self.E = n, A, T, E
        f = functools.partial(torch.zeros, device=DEV)
        self.state, self.steps, self.obs = f((n, 4), dtype=torch.float64), f(n, dtype=torch.int32), f((n, 4))
        self.noises, self.rec_obs = f((n, A)), f((n, E, T + 1, 4))
        self.rec_action, self.rec_reward = f((n, E, T), dtype=torch.int32), f((n, E, T))
        self.rec_visits, self.rec_value = f((n, E, T, A), dtype=torch.int32), f((n, E, T))
        self.rec_pred, self.rec_policy, self.rec_cq = f((n, E, T)), f((n, E, T, A)), f((n, E, T))
        self.ep_len, self.ep_count, self.ep_return = f((n, E), dtype=torch.int32), f(n, dtype=torch.int32), f((n, E))
        self.counter = f(1, dtype=torch.int64)
        for name, v in CANARY.items():
            if hasattr(self, name):
                getattr(self, name).fill_(v)

    NAMES = ("state", "steps", "obs", "rec_obs", "rec_action", "rec_reward", "rec_visits", "rec_value", "rec_pred",
             "rec_policy", "rec_cq", "ep_len", "ep_count", "ep_return")

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in self.NAMES}

    def launch(self, visits, value, key, max_steps, pred=None, ret=True, gumbel=None):
        from lightzero_amd._lib import call, ptr, stream_ptr
        keep = [_dev(visits), _dev(value), None if pred is None else _dev(pred)]
        self.counter.fill_(int(key))
        head = [self.n, self.A, self.T, self.E, ptr(keep[0]), ptr(keep[1]), ptr(keep[2])]
        env = [ptr(self.state), ptr(self.steps), ptr(self.obs), ptr(self.noises), 0.3]
        rec = [ptr(self.rec_obs), ptr(self.rec_action), ptr(self.rec_reward), ptr(self.rec_visits), ptr(self.rec_value),
               None if pred is None else ptr(self.rec_pred)]
        tail = [ptr(self.ep_len), ptr(self.ep_count), ptr(self.ep_return) if ret else None, int(max_steps), SEED,
                ptr(self.counter), stream_ptr()]
        if gumbel is None:
            call("lzm_cartpole_collect_step", *head, *env, 1.0, 1, *rec, *tail)
        else:
            keep += [_dev(np.asarray(g)) for g in gumbel]
            call("lzm_cartpole_collect_step_gumbel", *head, *[ptr(g) for g in keep[3:]], *env, *rec,
                 ptr(self.rec_policy), ptr(self.rec_cq), *tail)
        torch.cuda.synchronize()


def restate_cartpole_step(h, action, visits, value, key, T, E, max_steps, pred=None, ret=True, gumbel=None):
    n = len(action)
    reset = cr.cartpole_reset(SEED, n, step=key)
    dones = np.zeros(n, bool)
    for i in range(n):
        a = int(action[i])
        e, t = int(h["ep_count"][i]) % E, int(h["steps"][i])
        if t < T:
            h["rec_obs"][i, e, t] = h["obs"][i]
            h["rec_action"][i, e, t] = a
            h["rec_visits"][i, e, t] = visits[i]
            h["rec_value"][i, e, t] = value[i]
            h["rec_reward"][i, e, t] = 1.0
            if pred is not None:
                h["rec_pred"][i, e, t] = pred[i]
            if gumbel is not None:
                h["rec_policy"][i, e, t] = gumbel[1][i]
                h["rec_cq"][i, e, t] = cq_mean(gumbel[2][i])
        s1, term = cartpole.step(h["state"][i], a)
        nt = t + 1
        dones[i] = term or nt >= max_steps
        if dones[i]:
            if nt <= T:
                h["rec_obs"][i, e, nt] = s1.astype(np.float32)
            h["ep_len"][i, e] = nt
            if ret:
                h["ep_return"][i, e] = np.float32(nt)  # the reward sum, 1 per step
            h["ep_count"][i] += 1
            h["state"][i], h["steps"][i] = reset[i], 0
        else:
            h["state"][i], h["steps"][i] = s1, nt
        h["obs"][i] = h["state"][i].astype(np.float32)
    return dones


@pytest.mark.parametrize("pred,ret", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("E", [3, 1])
@pytest.mark.parametrize("entry,A", [("plain", 2), ("gumbel", 2), ("gumbel", 1), ("gumbel", 4)])
def test_cartpole_recording_edges(entry, A, E, pred, ret):
    idle, out = [0.25, 0.5, 0.0, 0.0], [2.4 - 1e-9, 1.0, 0.0, 0.0]  # `out` is one step from the x threshold
    rows = [(idle, 0, c) for c in (0, E - 1, E, 2 * E + 1)] + [(idle, s, 1) for s in (0, 3, 4, 7, 8)]
    rows += [(out, 3, 0), (out, 3, 2 * E + 1), (out, 4, 1), (out, 7, E), (out, 0, 0), (idle, 2, E + 1)]
    rng = np.random.default_rng(19)
    action = (np.arange(len(rows)) % A).astype(np.int32)
    gumbel = None
    if entry == "gumbel":
        given = np.array([-1, 0, A - 1, A, A + 5], np.int32)
        rows += [(idle, 1, 0)] * 5
        action = np.concatenate([action, np.clip(given, 0, A - 1)])
    n = len(rows)
    k = _Cart(n, A, REC_T, E)
    state = np.array([r[0] for r in rows], np.float64) + np.arange(n)[:, None] * np.array([1e-3, 0, 0, 0])
    state[[r[0] is out for r in rows]] = out
    k.state.copy_(_dev(state))
    k.obs.copy_(_dev(rng.random((n, 4), dtype=np.float32)))  # (known values, not the state's: rec_obs copies them)
    k.steps.copy_(_dev(np.array([r[1] for r in rows], np.int32)))
    k.ep_count.copy_(_dev(np.array([r[2] for r in rows], np.int32)))
    value = rng.normal(size=n).astype(np.float32)
    pv = rng.normal(size=n).astype(np.float32) if pred else None
    if entry == "gumbel":
        raw = np.concatenate([action[:n - 5], given])
        cq = (rng.random((n, A)) * 6).astype(np.float32)
        if A == 4:
            cq[0], cq[1] = [1e8, 1, -1e8, 1], [1, 1e8, 1, -1e8]
            assert cq_mean(cq[0]) == 0.25 and cq_mean(cq[1]) == 0.0
        gumbel = (raw, rng.dirichlet([0.5] * A, size=n).astype(np.float32), cq)
        visits = _one_hot(action, A, other=True)
    else:
        visits = _one_hot(action, A)
    want = k.host()
    dones = restate_cartpole_step(want, action, visits, value, KEY + 2, REC_T, E, REC_MAX, pred=pv, ret=ret,
                                  gumbel=gumbel)
    assert dones.sum() == 6 and not dones[:8].any()
    k.launch(visits, value, KEY + 2, REC_MAX, pred=pv, ret=ret, gumbel=gumbel)
    got = k.host()
    _assert_same(got, want, f"cartpole {entry} A={A} E={E}")
    assert got["ep_len"][11, 1 % E] == 5 and (got["rec_obs"][11, 1 % E] == np.float32(CANARY["rec_obs"])).all()
    assert got["ep_len"][9, 0] == 4 and (got["rec_obs"][9, 0, REC_T] != np.float32(CANARY["rec_obs"])).all()
    if ret:
        assert got["ep_return"][11, 1 % E] == 5.0 and got["ep_return"][8, 1 % E] == 9.0  # nt as a float
    if entry == "gumbel":
        assert got["rec_action"][n - 5:, 0, 1].tolist() == np.clip(given, 0, A - 1).tolist()
    assert (k.noises.cpu().numpy() >= 0).all()


def test_collect_steps_refuse_bad_arguments_and_launch_nothing():
    from lightzero_amd._lib import LZM_ERR_ARG, load, ptr, stream_ptr
    L = load()
    n, T, E = 3, 2, 1
    rng = np.random.default_rng(23)
    for game in ("breakout", "pong", "cartpole"):
        k = _Cart(n, 2, T, E) if game == "cartpole" else _Edge(game, n, T, E)
        A = k.A
        if game != "cartpole":
            k.put([ec.words(game, (ec._idle(30) if game == "breakout" else ec._pg()))] * n, [0] * n, [0] * n, rng)
        v, val, pv = _dev(_one_hot(np.zeros(n, np.int32), A)), _dev(np.zeros(n, np.float32)), _dev(np.ones(n, np.float32))
        act, pol = _dev(np.zeros(n, np.int32)), _dev(np.ones((n, A), np.float32))
        before = k.host()
        noises = k.noises.cpu().numpy()
        fn = getattr(L, {"breakout": "lzm_atari", "pong": "lzm_pong", "cartpole": "lzm_cartpole"}[game] + "_collect_step")

        def plain(A=A, pred=None, rec_pred=None, temperature=1.0, cur=None):
            env = [ptr(k.state), ptr(k.steps)] + ([] if game == "cartpole" else [cur or ptr(k.cur)]) + \
                  [ptr(k.obs), ptr(k.noises), 0.3, temperature, 1]
            rec0 = ptr(k.rec_obs) if game == "cartpole" else ptr(k.rec_frames)
            return fn(n, A, T, E, ptr(v), ptr(val), pred, *env, rec0, ptr(k.rec_action), ptr(k.rec_reward),
                      ptr(k.rec_visits), ptr(k.rec_value), rec_pred, ptr(k.ep_len), ptr(k.ep_count), ptr(k.ep_return), 9,
                      SEED, ptr(k.counter), stream_ptr())

        assert plain(pred=ptr(pv)) == LZM_ERR_ARG            # pred_value without rec_pred
        assert plain(rec_pred=ptr(k.rec_pred)) == LZM_ERR_ARG  # and the other way round
        assert plain(A=65) == LZM_ERR_ARG
        assert plain(temperature=0.0) == LZM_ERR_ARG
        if game != "cartpole":
            assert plain(cur=ptr(k.cur.view(-1)[4:])) == LZM_ERR_ARG  # a misaligned newest-frame buffer
        if game != "pong":
            gfn = getattr(L, ("lzm_cartpole" if game == "cartpole" else "lzm_atari") + "_collect_step_gumbel")
            env = [ptr(k.state), ptr(k.steps)] + ([] if game == "cartpole" else [ptr(k.cur)]) + \
                  [ptr(k.obs), ptr(k.noises), 0.3]
            rec0 = ptr(k.rec_obs) if game == "cartpole" else ptr(k.rec_frames)
            assert gfn(n, A, T, E, ptr(v), ptr(val), None, ptr(act), ptr(pol), ptr(pol), *env, rec0, ptr(k.rec_action),
                       ptr(k.rec_reward), ptr(k.rec_visits), ptr(k.rec_value), None, ptr(k.rec_policy), None,
                       ptr(k.ep_len), ptr(k.ep_count), ptr(k.ep_return), 9, SEED, ptr(k.counter),
                       stream_ptr()) == LZM_ERR_ARG       # rec_cq null
        torch.cuda.synchronize()
        _assert_same(k.host(), before, f"{game}: a refused call")
        assert np.array_equal(k.noises.cpu().numpy(), noises)
