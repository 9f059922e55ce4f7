"""CPU: the host restatement of the collect kernels' random layer (oracle/collect_rng.py) samples the
right laws.

tests/test_gpu_collect_rng.py pins the device kernels to this restatement draw for draw; here the
restatement itself is checked, on fixed seeds: the Dirichlet noise against its Beta marginals and its
variance (with a power check: the same KS test rejects three deliberately wrong Gamma samplers, which a
check of the mean would pass), select_action against v^(1/T) / sum, the reset draws against their uniform
laws, the streams' separation, and the iteration, counter and decision-margin caps that let the GPU test
demand every row.

Observed at the committed seeds (the conditions are p >= 1e-4 and margins >= 1e-9):
- Dirichlet KS: smallest p 0.0345 over 93 tests; mean column variances within 1.2 % of theory;
  at most 5 iterations per Gamma, block counter at most 214 (A = 64, where 3 blocks per action make it
  at least 192);
- smallest Gamma decision margin 1.8e-8 (the statistical inputs and the GPU test's inputs: the same row);
- select_action chi-square: smallest p 0.169 over 15 tests; smallest selection margin 9.7e-7;
- resets: CartPole KS p >= 0.047 over 15 tests, paddle chi-square p >= 0.055 over 6, serve bits p 0.81.
"""
import numpy as np
import pytest
from scipy import stats

from oracle import collect_rng as cr

SEED = 5
N_STAT = 20000
STEP_KEYS = (1, 2, 2 ** 32 + 5)
DIRICHLET_CASES = [(2, 0.3), (4, 0.3), (6, 0.3), (18, 0.3), (64, 0.3), (4, 1.0), (3, 2.5)]
TEMPERATURES = (1.0, 0.5, 0.25)
P_MIN = 1e-4
MARGIN_MIN = 1e-9

# ---- what tests/test_gpu_collect_rng.py launches (its raw calls): the margin caps below cover these inputs
GPU_SEED = 5
GPU_COUNTERS = (0, 1, 2 ** 32 + 5)
GPU_CARTPOLE_N = 4096
GPU_CARTPOLE_A = (2, 3, 6, 18, 64)
GPU_CARTPOLE_ALPHAS = {3: (0.3, 1.0, 2.5)}  # (the other A: 0.3, the collector's default)
GPU_ATARI = {"breakout": 4, "pong": 6}
GPU_ATARI_N = 256
VISIT_SUM = 50


def visit_rows(A, n, seed=0):
    """[n][A] int32 root visit counts: random compositions of 50 over a random support (so with zeros), and
    in every group of 16 rows one count alone in the first, the last and a middle slot, a zero in the first
    slot, in the last, and in both."""
    rng = np.random.default_rng(1000 * A + seed)
    v = np.zeros((n, A), dtype=np.int32)
    for i in range(n):
        k = i % 16
        if k == 0:
            support = [0]
        elif k == 1:
            support = [A - 1]
        elif k == 2:
            support = [A // 2]
        else:
            size = int(rng.integers(1, A + 1))
            support = rng.choice(A, size=size, replace=False)
            if k in (3, 5):
                support = support[support != 0]
            if k in (4, 5):
                support = support[support != A - 1]
            if len(support) == 0:  # (A = 2 has no slot left for k = 5: the first then)
                banned = ([0] if k in (3, 5) else []) + ([A - 1] if k in (4, 5) else [])
                support = [a for a in range(A) if a not in banned][:1] or [0]
        v[i, support] = rng.multinomial(VISIT_SUM, rng.dirichlet(np.ones(len(support))))
    return v


def tie_rows(A, n, seed=0):
    """[n][A] small counts with many ties for the maximum (deterministic mode takes the first)"""
    return np.random.default_rng(2000 * A + seed).integers(0, 4, size=(n, A)).astype(np.int32)


def _columns(A):
    return list(range(A)) if A <= 6 else [0, 1, 2, A // 2, A - 2, A - 1]


def _ks_min_p(noise, A, alpha):
    law = stats.beta(alpha, (A - 1) * alpha)
    return min(stats.kstest(noise[:, c].astype(np.float64), law.cdf).pvalue for c in _columns(A))


@pytest.fixture(scope="module")
def dirichlet_runs():
    """(A, alpha, key) -> dirichlet_noise(..., full=True) at the statistical inputs, computed once"""
    return {(A, alpha, key): cr.dirichlet_noise(SEED, N_STAT, key, A, alpha, full=True)
            for A, alpha in DIRICHLET_CASES for key in STEP_KEYS}


def test_dirichlet_marginals_and_variance(dirichlet_runs):
    """Every checked column (all of them for A <= 6, six for A = 18 and 64) passes a KS test against
    Beta(alpha, (A - 1) alpha): 93 tests, none below p = 1e-4 (observed minimum: see the module docstring).

    The mean column variance against (A - 1) / (A^2 (A alpha + 1)): a column's sample variance over N rows
    has relative standard error sqrt((kurtosis - 1) / N) (kurtosis of the Beta marginal, from scipy); the mean
    over columns cannot have a larger one (Cauchy-Schwarz), so the bound is 5 of those."""
    ps, devs = [], []
    for (A, alpha, key), run in dirichlet_runs.items():
        noise = run["noise"]
        assert noise.dtype == np.float32 and noise.shape == (N_STAT, A)
        assert (noise >= 0).all() and np.abs(noise.astype(np.float64).sum(1) - 1.0).max() < 1e-6
        p = _ks_min_p(noise, A, alpha)
        ps.append(p)
        assert p >= P_MIN, (A, alpha, key, p)
        var = noise.astype(np.float64).var(axis=0).mean()
        theory = (A - 1) / (A * A * (A * alpha + 1))
        kurt = float(stats.beta(alpha, (A - 1) * alpha).stats(moments="k")) + 3.0
        bound = 5.0 * np.sqrt((kurt - 1.0) / N_STAT)
        devs.append(abs(var / theory - 1.0))
        assert devs[-1] < bound, (A, alpha, key, var, theory, bound)
    print(f"dirichlet: min KS p {min(ps):.4g} over {sum(len(_columns(A)) for A, _, _ in dirichlet_runs)} tests, "
          f"max variance deviation {max(devs):.3%}")


def test_ks_rejects_wrong_gamma_samplers():
    """The power check: on the same streams the same KS test rejects, at p < 1e-6, a sampler without the
    alpha < 1 boost, one whose boost exponent is alpha in place of 1 / alpha, and one with d = alpha - 1/3
    (no + 1; at alpha = 0.3 that d is negative and every row falls to 1 / A, at alpha = 0.6 it is a proper but
    wrong sampler). All three keep the mean 1 / A, which is all the older device check looked at."""
    for A, alpha, wrong in [(4, 0.3, dict(boost="none")), (4, 0.3, dict(boost="alpha")),
                            (4, 0.3, dict(d_plus_one=False)), (4, 0.6, dict(d_plus_one=False)),
                            (2, 0.3, dict(boost="none")), (6, 0.3, dict(boost="alpha"))]:
        noise = cr.dirichlet_noise(SEED, N_STAT, 1, A, alpha, **wrong)
        law = stats.beta(alpha, (A - 1) * alpha)
        p = max(stats.kstest(noise[:, c].astype(np.float64), law.cdf).pvalue for c in range(A))
        assert p < 1e-6, (A, alpha, wrong, p)
        assert abs(noise.astype(np.float64).mean() - 1.0 / A) < 1e-6  # the mean cannot tell
    # and Dirichlet(1) in place of Dirichlet(0.3)
    noise = cr.dirichlet_noise(SEED, N_STAT, 1, 4, 1.0)
    assert stats.kstest(noise[:, 0].astype(np.float64), stats.beta(0.3, 0.9).cdf).pvalue < 1e-6
    # the exact sampler at alpha = 0.6 passes (the d = alpha - 1/3 rejection above is not the law's doing)
    assert _ks_min_p(cr.dirichlet_noise(SEED, N_STAT, 1, 4, 0.6), 4, 0.6) >= P_MIN


def test_gamma_iteration_and_counter_caps(dirichlet_runs):
    """no row runs out of the 64 iterations, no stream's block counter passes 0xffff (it would wrap into
    the purpose's bits)"""
    for key, run in dirichlet_runs.items():
        assert not run["exhausted"].any(), key
        assert run["ctr"].max() <= 0xffff, key
    print("max iterations", max(r["max_iters"] for r in dirichlet_runs.values()),
          "max ctr", max(int(r["ctr"].max()) for r in dirichlet_runs.values()))


def _gpu_noise_inputs():
    for A in GPU_CARTPOLE_A:
        for alpha in GPU_CARTPOLE_ALPHAS.get(A, (0.3,)):
            for key in GPU_COUNTERS:
                yield GPU_CARTPOLE_N, A, alpha, key
    for A in GPU_ATARI.values():
        for key in GPU_COUNTERS:
            yield GPU_ATARI_N, A, 0.3, key


def test_gamma_decision_margins(dirichlet_runs):
    """A condition on the committed inputs, not a measurement: no row's Gamma decision (v0 > 0, log u < rhs)
    is closer than 1e-9 to flipping, at the statistical inputs and at every input of the GPU test's raw
    calls, so a few double ulps between the device's and numpy's log / cos cannot change a branch and the GPU
    test may demand every row. If an input ever violates this, change its seed."""
    stat = min(float(r["margin"].min()) for r in dirichlet_runs.values())
    assert stat >= MARGIN_MIN, stat
    gpu = np.inf
    for n, A, alpha, key in _gpu_noise_inputs():
        run = cr.dirichlet_noise(GPU_SEED, n, key, A, alpha, full=True)
        assert not run["exhausted"].any() and run["ctr"].max() <= 0xffff
        gpu = min(gpu, float(run["margin"].min()))
        assert gpu >= MARGIN_MIN, (n, A, alpha, key, gpu)
    print(f"gamma margins: statistical inputs {stat:.3g}, GPU inputs {gpu:.3g}")


# ---------------------------------------------------------------- select_action
FIXED_ROWS = [
    [15, 35],
    [0, 20, 12, 18],
    [9, 0, 14, 7, 20, 0],
    [0, 5, 3, 0, 4, 2, 6, 0, 3, 5, 2, 4, 0, 3, 6, 2, 5, 0],
    [3] * 10 + [0] * 20 + [2] * 6 + [0] * 20 + [1] * 8,
]


def test_select_action_follows_the_categorical_law():
    """chi-square of 20,000 restated draws (one fixed row over the env index) against v^(1/T) / sum, for
    five rows (A = 2, 4, 6, 18, 64, with zeros) and three temperatures: no p below 1e-4; the zero-count
    actions are never drawn"""
    ps = []
    for row in FIXED_ROWS:
        v = np.asarray(row, dtype=np.int32)
        assert v.sum() == VISIT_SUM
        for k, T in enumerate(TEMPERATURES):
            act, _ = cr.select_action(np.tile(v, (N_STAT, 1)), T, False, SEED, STEP_KEYS[k])
            w = v.astype(np.float64) ** (1.0 / T)
            expect = w / w.sum() * N_STAT
            got = np.bincount(act, minlength=len(v))
            assert (got[v == 0] == 0).all(), (row, T)
            assert expect[v > 0].min() >= 5.0  # the chi-square approximation's usual condition
            p = stats.chisquare(got[v > 0], expect[v > 0]).pvalue
            ps.append(p)
            assert p >= P_MIN, (row, T, p)
    print(f"select_action: min chi-square p {min(ps):.4g} over {len(ps)} tests")


def test_select_action_rows_and_margins():
    """the GPU test's visit rows: zero-count actions are never drawn, a lone count is always drawn, the
    smallest selection margin is >= 1e-9 (the condition that lets the GPU test demand every row), and
    deterministic mode is np.argmax (the first maximum) on rows with ties"""
    smallest = np.inf
    for n, As in [(GPU_CARTPOLE_N, GPU_CARTPOLE_A), (GPU_ATARI_N, tuple(GPU_ATARI.values()))]:
        for A in As:
            v = visit_rows(A, n)
            assert (v.sum(1) == VISIT_SUM).all() and (v == 0).any()
            assert (v[0::16, 1:] == 0).all() and (v[1::16, :-1] == 0).all()
            assert (v[3::16, 0] == 0).all() and (v[4::16, -1] == 0).all()
            for T in TEMPERATURES:
                for key in GPU_COUNTERS:
                    act, margin = cr.select_action(v, T, False, GPU_SEED, key)
                    assert (v[np.arange(n), act] > 0).all(), (A, T, key)
                    assert (act[0::16] == 0).all() and (act[1::16] == A - 1).all() and (act[2::16] == A // 2).all()
                    smallest = min(smallest, float(margin.min()))
                    assert smallest >= MARGIN_MIN, (A, T, key, smallest)
            t = tie_rows(A, n)
            first_max = np.array([next(a for a in range(A) if row[a] == row.max()) for row in t])
            assert (np.sort(t, axis=1)[:, -1] == np.sort(t, axis=1)[:, -2]).any()  # ties for the maximum
            act, _ = cr.select_action(t, 1.0, True, GPU_SEED, 1)
            assert (act == first_max).all() and (act == np.argmax(t, axis=1)).all()
    print(f"select_action: smallest margin {smallest:.3g}")


def test_select_action_fallback_and_temperature():
    # all-zero counts: nothing has weight, the draw falls to the last action
    act, _ = cr.select_action(np.zeros((8, 5), np.int32), 1.0, False, SEED, 1)
    assert (act == 4).all()
    # negative counts weigh nothing
    act, _ = cr.select_action(np.tile(np.array([-3, 7, -1], np.int32), (64, 1)), 0.5, False, SEED, 1)
    assert (act == 1).all()
    # the same uniforms at a lower temperature move towards the larger count, never away from it
    v = np.tile(np.array([15, 35], np.int32), (N_STAT, 1))
    a1, _ = cr.select_action(v, 1.0, False, SEED, 3)
    a4, _ = cr.select_action(v, 0.25, False, SEED, 3)
    assert (a4 >= a1).all() and (a4 > a1).any()


# ---------------------------------------------------------------- streams
def test_streams_are_separate():
    seed, env, step = SEED, 7, 11
    blocks = {p: tuple(cr.first_block(seed, env, step, p).tolist()) for p in (1, 2, 3, 4, 5, 6)}
    assert len(set(blocks.values())) == 6  # purposes 2, 3, 4 and 6 (and the reset entry points' 1 and 5)
    base = blocks[2]
    assert tuple(cr.first_block(seed, env, step + 2 ** 32, 2).tolist()) != base  # the counter's high word
    assert tuple(cr.first_block(seed, env, step + 1, 2).tolist()) != base
    assert tuple(cr.first_block(seed, env + 1, step, 2).tolist()) != base
    assert tuple(cr.first_block(seed + 1, env, step, 2).tolist()) != base
    # the words are what Philox gives for the documented counter and key
    want = cr.philox4x32_10([env, 11, 1, (4 << 16) | 0], [seed, 0x434f4c4c])
    assert cr.first_block(seed, env, 2 ** 32 + 11, 4).tolist() == want.tolist()
    # a stream's second block is counter word 3 plus one; only the masked lanes advance
    rs = cr.PhiloxStream(seed, np.arange(4), step, 4)
    rs.next(np.array([True, False, True, False]))
    b = rs.next()
    assert rs.ctr.tolist() == [2, 1, 2, 1]
    assert b[0].tolist() == cr.philox4x32_10([0, step, 0, (4 << 16) | 1], [seed, 0x434f4c4c]).tolist()
    assert b[1].tolist() == cr.philox4x32_10([1, step, 0, (4 << 16) | 0], [seed, 0x434f4c4c]).tolist()
    # the reset entry points' step words
    rs = cr.PhiloxStream(seed, [0], cr.RESET_STEP, 1)
    assert (rs.step_lo, rs.step_hi) == (0xffffffff, 0xffffffff)


def test_oracle_philox_agrees():
    """the numpy Philox and the C restatement's (oracle.oracle.philox4x32_10) give the same words"""
    from oracle.oracle import philox4x32_10
    rng = np.random.default_rng(0)
    for _ in range(16):
        c, k = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64), rng.integers(0, 2 ** 32, size=2, dtype=np.uint64)
        assert cr.philox4x32_10(c, k).tolist() == philox4x32_10(c.astype(np.uint32), k.astype(np.uint32)).tolist()


def test_u01():
    assert cr.u01(0, 0) == 0.5 * 2.0 ** -53
    assert cr.u01(0xffffffff, 0xffffffff) <= 1.0
    assert cr.u01(1 << 31, 0) == (2.0 ** 52 + 0.5) * 2.0 ** -53
    assert cr.u01(0x1f, 0x3f) == cr.u01(0, 0)  # the low 5 and 6 bits are dropped


# ---------------------------------------------------------------- resets and serves
def test_cartpole_resets_are_uniform():
    ps = []
    for step in (None, 1, 2 ** 32 + 5):
        s = cr.cartpole_reset(SEED, N_STAT, step)
        assert s.shape == (N_STAT, 4) and s.dtype == np.float64
        assert (s > -0.05).all() and (s < 0.05).all()
        for j in range(4):
            ps.append(stats.kstest(s[:, j], stats.uniform(-0.05, 0.1).cdf).pvalue)
        ps.append(stats.kstest(s.reshape(-1), stats.uniform(-0.05, 0.1).cdf).pvalue)
    assert min(ps) >= P_MIN, ps
    assert not np.array_equal(cr.cartpole_reset(SEED, 8), cr.cartpole_reset(SEED, 8, cr.RESET_STEP))  # purposes 1, 3
    print(f"cartpole resets: min KS p {min(ps):.3g}")


def test_paddle_draws_are_uniform():
    ps = []
    for step in (None, 2):
        b, p = cr.breakout_reset(SEED, N_STAT, step), cr.pong_reset(SEED, N_STAT, step)
        for col in (b[:, 0], p[:, 0], p[:, 6]):
            assert col.min() >= 2 and col.max() <= 54
            ps.append(stats.chisquare(np.bincount(col - 2, minlength=53)).pvalue)
        assert np.array_equal(b[:, 0], p[:, 0])  # the same word of the same block
        other = np.ones(16, bool)
        other[[0, 6, 7, 8, 9]] = False
        assert (b[:, 6] == -1).all() and (b[:, 7] == -1).all() and (b[:, 8] == (1 << 26) - 1).all()
        assert (b[:, 9] == 1).all() and (b[:, other] == 0).all()
        other[[7, 8, 9]] = True
        assert (p[:, other] == 0).all()
    assert min(ps) >= P_MIN, ps
    print(f"paddles: min chi-square p {min(ps):.3g}")


def test_serve_bits_are_fair():
    b0, b1 = cr.serve_bits(SEED, N_STAT, 3)
    p = stats.chisquare(np.bincount(b0 + 2 * b1.astype(np.int64), minlength=4)).pvalue
    assert p >= P_MIN, p
    print(f"serve bits: chi-square p {p:.3g}")
