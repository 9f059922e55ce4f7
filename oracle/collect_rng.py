"""Host restatement (numpy, float64) of the device collect step's random layer.

Written from lightzero_amd/csrc/lzm_collect.h and lzm_atari.h, vectorised over envs: the Philox streams
keyed by (seed, env, step, purpose), the 53-bit uniform `u01`, select_action's draw from the root visit
counts, the next root's Dirichlet noise (Marsaglia & Tsang's Gamma sampler, with the U^(1/alpha) boost for
alpha < 1), the CartPole / Breakout / Pong reset draws and the serve bits. Every env is a lane with its own
block counter; only the lanes that draw advance it, as the device's per-thread streams do.

tests/test_collect_rng.py checks these samplers against the Dirichlet, categorical and uniform laws on the
CPU; tests/test_gpu_collect_rng.py checks the kernels against them draw for draw.

The purposes (the high half of the fourth counter word): 1 CartPole reset entry point, 2 select_action,
3 the in-loop auto-reset (every env), 4 Dirichlet noise, 5 the Atari reset entry points, 6 the Atari games'
serve. The reset entry points run outside the step loop and use the step words 0xffffffff, 0xffffffff
(RESET_STEP).
"""
import numpy as np

KEY1 = 0x434f4c4c          # the collect streams' second key word ("COLL")
RESET_STEP = 2 ** 64 - 1   # the reset entry points' step words: 0xffffffff, 0xffffffff
MAX_ITERS = 64             # gamma_sample's iteration cap
PADDLE_SPAN = 53           # 64 - 2 walls of 2 - a paddle of 8 + 1 (Breakout's columns, Pong's rows)
_M32 = np.uint64(0xffffffff)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) over lanes: ctr [..., 4], key [..., 2] -> [..., 4] (uint64 arrays
    holding 32-bit words)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., k] & _M32 for k in range(4))
    k0, k1 = key[..., 0] & _M32, key[..., 1] & _M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1)


# the Random123 known answers (tests/test_oracle.py holds the same three for the C restatement)
assert philox4x32_10([0, 0, 0, 0], [0, 0]).tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
assert philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2).tolist() == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
assert philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]).tolist() == [
    0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def u01(a, b):
    """uniform in (0, 1) from two Philox words: 53 bits (27 of a, 26 of b), plus a half, over 2^53"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    m = ((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))
    return (m.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


class PhiloxStream:
    """One stream per env: counter (env, step & 0xffffffff, step >> 32, purpose << 16 | ctr & 0xffff), key
    (seed, KEY1). `ctr` counts each env's blocks; next(mask) draws a block for the masked lanes only."""

    def __init__(self, seed, env, step, purpose):
        self.env = np.atleast_1d(np.asarray(env, dtype=np.uint64)) & _M32
        self.n = len(self.env)
        step = int(step) & (2 ** 64 - 1)
        self.step_lo, self.step_hi = step & 0xffffffff, step >> 32
        self.purpose = int(purpose)
        self.key = np.array([int(seed) & 0xffffffff, KEY1], dtype=np.uint64)
        self.ctr = np.zeros(self.n, dtype=np.int64)

    def next(self, mask=None):
        """[n][4] words; the rows outside `mask` are zero and their counters stay"""
        idx = np.arange(self.n) if mask is None else np.flatnonzero(mask)
        c = np.empty((len(idx), 4), dtype=np.uint64)
        c[:, 0] = self.env[idx]
        c[:, 1], c[:, 2] = self.step_lo, self.step_hi
        c[:, 3] = np.uint64(self.purpose << 16) | (self.ctr[idx].astype(np.uint64) & np.uint64(0xffff))
        out = np.zeros((self.n, 4), dtype=np.uint64)
        out[idx] = philox4x32_10(c, self.key)
        self.ctr[idx] += 1
        return out


def gamma_sample(alpha, rs, boost="exact", d_plus_one=True):
    """Gamma(alpha) per lane of the stream `rs`, as lzm_collect.h's gamma_sample. alpha: the float32 the
    kernel receives (widened here). Returns (g, margin, exhausted, iters): margin is each lane's smallest
    |v0| and |log u - rhs| over its iterations (how far a decision was from flipping), exhausted the lanes
    that ran out of the 64 iterations, iters the iterations each lane ran.

    boost / d_plus_one exist for the tests' power check only (deliberately wrong samplers): boost "none"
    skips the alpha < 1 boost, "alpha" raises U to alpha instead of 1 / alpha; d_plus_one=False takes
    d = alpha - 1/3 for alpha < 1."""
    alpha = float(np.float32(alpha))
    n = rs.n
    boost_a = alpha + 1.0 if (alpha < 1.0 and d_plus_one) else alpha
    d = boost_a - 1.0 / 3.0
    with np.errstate(invalid="ignore", divide="ignore"):
        c = 1.0 / np.sqrt(9.0 * d)
        g = np.full(n, d)
        active = np.ones(n, dtype=bool)
        margin = np.full(n, np.inf)
        iters = np.zeros(n, dtype=np.int64)
        for _ in range(MAX_ITERS):
            idx = np.flatnonzero(active)
            if not len(idx):
                break
            iters[idx] += 1
            r = rs.next(active)[idx]
            u1, u2 = u01(r[:, 0], r[:, 1]), u01(r[:, 2], r[:, 3])
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)  # Box-Muller
            v0 = 1.0 + c * z
            margin[idx] = np.fmin(margin[idx], np.abs(v0))
            pos = ~(v0 <= 0.0)  # `if (v0 <= 0.0) continue;`
            pidx = idx[pos]
            pmask = np.zeros(n, dtype=bool)
            pmask[pidx] = True
            r2 = rs.next(pmask)[pidx]  # a rejected v0 consumed one block, not two
            z, v0 = z[pos], v0[pos]
            v = v0 * v0 * v0
            lu = np.log(u01(r2[:, 0], r2[:, 1]))
            rhs = 0.5 * z * z + d - d * v + d * np.log(v)
            margin[pidx] = np.fmin(margin[pidx], np.abs(lu - rhs))
            acc = lu < rhs
            g[pidx[acc]] = d * v[acc]
            active[pidx[acc]] = False
        if alpha < 1.0 and boost != "none":
            r = rs.next()
            g = g * np.power(u01(r[:, 0], r[:, 1]), alpha if boost == "alpha" else 1.0 / alpha)
    return g, margin, active, iters


def dirichlet_noise(seed, n, step, A, alpha, full=False, **wrong):
    """The next root's Dirichlet(alpha) noise the collect kernels write at step key `step`: [n][A] float32
    (purpose 4, the actions' Gammas in order on one stream, g / sum). full=True returns a dict with the
    margins, the exhausted flags, the largest iteration count and the streams' final counters as well."""
    rs = PhiloxStream(seed, np.arange(n), step, 4)
    g = np.empty((n, A))
    gs = np.zeros(n)
    margin = np.full(n, np.inf)
    exhausted = np.zeros(n, dtype=bool)
    max_iters = 0
    for a in range(A):
        g[:, a], m, ex, it = gamma_sample(alpha, rs, **wrong)
        gs = gs + g[:, a]
        margin = np.fmin(margin, m)
        exhausted |= ex
        max_iters = max(max_iters, int(it.max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        noise = np.where((gs > 0.0)[:, None], g / gs[:, None], 1.0 / A).astype(np.float32)
    if full:
        return dict(noise=noise, margin=margin, exhausted=exhausted, max_iters=max_iters, ctr=rs.ctr.copy())
    return noise


def select_action(visits, temperature, deterministic, seed, step, env=None):
    """The action the collect kernels choose from the root visit counts [n][A] at step key `step` (purpose
    2). Returns (action [n] int32, margin [n]): margin = min_a |u tot - cum_a| / tot, how far the draw was
    from the nearest boundary of the running sum (inf in deterministic mode, which draws nothing). env: the
    rows' env indices (default 0 .. n-1)."""
    v = np.asarray(visits, dtype=np.int64)
    n, A = v.shape
    if deterministic:
        return np.argmax(v, axis=1).astype(np.int32), np.full(n, np.inf)  # the first maximum
    inv_t = 1.0 / float(np.float32(temperature))
    w = np.power(np.maximum(v, 0).astype(np.float64), inv_t)
    cum = np.cumsum(w, axis=1)  # sequential, in action order, as the kernel's running sum
    tot = cum[:, -1]
    rs = PhiloxStream(seed, np.arange(n) if env is None else env, step, 2)
    r = rs.next()
    u = u01(r[:, 0], r[:, 1]) * tot
    hit = (w > 0.0) & (u[:, None] < cum)
    action = np.where(hit.any(axis=1), np.argmax(hit, axis=1), A - 1).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.abs(u[:, None] - cum).min(axis=1) / tot
    return action, margin


def cartpole_reset(seed, n, step=None):
    """CartPole's reset state [n][4] float64, U(-0.05, 0.05)^4 from two blocks: lzm_cartpole_reset
    (step=None: purpose 1 at RESET_STEP) or the collect step's auto-reset at step key `step` (purpose 3)."""
    rs = PhiloxStream(seed, np.arange(n), RESET_STEP if step is None else step, 1 if step is None else 3)
    a, b = rs.next(), rs.next()
    u = np.stack([u01(a[:, 0], a[:, 1]), u01(a[:, 2], a[:, 3]), u01(b[:, 0], b[:, 1]), u01(b[:, 2], b[:, 3])], axis=1)
    return -0.05 + 0.1 * u


def _atari_reset_block(seed, n, step):
    rs = PhiloxStream(seed, np.arange(n), RESET_STEP if step is None else step, 5 if step is None else 3)
    return rs.next()


def breakout_reset(seed, n, step=None):
    """Breakout's reset state [n][16] int32 (at_reset): the paddle column 2 + r.x % 53, a full wall of
    bricks, one life. step=None: lzm_atari_reset (purpose 5); else the auto-reset at that step key."""
    r = _atari_reset_block(seed, n, step)
    s = np.zeros((n, 16), dtype=np.int32)
    s[:, 0] = 2 + (r[:, 0] % np.uint64(PADDLE_SPAN)).astype(np.int32)
    s[:, 6], s[:, 7], s[:, 8], s[:, 9] = -1, -1, (1 << 26) - 1, 1  # bricks 0..31, 32..63, 64..89; lives
    return s


def pong_reset(seed, n, step=None):
    """Pong's reset state [n][16] int32 (pg_reset): the agent's paddle 2 + r.x % 53, the opponent's
    2 + r.y % 53 (word 6). step as breakout_reset (lzm_pong_reset is the entry point)."""
    r = _atari_reset_block(seed, n, step)
    s = np.zeros((n, 16), dtype=np.int32)
    s[:, 0] = 2 + (r[:, 0] % np.uint64(PADDLE_SPAN)).astype(np.int32)
    s[:, 6] = 2 + (r[:, 1] % np.uint64(PADDLE_SPAN)).astype(np.int32)
    return s


def serve_bits(seed, n, step):
    """The serve's two bits at step key `step` (the first block of purpose 6): (r.x & 1, r.x & 2) as bools.
    Breakout's ball leaves with vx = +1 where the first is set, else -1; Pong's with vx from the first and
    vy from the second."""
    r = PhiloxStream(seed, np.arange(n), step, 6).next()
    return (r[:, 0] & np.uint64(1)) != 0, (r[:, 0] & np.uint64(2)) != 0


def first_block(seed, env, step, purpose):
    """the first block [4] of one env's stream (the stream-separation checks)"""
    return PhiloxStream(seed, [env], step, purpose).next()[0]
