"""Plain numpy-float32 restatement of LightZero's Stochastic MuZero tree (test infrastructure; the package never
imports it): lzero/mcts/ctree/ctree_stochastic_muzero/lib/cnode.cpp, line numbers of that file. Every quantity is
a float32 scalar and every sum runs in the C++ loops' order. The compiled reference module imports expf, logf and
sqrtf from libm (nm -D; no double exp / log / sqrt), so those are the host libm's float functions here.

The two random choices are callables: tie_draw(level, root) -> the rand() value of cselect_child (:659) and
chance_draw(level, root, priors) -> the outcome index of a chance node (:610-630). glibc_draws / onehot_chance
replay the compiled reference's transcripts (one-hot chance rows make its std::random_device draw deterministic);
philox_draws is the device's rule and makes this module the yardstick for the kernels.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("expf", "logf", "sqrtf"):
    getattr(_libm, _n).argtypes = [ctypes.c_float]
    getattr(_libm, _n).restype = ctypes.c_float
FLOAT_MAX, FLOAT_MIN = F(1000000.0), F(-1000000.0)
KEY = 0x4c5a4d43


def chance_pick(priors, u):
    """the first outcome whose running double sum of the float32 priors exceeds u * total; if rounding leaves
    none, the last outcome with a non-zero prior"""
    pre, run = [], 0.0
    for p in priors:
        run += float(p)
        pre.append(run)
    for j, s in enumerate(pre):
        if s > u * run:
            return j
    nz = [j for j, p in enumerate(priors) if p != 0]
    return nz[-1] if nz else 0


def chance_u(w0, w1):
    """the 53-bit uniform in (0, 1) of two Philox words (lzm_collect.h u01)"""
    return ((((int(w0) >> 5) << 26) | (int(w1) >> 6)) + 0.5) * 2.0 ** -53


def philox_draws(seed):
    """(tie_draw, chance_draw) of one traverse under the device's rule (include/lzmcts.h)"""
    from oracle.oracle import philox4x32_10
    key = [int(seed) & 0xFFFFFFFF, KEY]

    def chance(level, root, priors):
        o = philox4x32_10([level, root, 1, 0], key)
        return chance_pick(priors, chance_u(o[0], o[1]))
    return (lambda level, root: int(philox4x32_10([level, root, 0, 0], key)[0]) >> 1), chance


def glibc_draws(seed, n=1 << 14):
    """tie_draw of one reference traverse: srand(seed), then rand() in batch order, one per decision level"""
    from oracle.oracle import glibc_rand_stream
    it = iter(glibc_rand_stream(int(seed), n))
    return lambda level, root: int(next(it))


def onehot_chance(level, root, priors):
    hot = [j for j, p in enumerate(priors) if p == 1]
    assert len(hot) == 1 and sum(1 for p in priors if p != 0) == 1, "the reference's draw is not deterministic here"
    return hot[0]


class MinMax:  # CMinMaxStats (common_lib/cminimax.cpp)
    def __init__(self, delta):
        self.mx, self.mn, self.delta = FLOAT_MIN, FLOAT_MAX, F(delta)

    def update(self, v):
        self.mx, self.mn = max(self.mx, v), min(self.mn, v)

    def normalize(self, v):
        d = F(self.mx - self.mn)
        if d > 0:
            return F(F(v - self.mn) / (self.delta if d < self.delta else d))
        return v


class Node:
    def __init__(self, prior, legal, is_chance):
        self.prior, self.legal, self.is_chance = F(prior), list(legal), is_chance
        self.visit, self.value_sum, self.reward = 0, F(0), F(0)
        self.best, self.to_play, self.latent, self.children = -1, 0, -1, {}

    def value(self):  # :245-261
        return F(0) if self.visit == 0 else F(self.value_sum / F(self.visit))

    def expand(self, to_play, latent, reward, logits):  # :96-173
        self.to_play, self.latent = to_play, latent
        self.reward = F(0) if self.is_chance else F(reward)
        if not self.legal:
            self.legal = list(range(len(logits)))
        pmax = FLOAT_MIN
        for a in self.legal:
            if pmax < logits[a]:
                pmax = F(logits[a])
        e, s = {}, F(0)
        for a in self.legal:
            e[a] = F(_libm.expf(F(F(logits[a]) - pmax)))
            s = F(s + e[a])
        for a in self.legal:
            self.children[a] = Node(F(e[a] / s), [], not self.is_chance)


class Tree:
    """CRoots + CSearchResults of one batch"""

    def __init__(self, legal_lists, ties=None):
        self.roots = [Node(0, l, False) for l in legal_lists]
        self.B = len(self.roots)
        self.ties = ties if ties is not None else []  # sizes of the tie lists longer than one

    def prepare(self, noise_weight, noises, rewards, logits, to_play):  # :349-386
        f = F(noise_weight)
        for i, r in enumerate(self.roots):
            r.expand(int(to_play[i]), 0, rewards[i], logits[i])
            if noises is not None:
                for j, a in enumerate(r.legal):
                    c = r.children[a]
                    c.prior = F(F(c.prior * F(F(1) - f)) + F(F(noises[i][j]) * f))
            r.visit += 1

    def _select(self, node, mm, base, init, disc, mean_q, players, level, root, tie_draw, chance_draw):
        if node.is_chance:  # :610-630, the children in outcome order
            keys = sorted(node.children)
            return keys[chance_draw(level, root, [node.children[k].prior for k in keys])]
        N = F(node.visit - 1)
        pbc0 = F(F(_libm.logf(F(F(F(N + F(base)) + F(1)) / F(base)))) + F(init))
        sq = F(_libm.sqrtf(N))
        best, lst = FLOAT_MIN, []
        for a in node.legal:
            c = node.children[a]
            pb_c = F(pbc0 * F(sq / F(c.visit + 1)))
            if c.visit == 0:
                vs = mean_q
            else:
                cv = c.value() if players == 1 else F(-c.value())
                vs = F(c.reward + F(disc * cv))
            vs = min(max(mm.normalize(vs), F(0)), F(1))
            score = F(F(pb_c * c.prior) + vs)
            if best < score:
                best, lst = score, [a]
            elif score >= F(best - F(0.000001)):
                lst.append(a)
        if len(lst) > 1:
            self.ties.append(len(lst))
        return lst[tie_draw(level, root) % len(lst)] if lst else 0

    def traverse(self, base, init, disc, mms, vtp_in, tie_draw, chance_draw):  # :711-786
        disc, vtp = F(disc), [int(v) for v in vtp_in]
        players = 1 if max(vtp) == -1 else 2
        self.paths, out = [], {k: [] for k in ("is_chance", "x", "y", "a", "vtp", "len")}
        for i, node in enumerate(self.roots):
            path, parent_q, action, level = [node], F(0), -1, 0
            while node.children:
                tq, tv = F(0), 0  # compute_mean_q :195-229
                for a in node.legal:
                    c = node.children[a]
                    if c.visit > 0:
                        tq, tv = F(tq + F(c.reward + F(disc * c.value()))), tv + 1
                mean_q = F(tq / F(tv)) if level == 0 and tv > 0 else F(F(parent_q + tq) / F(tv + 1))
                parent_q = mean_q
                action = self._select(node, mms[i], base, init, disc, mean_q, players, level, i, tie_draw, chance_draw)
                if players > 1:
                    vtp[i] = 2 if vtp[i] == 1 else 1
                node.best = action
                node = node.children[action]
                path.append(node)
                level += 1
            self.paths.append(path)
            for k, v in zip(("is_chance", "x", "y", "a", "vtp", "len"),
                            (int(node.is_chance), path[-2].latent, i, action, vtp[i], level)):
                out[k].append(v)
        self.leaf_is_chance = out["is_chance"]
        return out

    def backprop(self, cur, disc, rewards, values, logits, mms, to_play, leaf_idx=None):  # :496-592
        disc = F(disc)
        for k, i in enumerate(range(self.B) if leaf_idx is None else leaf_idx):
            path, tp, b = self.paths[i], int(to_play[i]), F(values[k])
            path[-1].expand(tp, cur, rewards[k], logits[k])
            for node in reversed(path):
                same = tp == -1 or node.to_play == tp
                node.value_sum = F(node.value_sum + (b if same else F(-b)))
                node.visit += 1
                v = node.value() if tp == -1 else F(-node.value())
                mms[i].update(F(node.reward + F(disc * v)))
                r = node.reward if tp == -1 or node.to_play != tp else F(-node.reward)
                b = F(r + F(disc * b))

    def distributions(self):
        return [[r.children[a].visit for a in r.legal] if r.children else [] for r in self.roots]

    def values(self):
        return np.array([r.value() for r in self.roots], F)

    def trajectories(self):  # :263-283
        out = []
        for n in self.roots:
            t = []
            while n.best >= 0:
                t.append(n.best)
                n = n.children[n.best]
            out.append(t)
        return out


def pad(rows, width, fill=-1):
    out = np.full((len(rows), max(width, 1)), fill, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def legal_lists(g):
    return [[int(a) for a in row if a >= 0] for row in g["legal_lists"]]


def replay(g, draws):
    """Runs transcript g's search (its scripted network: both head sets for every (simulation, root)) with
    draws(k) -> (tie_draw, chance_draw) of simulation k. Returns the arrays a transcript records, and `ties`."""
    B, S, A, C, noise = [int(v) for v in g["meta"][:5]]
    base, init, disc, vdm, nw = [float(v) for v in g["consts"]]
    t = Tree(legal_lists(g))
    mms = [MinMax(vdm) for _ in range(B)]
    t.prepare(nw, g["noises"] if noise else None, g["root_reward"], g["root_logits"], g["to_play"])
    req = {k: np.zeros((S, B), np.int32) for k in ("is_chance", "x", "y", "a", "vtp", "len")}
    for k in range(S):
        out = t.traverse(int(base), init, disc, mms, g["to_play"], *draws(k))
        for name in req:
            req[name][k] = out[name]
        ch = np.array(out["is_chance"], bool)
        r = np.where(ch, 0, g["resp_d_reward"][k])
        v = np.where(ch, g["resp_c_value"][k], g["resp_d_value"][k])
        rows = [g["resp_c_logits"][k, i] if ch[i] else g["resp_d_logits"][k, i] for i in range(B)]
        t.backprop(k + 1, disc, r, v, rows, mms, out["vtp"])
    res = {"req_" + k: v for k, v in req.items()}
    res.update(out_dist=pad(t.distributions(), A), out_values=t.values(),
               out_traj=pad(t.trajectories(), S + 1), ties=len(t.ties))
    return res
