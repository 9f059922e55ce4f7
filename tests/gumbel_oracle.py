"""Plain float32 host restatement of LightZero's Gumbel MuZero tree, for the tests only.

Restates lzero/mcts/ctree/ctree_gumbel_muzero/lib/cnode.cpp (line numbers of that file below) in numpy
float32 scalars, every sum sequential in legal order as the C++ loops run. expf / logf are the host libm's
through ctypes; the Gumbel table (generate_gumbel :1134-1152 with std::mt19937(0)) is read from the
fixture tests/golden/gumbel/gmz_tables.npz, so nothing here needs libstdc++. The package never imports this file.
"""
import ctypes
import ctypes.util
import os

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.argtypes = [ctypes.c_float]
_libm.expf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.logf.restype = ctypes.c_float
NEG_INF = F(-np.inf)
FLOAT_MIN = F(-1000000.0)  # common_lib/cminimax.h:9-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gumbel")


def expf(x):
    return F(_libm.expf(float(x)))


def logf(x):
    return F(_libm.logf(float(x)))


def gumbel_table():
    return np.load(os.path.join(GOLDEN, "gmz_tables.npz"))["gumbel"].astype(np.float32)


def considered_visits(m, S):
    """get_sequence_of_considered_visits (:1042-1077) for the row cselect_root_child reads (:727-729)."""
    m = min(m, S)
    if m <= 1:
        return list(range(S))
    log2max = int(np.ceil(np.log2(m)))
    seq, visits, n = [], [0] * m, m
    while len(seq) < S:
        extra = max(1, int(S // (log2max * n)))
        for _ in range(extra):
            seq.extend(visits[:n])
            for j in range(n):
                visits[j] += 1
        n = max(2, n // 2)
    return seq[:S]


def csoftmax(x):
    """csoftmax (:904-933)."""
    m = x[0]
    for v in x[1:]:
        if v > m:
            m = v
    s = F(0)
    for v in x:
        s = F(s + expf(F(v - m)))
    ls = logf(s)
    return [expf(F(F(v - m) - ls)) for v in x]


class Node:
    __slots__ = ("prior", "legal", "visit", "value_sum", "raw_value", "best", "to_play", "reward", "latent",
                 "children")

    def __init__(self, prior, legal):
        self.prior, self.legal = F(prior), list(legal)
        self.visit, self.value_sum, self.raw_value = 0, F(0), F(0)
        self.best, self.to_play, self.reward, self.latent = -1, 0, F(0), -1
        self.children = {}

    def value(self):  # CNode::value (:245-261)
        return F(0) if self.visit == 0 else F(self.value_sum / F(self.visit))

    def expand(self, to_play, latent, reward, value, logits):  # CNode::expand (:94-156)
        self.to_play, self.latent, self.reward, self.raw_value = to_play, latent, F(reward), F(value)
        if not self.legal:
            self.legal = list(range(len(logits)))
        pmax = FLOAT_MIN
        for a in self.legal:
            if pmax < logits[a]:
                pmax = F(logits[a])
        e, s = {}, F(0)
        for a in self.legal:
            e[a] = expf(F(F(logits[a]) - pmax))
            s = F(s + e[a])
        for a in self.legal:
            self.children[a] = Node(F(e[a] / s), [])


def completed_q(node, disc):
    """qtransform_completed_by_mix_value (:989-1040; defaults cnode.h:100-102: maxvisit_init 50, value_scale 0.1,
    rescale, epsilon 1e-8) with get_q (:181-197), compute_mixed_value (:935-970), rescale_qvalues (:972-987).
    Returns (completed q, child visits, child priors) in legal order."""
    ch = [node.children[a] for a in node.legal]
    visits = [c.visit for c in ch]
    priors = [c.prior for c in ch]
    q = [F(c.reward + F(disc * c.value())) for c in ch]
    p = csoftmax(priors)
    vsum = F(0)
    for v in visits:
        vsum = F(vsum + F(v))
    p = [max(x, F(-10e7)) for x in p]
    psum = F(0)
    for x, v in zip(p, visits):
        if v > 0:
            psum = F(psum + x)
    wq = F(0)
    for x, v, qq in zip(p, visits, q):
        if v > 0:
            wq = F(wq + F(F(x * qq) / psum))
    mixed = F(F(node.raw_value + F(vsum * wq)) / F(vsum + F(1)))
    c = [qq if v > 0 else mixed for qq, v in zip(q, visits)]
    mx, mn = max(c), min(c)
    gap = max(F(mx - mn), F(1e-8))
    c = [F(F(x - mn) / gap) for x in c]
    scale = F(F(50.0) + F(max(visits)))
    c = [F(F(x * scale) * F(0.1)) for x in c]
    return c, visits, priors


def select_root(node, disc, S, m, gumbel):
    """cselect_root_child (:701-745) with score_considered (:1097-1132)."""
    c, visits, priors = completed_q(node, disc)
    considered = considered_visits(m, S)[sum(visits)]
    pm = max(priors)
    best, arg = node.legal[0], NEG_INF
    for j, a in enumerate(node.legal):
        s = F(F(gumbel[j] + F(priors[j] - pm)) + c[j])
        s = F(max(F(-1e9), s) + (F(0) if visits[j] == considered else NEG_INF))
        if s > arg:
            arg, best = s, a
    return best


def select_interior(node, disc):
    """cselect_interior_child (:747-790)."""
    c, visits, priors = completed_q(node, disc)
    probs = csoftmax([F(p + q) for p, q in zip(priors, c)])
    tot = sum(visits)
    best, arg = node.legal[0], NEG_INF
    for j, a in enumerate(node.legal):
        s = F(probs[j] - F(F(visits[j]) / F(1 + tot)))
        if s > arg:
            arg, best = s, a
    return best


class GumbelTree:
    """CRoots + CSearchResults + CMinMaxStatsList of one batch."""

    def __init__(self, legal_lists, A, gumbel=None):
        self.B, self.A = len(legal_lists), A
        self.gumbel = gumbel_table() if gumbel is None else gumbel
        self.roots = [Node(0, l) for l in legal_lists]
        self.minmax = [[FLOAT_MIN, F(1000000.0)] for _ in range(self.B)]  # CMinMaxStats::clear
        self.paths = None

    def prepare(self, noise_weight, noises, rewards, values, logits, to_play):
        """CRoots::prepare / prepare_no_noise (:418-455), add_exploration_noise (:158-175)."""
        f = F(noise_weight)
        for i, r in enumerate(self.roots):
            r.expand(int(to_play[i]), 0, rewards[i], values[i], logits[i])
            if noises is not None:
                for j, a in enumerate(r.legal):
                    c = r.children[a]
                    c.prior = F(F(c.prior * F(F(1) - f)) + F(F(noises[i][j]) * f))
            r.visit += 1

    def traverse(self, S, m, disc, vtp):
        """cbatch_traverse (:834-898) -> x, y, last actions, virtual_to_play, search_lens."""
        disc = F(disc)
        self.paths = []
        xs, ys, acts, lens = [], [], [], []
        for i, root in enumerate(self.roots):
            node, path, is_root, last = root, [root], True, -1
            while node.children:
                a = select_root(node, disc, S, m, self.gumbel) if is_root else select_interior(node, disc)
                is_root = False
                node.best = a
                node = node.children[a]
                last = a
                path.append(node)
            self.paths.append(path)
            xs.append(path[-2].latent)
            ys.append(i)
            acts.append(last)
            lens.append(len(path) - 1)
        return xs, ys, acts, list(vtp), lens

    def backprop(self, cur, disc, rewards, values, logits, to_play):
        """cbatch_back_propagate (:633-652) with cback_propagate (:605-631): no player sign anywhere."""
        disc = F(disc)
        for i, path in enumerate(self.paths):
            path[-1].expand(int(to_play[i]), cur, rewards[i], values[i], logits[i])
            b = F(values[i])
            mm = self.minmax[i]
            for node in reversed(path):
                node.value_sum = F(node.value_sum + b)
                node.visit += 1
                q = F(node.reward + F(disc * node.value()))
                mm[0], mm[1] = max(mm[0], q), min(mm[1], q)
                b = F(node.reward + F(disc * b))

    def distributions(self):
        return [[r.children[a].visit for a in r.legal] for r in self.roots]

    def values(self):
        return [r.value() for r in self.roots]

    def trajectories(self):  # CNode::get_trajectory (:263-283)
        out = []
        for r in self.roots:
            t, node = [], r
            while node.best >= 0:
                t.append(node.best)
                node = node.children[node.best]
            out.append(t)
        return out

    def children_values(self, disc):  # get_children_value (:309-338)
        out = np.full((self.B, self.A), -np.inf, np.float32)
        for i, r in enumerate(self.roots):
            c, _, _ = completed_q(r, F(disc))
            for j, a in enumerate(r.legal):
                out[i, a] = c[j]
        return out

    def policies(self, disc):  # get_policy (:355-385)
        out = np.zeros((self.B, self.A), np.float32)
        for i, r in enumerate(self.roots):
            c, _, priors = completed_q(r, F(disc))
            row = [NEG_INF] * self.A
            for j, a in enumerate(r.legal):
                row[a] = F(priors[j] + c[j])
            out[i] = csoftmax(row)
        return out


def legal_lists(g):
    """a transcript's root legal lists, in the order the reference was given them: the stored legal_lists
    (int32 [B, A], -1 padded) when present, the mask's ascending order otherwise"""
    if "legal_lists" in g.files:
        return [[int(a) for a in row if a >= 0] for row in g["legal_lists"]]
    B, A = g["legal_mask"].shape
    return [[a for a in range(A) if g["legal_mask"][i, a]] for i in range(B)]


def visits_full():
    """gmz_visits_full.npz as [(m, S, row)]: the reference's considered-visits row of every m in [0, 66] and
    S in {1..64, 100, 200}"""
    f = np.load(os.path.join(GOLDEN, "gmz_visits_full.npz"))
    rows = f["rows"]
    return [(int(m), int(S), rows[off:off + S].tolist()) for m, S, off in f["index"]]


def replay(g, feed=None):
    """Run the restatement over a transcript's inputs (a loaded gmz_*.npz) and its fed outputs (or `feed`: dict
    with resp_reward / resp_value / resp_logits). Returns the tree and the per-simulation requests."""
    B, S, A, m, noise = (int(v) for v in g["meta"])
    disc, nw = F(g["consts"][0]), F(g["consts"][1])
    legal = legal_lists(g)
    t = GumbelTree(legal, A)
    noises = [g["noises"][i, :len(legal[i])] for i in range(B)] if noise else None
    t.prepare(nw, noises, g["root_reward"], g["root_value"], g["root_logits"], g["to_play"])
    f = g if feed is None else feed
    req = {k: np.zeros((S, B), np.int32) for k in ("x", "y", "a", "vtp", "len")}
    for k in range(S):
        x, y, a, vtp, ln = t.traverse(S, m, disc, g["to_play"])
        req["x"][k], req["y"][k], req["a"][k], req["vtp"][k], req["len"][k] = x, y, a, vtp, ln
        t.backprop(k + 1, disc, f["resp_reward"][k], f["resp_value"][k], f["resp_logits"][k], g["to_play"])
    return t, req


def pad(rows, width, fill=-1):
    out = np.full((len(rows), max(1, width)), fill, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out
