"""Plain numpy-float32 restatement of LightZero's Sampled EfficientZero tree (test infrastructure; the package never
imports it): ctree_sampled_efficientzero/lib/cnode.cpp, line numbers of that file. Every tree quantity is a float32
scalar summed in the C++ loops' order; cucb_score's logf / sqrtf are the host libm's (nm -D, gen_golden_sampled.py).

A node has K slots whatever was sampled and the prior is uniform (cnode.cpp:1076-1079). The random
choices are callables: tie_draw(level, root) -> cselect_child's rand() (:1019), sampler(L, root, policy_row) -> the K
actions of the node simulation L expands. glibc_draws replays the reference's transcripts; philox_draws /
philox_sampler are the device's rule (include/lzmcts.h) and make this module the yardstick for the kernels.
"""
import numpy as np

from oracle.collect_rng import philox4x32_10, u01
from stochastic_oracle import F, FLOAT_MIN, MinMax, _libm, glibc_draws  # noqa: F401  (same libm, same rand stream)

KEY, PB_C, VDM, HORIZON, DISC = 0x53414d50, (19652, 1.25), 0.01, 5, 0.997


def scripted(B, S, K, dim, cont, players=1, net="rand", seed=0):
    """a search's inputs, the network as tables of (simulation, root); continuous policy rows are {mu, sigma > 0}"""
    rng = np.random.default_rng(7000 + 31 * seed + B + 13 * S + K)
    draw = (lambda *s: np.zeros(s, np.float32)) if net == "zero" else (
        lambda *s: rng.normal(0.0, 1.0, size=s).astype(np.float32))
    policy = (lambda *s: np.concatenate([rng.uniform(-1, 1, size=s + (dim,)), rng.uniform(0.2, 1.5, size=s + (dim,))],
                                        axis=-1).astype(np.float32)) if cont else (lambda *s: draw(*s, dim))
    return dict(to_play=np.array([1 + (i * 7) % 2 for i in range(B)] if players == 2 else [-1] * B, np.int32),
                root_vp=draw(B), root_policy=policy(B), resp_vp=draw(S, B) * np.float32(0.5), resp_value=draw(S, B),
                resp_policy=policy(S, B), seeds=rng.integers(0, 1000000, size=S), root_seed=int(rng.integers(2 ** 31)),
                meta=np.array([B, S, K, dim, int(cont)], np.int64))


def philox_draws(seed):
    key = [int(seed) & 0xFFFFFFFF, KEY]
    return lambda level, root: int(philox4x32_10([level, root, 0, 0], key)[0]) >> 1


def gaussian_z(seed, L, root, K, D):
    """the D standard normals of each of K slots, float64 [K, D]: Box-Muller pairs from counters
    (L, root, 2 | slot << 8, m)"""
    P = (D + 1) // 2
    ctr = np.zeros((K, P, 4), np.uint64)
    ctr[..., 0], ctr[..., 1] = L, root
    ctr[..., 2], ctr[..., 3] = (2 | (np.arange(K) << 8))[:, None], np.arange(P)[None, :]
    o = philox4x32_10(ctr, [int(seed) & 0xFFFFFFFF, KEY])
    r, a = np.sqrt(-2.0 * np.log(u01(o[..., 0], o[..., 1]))), 6.283185307179586 * u01(o[..., 2], o[..., 3])
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).reshape(K, 2 * P)[:, :D]


def discrete_probs(logits):
    """p_a of cnode.cpp:326-334: float exp and float running sum, the quotient in double, stored as float"""
    e = [F(_libm.expf(F(l))) for l in logits]
    s = F(0)
    for v in e:
        s = F(s + v)
    return np.array([F(float(v) / (float(s) + 1e-6)) for v in e], F)


def philox_sampler(seed, K, continuous):
    """sampler(L, root, row) -> float32 [K, D] (tanh-squashed) or int32 [K] under the device's counters"""
    def cont(L, root, row):
        D = len(row) // 2
        x = (row[:D].astype(np.float64) + row[D:].astype(np.float64) * gaussian_z(seed, L, root, K, D)).astype(F)
        return np.tanh(x.astype(np.float64)).astype(F)

    def disc(L, root, row):
        o = philox4x32_10([[L, root, 3, a] for a in range(len(row))], [int(seed) & 0xFFFFFFFF, KEY])
        with np.errstate(divide="ignore"):
            k = np.power(u01(o[:, 0], o[:, 1]), 1.0 / discrete_probs(row).astype(np.float64))
        return np.lexsort((np.arange(len(row)), -k))[:K].astype(np.int32)  # descending key, lower action first
    return cont if continuous else disc


class Node:
    def __init__(self):
        self.visit, self.value_sum, self.vp, self.is_reset = 0, F(0), F(0), 0
        self.to_play, self.latent, self.best, self.children, self.actions = 0, -1, -1, [], None

    def value(self):
        return F(0) if self.visit == 0 else F(self.value_sum / F(self.visit))

    def expand(self, K, to_play, latent, vp, actions):  # :194-452
        self.to_play, self.latent, self.vp, self.actions = int(to_play), latent, F(vp), actions
        self.children = [Node() for _ in range(K)]

    def true_reward(self, c):
        return c.vp if self.is_reset == 1 else F(c.vp - self.vp)


def select(node, mm, disc, mean_q, players, draw):  # cselect_child, cucb_score :973-1108
    N, base = F(node.visit - 1), F(PB_C[0])
    pbc0 = F(F(_libm.logf(F(F(F(N + base) + F(1)) / base))) + F(PB_C[1]))
    sq, best, lst = F(_libm.sqrtf(N)), FLOAT_MIN, []
    for j, c in enumerate(node.children):
        vs = mean_q if c.visit == 0 else F(
            node.true_reward(c) + F(disc * (c.value() if players == 1 else F(-c.value()))))
        score = F(F(F(pbc0 * F(sq / F(c.visit + 1))) / F(len(node.children))) + min(max(mm.normalize(vs), F(0)), F(1)))
        if best < score:
            best, lst = score, [j]
        elif score >= F(best - F(0.000001)):
            lst.append(j)
    return lst[draw() % len(lst)]


def traverse(root, i, mm, disc, players, vtp, tie_draw):  # cbatch_traverse :1145-1186 -> (path, slot, vtp)
    path, parent_q, slot = [root], F(0), -1
    while path[-1].children:
        node, tq, tv, level = path[-1], F(0), 0, len(path) - 1
        for c in node.children:  # compute_mean_q :483-523
            if c.visit > 0:
                tq, tv = F(tq + F(node.true_reward(c) + F(disc * c.value()))), tv + 1
        parent_q = F(tq / F(tv)) if level == 0 and tv > 0 else F(F(parent_q + tq) / F(tv + 1))
        slot = node.best = select(node, mm, disc, parent_q, players, lambda: tie_draw(level, i))
        vtp = vtp if players == 1 else 3 - vtp
        path.append(node.children[slot])
    return path, slot, vtp


def backprop(path, mm, disc, tp, value):  # cbackpropagate :860-945
    b = F(value)
    for l in range(len(path) - 1, -1, -1):
        node, same = path[l], tp == -1 or path[l].to_play == tp
        node.value_sum, node.visit = F(node.value_sum + (b if same else F(-b))), node.visit + 1
        pvp, reset = (path[l - 1].vp, path[l - 1].is_reset) if l >= 1 else (F(0), 0)
        mm.update(F(F(node.vp - pvp) + F(disc * node.value())))
        tr = node.vp if reset == 1 else F(node.vp - pvp)
        b = F(F(-tr if tp != -1 and node.to_play == tp else tr) + F(disc * b))


def replay(g, tie_draws, sampler=None):
    """Runs g's search (scripted()'s tables) with tie_draws(k) -> simulation k's tie_draw and sampler(k) -> the sampler
    of the node it expands (-1: the roots) -> a transcript's arrays, the best slot paths and, with a sampler, actions"""
    B, S, K = (int(v) for v in g["meta"][:3])
    sm, disc = sampler or (lambda k: (lambda L, i, row: [None] * K)), F(DISC)
    roots, mms = [Node() for _ in range(B)], [MinMax(VDM) for _ in range(B)]
    for i, r in enumerate(roots):  # CRoots::prepare_no_noise :699-715
        r.expand(K, g["to_play"][i], 0, g["root_vp"][i], sm(-1)(0, i, g["root_policy"][i]))
        r.visit += 1
    players = 1 if max(g["to_play"]) == -1 else 2
    req = {k: np.zeros((S, B), np.int32) for k in ("x", "y", "slot", "vtp", "len")}
    acts = []
    for k in range(S):  # (roots are independent: each root's walk and backup in turn, the draws in batch order)
        draw = tie_draws(k)
        for i, r in enumerate(roots):
            path, slot, vtp = traverse(r, i, mms[i], disc, players, int(g["to_play"][i]), draw)
            for n, v in zip(req, (path[-2].latent, i, slot, vtp, len(path) - 1)):
                req[n][k, i] = v
            acts.append(path[-2].actions[slot])
            path[-1].expand(K, vtp, k + 1, g["resp_vp"][k, i], sm(k)(k + 1, i, g["resp_policy"][k, i]))
            path[-1].is_reset = int((len(path) - 1) % HORIZON == 0)  # :967, mcts_ctree_sampled.py:215
            backprop(path, mms[i], disc, vtp, g["resp_value"][k, i])
    res = {"req_" + k: v for k, v in req.items()}
    best = lambda n: [] if n.best < 0 else [n.best] + best(n.children[n.best])
    res.update(out_dist=np.array([[c.visit for c in r.children] for r in roots], np.int32),
               out_values=np.array([r.value() for r in roots], F), traj=[best(r) for r in roots])
    if sampler is not None:
        res.update(req_action=np.array(acts).reshape((S, B) + np.shape(acts[0])),
                   root_actions=np.stack([r.actions for r in roots]))
    return res
