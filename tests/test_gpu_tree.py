"""GPU: the HIP tree (traverse / backprop through the C ABI) against the reference's golden
transcripts and, at sizes beyond the fixtures, against the oracle on identical inputs.
Bit-exact: every request (x, y, action, virtual_to_play, search_len) of every simulation, the
final visit distributions, root values and best-action trajectories. The edge transcripts (tests/golden/tree/:
other constants, horizons, float regimes, paths past 64 levels, unsorted root lists) also run through the
mz_tree / ez_tree module API, and every transcript through the launch the search loop uses
(decode_backprop_traverse)."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.oracle import OracleTree, load_transcript, replay_transcript, transcript_legal  # noqa: E402
from tests.helpers import GpuTree, random_transcript, run_transcript  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRANSCRIPTS = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if not p.endswith("glibc_rand.npz") and not os.path.basename(p).startswith(("az_", "reuse_", "ptree_")))


# the setting, float, depth and list-order edges (tests/golden/gen_golden.py EDGE_CASES; tests/test_oracle.py asserts
# that none is missing)
EDGE_TRANSCRIPTS = sorted(glob.glob(os.path.join(GOLDEN, "tree", "*.npz")))


@pytest.mark.parametrize("path", TRANSCRIPTS + EDGE_TRANSCRIPTS, ids=lambda p: os.path.basename(p)[:-4])
def test_gpu_reproduces_reference_transcript(path):
    bad = replay_transcript(load_transcript(path), tree_factory=GpuTree)
    assert not bad, bad


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def lists_of(tr):
    """the root legal lists in the order the reference was given them"""
    legal, cnt = transcript_legal(tr)
    return [legal[i, :cnt[i]].tolist() for i in range(len(cnt))]


@pytest.mark.parametrize("path", EDGE_TRANSCRIPTS, ids=lambda p: os.path.basename(p)[:-4])
def test_module_api_replays_edge_transcript(path):
    """the list-in / list-out surface (mz_tree / ez_tree) over the edge transcripts: Roots with the unsorted lists,
    the transcript's own constants, delta and horizon; every request, search_len and the three outputs, trajectories
    longer than 64 whole"""
    from lightzero_amd.ctree import ez_tree, mz_tree
    from lightzero_amd.tree import set_seed_source
    tr = load_transcript(path)
    B, S, A, players, noise, ez, horizon = (int(v) for v in tr["meta"])
    base, init, disc, vdm, nw = (float(v) for v in tr["consts"])
    mod = ez_tree if ez else mz_tree
    legal = lists_of(tr)
    to_play = tr["to_play"].tolist()
    roots = mod.Roots(B, legal)
    if noise:
        roots.prepare(nw, [tr["noises"][i, :len(legal[i])].tolist() for i in range(B)], tr["root_reward"].tolist(),
                      tr["root_logits"].tolist(), to_play)
    else:
        roots.prepare_no_noise(tr["root_reward"].tolist(), tr["root_logits"].tolist(), to_play)
    mms = mod.MinMaxStatsList(B)
    mms.set_delta(vdm)
    seeds = iter(tr["seeds"].tolist())
    set_seed_source(lambda: next(seeds))
    try:
        for k in range(S):
            res = mod.ResultsWrapper(num=B)
            x, y, a, vtp = mod.batch_traverse(roots, int(base), init, disc, mms, res, list(to_play))
            assert x == tr["req_x"][k].tolist() and y == tr["req_y"][k].tolist(), k
            assert a == tr["req_a"][k].tolist() and vtp == tr["req_vtp"][k].tolist(), k
            slen = res.get_search_len()
            assert slen == tr["req_len"][k].tolist(), k
            args = (k + 1, disc, tr["resp_reward"][k].tolist(), tr["resp_value"][k].tolist(),
                    tr["resp_logits"][k].tolist(), mms, res)
            if ez:
                is_reset = [int(n % horizon == 0) for n in slen]
                assert is_reset == tr["resp_is_reset"][k].tolist(), k
                mod.batch_backpropagate(*args, is_reset, vtp)
            else:
                mod.batch_backpropagate(*args, vtp)
    finally:
        set_seed_source(None)
    dist = roots.get_distributions()
    assert dist == [[int(v) for v in row if v >= 0] for row in tr["out_dist"]]
    assert np.array_equal(bits(roots.get_values()), bits(tr["out_values"]))
    traj = roots.get_trajectories()
    assert traj == [[int(v) for v in row if v >= 0] for row in tr["out_traj"]]
    if tr["req_len"].max() > 64 and A == 1:
        assert max(len(t) for t in traj) > 64
    roots.clear()


@pytest.mark.parametrize("path", TRANSCRIPTS + EDGE_TRANSCRIPTS, ids=lambda p: os.path.basename(p)[:-4])
def test_decode_backprop_traverse_replays_transcripts(path):
    """the launch the search loop really uses (decode_backprop_traverse; decode_backprop for the last simulation)
    over every transcript's inputs: the scripted reward / value go in as scalar-head outputs, so the kernel decodes
    them (the inverse scalar transform) and the restatement is fed what the kernel decoded. EfficientZero: the
    kernel derives is_reset from the search length and the horizon itself."""
    from lightzero_amd.tree import DeviceTree, new_minmax, seed_tensor
    tr = load_transcript(path)
    B, S, A, players, noise, ez, horizon = (int(v) for v in tr["meta"])
    base, init, disc, vdm, nw = (float(v) for v in tr["consts"])
    init, disc, vdm, nw = (float(np.float32(v)) for v in (init, disc, vdm, nw))
    dev = torch.device("cuda", 0)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    legal, cnt = transcript_legal(tr)
    vtp_in = d(tr["to_play"], np.int32)
    t = DeviceTree(B, A, S, ez=bool(ez), device=dev)
    t.prepare(d(legal, np.int32), d(cnt, np.int32), d(tr["noises"], np.float32) if noise else None,
              nw if noise else 0.0, d(tr["root_reward"], np.float32), d(tr["root_logits"], np.float32), vtp_in)
    mm = new_minmax(B, vdm, dev)
    r, v = d(tr["resp_reward"][..., None], np.float32), d(tr["resp_value"][..., None], np.float32)
    p = d(tr["resp_logits"], np.float32)
    seeds = [seed_tensor(int(s), dev) for s in tr["seeds"]]
    decoded = torch.zeros((S, B, 2), dtype=torch.float32, device=dev)
    req = torch.zeros((S, 5, B), dtype=torch.int32, device=dev)
    resets = torch.zeros((S, B), dtype=torch.int32, device=dev)
    kw = dict(lstm_horizon=horizon, out_is_reset=t.is_reset) if ez else {}
    t.traverse(mm, seeds[0], vtp_in, int(base), init, disc)
    for k in range(S):
        req[k] = torch.stack([t.x, t.y, t.action, t.vtp, t.search_len])
        args = (k + 1, disc, mm, r[k], v[k], False, p[k], t.vtp)
        if k + 1 < S:
            t.decode_backprop_traverse(*args, seeds[k + 1], vtp_in, int(base), init, out_decoded=decoded[k], **kw)
        else:
            t.decode_backprop(*args, out_decoded=decoded[k], **kw)
        resets[k] = t.is_reset
    dec, req, resets = decoded.cpu().numpy(), req.cpu().numpy(), resets.cpu().numpy()
    got = dict(dist=t.distributions().cpu().numpy(), values=t.values().cpu().numpy(),
               traj=t.trajectories(S + 2).cpu().numpy(), mm=mm[:, :2].cpu().numpy())
    t.check_errors()
    t.close()
    assert np.all(np.isfinite(dec))
    if ez:
        assert np.array_equal(resets, (req[:, 4] % horizon == 0).astype(np.int32))
    ot = OracleTree(B, A, S, ez=bool(ez))
    ot.set_legal(legal, cnt)
    ot.set_delta(np.float32(vdm))
    ot.prepare(np.float32(nw), tr["noises"] if noise else None, tr["root_reward"], tr["root_logits"], tr["to_play"])
    for k in range(S):
        out = ot.traverse(base, np.float32(init), np.float32(disc), int(tr["seeds"][k]), tr["to_play"])
        for j, key in enumerate(("x", "y", "a", "vtp", "len")):
            assert np.array_equal(req[k, j], out[j]), (key, k)
        ot.backprop(k + 1, np.float32(disc), dec[k, :, 0], dec[k, :, 1], tr["resp_logits"][k], out[3],
                    (out[4] % horizon == 0).astype(np.int32) if ez else None)
    assert np.array_equal(got["dist"], ot.distributions())
    assert np.array_equal(got["traj"], ot.trajectories(S + 2))
    assert np.array_equal(bits(got["values"]), bits(ot.values()))
    # the min-max pair: the same bits, but for the sign of a zero. The reference keeps the first zero a backup meets
    # (`if (v > maximum)` is false between +0 and -0); the device takes an order-free wave max / min, for which the
    # two zeros are one value. h^-1(0) = 0 * (a negative rounding residue) = -0, so the zero-net transcripts meet both.
    # No output can tell: mm_normalize reads the pair through maximum - minimum and v - minimum only, and a -0 score
    # is added to a prior term that is never -0.
    want = ot.minmax()
    zero = (got["mm"] == 0) & (want == 0)
    assert np.array_equal(np.where(zero, 0, bits(got["mm"])), np.where(zero, 0, bits(want)))


def assert_same(a, b):
    for k in ("x", "y", "a", "vtp", "len", "dist", "traj"):
        if not np.array_equal(a[k], b[k]):
            idx = np.argwhere(a[k] != b[k])[:5]
            raise AssertionError(f"{k} differs at {idx.tolist()}")
    assert np.array_equal(a["values"], b["values"]), np.abs(a["values"] - b["values"]).max()


CASES = [
    # (B, S, A, players, ez, net, ragged)
    (256, 50, 2, 1, False, "rand", False),
    (256, 50, 2, 1, False, "zero", False),
    (256, 50, 2, 2, False, "quant", False),
    (512, 100, 9, 2, False, "rand", True),
    (1024, 50, 4, 1, False, "quant", False),
    (2048, 30, 4, 1, False, "rand", False),  # > one workgroup of roots per traverse round
    (1, 20, 1, 1, False, "rand", False),
    (3, 15, 64, 1, False, "rand", True),
    (100, 40, 6, 1, True, "rand", False),
    (64, 50, 18, 2, True, "quant", True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b{}_s{}_a{}_p{}_{}_{}{}".format(
    c[0], c[1], c[2], c[3], "ez" if c[4] else "mz", c[5], "_ragged" if c[6] else ""))
def test_gpu_matches_oracle_parity_mode(case):
    B, S, A, players, ez, net, ragged = case
    tr = random_transcript(B, S, A, seed=B + S + A, players=players, ez=ez, net=net, ragged=ragged)
    assert_same(run_transcript(tr, GpuTree), run_transcript(tr, OracleTree))


@pytest.mark.parametrize("case", [(256, 50, 2, 1, False), (512, 30, 9, 2, False), (128, 40, 6, 1, True)])
def test_gpu_matches_oracle_fast_mode(case):
    B, S, A, players, ez = case
    tr = random_transcript(B, S, A, seed=7 * B + S, players=players, ez=ez, net="quant")
    assert_same(run_transcript(tr, GpuTree, fast_rng=True), run_transcript(tr, OracleTree, fast_rng=True))


def test_empty_legal_list_means_all_actions():
    # CNode::expand fills 0..A-1 when legal_actions is empty (cnode.cpp:101-107)
    tr = random_transcript(8, 10, 3, seed=1)
    B, A = 8, 3
    gt = GpuTree(B, A, 10)
    ot = OracleTree(B, A, 10)
    legal = np.full((B, A), -1, np.int32)
    cnt = np.zeros(B, np.int32)
    gt.set_legal(legal, cnt)
    full = np.tile(np.arange(A, dtype=np.int32), (B, 1))
    ot.set_legal(full, np.full(B, A, np.int32))
    for t in (gt, ot):
        t.set_delta(np.float32(0.01))
        t.prepare(np.float32(0.25), tr["noises"][:, :A], tr["root_reward"], tr["root_logits"], tr["to_play"])
    for k in range(10):
        og = gt.traverse(19652, np.float32(1.25), np.float32(0.997), k + 11, tr["to_play"])
        oo = ot.traverse(19652, np.float32(1.25), np.float32(0.997), k + 11, tr["to_play"])
        assert all(np.array_equal(a, b) for a, b in zip(og, oo))
        for t, o in ((gt, og), (ot, oo)):
            t.backprop(k + 1, np.float32(0.997), tr["resp_reward"][k], tr["resp_value"][k], tr["resp_logits"][k], o[3])
    assert np.array_equal(gt.distributions(), ot.distributions())


def test_module_api_matches_oracle_and_grows_capacity():
    """mz_tree-compatible list API (mz_tree.pyx surface); 80 simulations > default capacity."""
    from lightzero_amd.ctree import mz_tree
    from lightzero_amd.tree import SequentialSeeds, set_seed_source
    B, S, A = 40, 80, 3
    tr = random_transcript(B, S, A, seed=99)
    roots = mz_tree.Roots(B, [list(range(A)) for _ in range(B)])
    roots.prepare(0.25, [r.tolist() for r in tr["noises"]], [0.0] * B, tr["root_logits"].tolist(), [-1] * B)
    mms = mz_tree.MinMaxStatsList(B)
    mms.set_delta(0.01)
    ot = OracleTree(B, A, S)
    ot.set_delta(np.float32(0.01))
    ot.prepare(np.float32(0.25), tr["noises"], np.zeros(B, np.float32), tr["root_logits"], np.full(B, -1, np.int32))
    set_seed_source(SequentialSeeds(99))
    try:
        for k in range(S):
            res = mz_tree.ResultsWrapper(num=B)
            x, y, a, vtp = mz_tree.batch_traverse(roots, 19652, 1.25, 0.997, mms, res, [-1] * B)
            ox, oy, oa, ovtp, olen = ot.traverse(19652, np.float32(1.25), np.float32(0.997),
                                                 (1000003 * 99 + k) % 1000000, np.full(B, -1, np.int32))
            assert x == ox.tolist() and y == oy.tolist() and a == oa.tolist() and vtp == ovtp.tolist()
            assert res.get_search_len() == olen.tolist()
            mz_tree.batch_backpropagate(k + 1, 0.997, tr["resp_reward"][k % tr["resp_reward"].shape[0]].tolist(),
                                        tr["resp_value"][k].tolist(), tr["resp_logits"][k].tolist(), mms, res, vtp)
            ot.backprop(k + 1, np.float32(0.997), tr["resp_reward"][k], tr["resp_value"][k], tr["resp_logits"][k],
                        ovtp)
    finally:
        set_seed_source(None)
    assert roots.get_distributions() == [[int(v) for v in row] for row in ot.distributions()]
    assert np.array_equal(np.array(roots.get_values(), np.float32), ot.values())
    traj = ot.trajectories(S + 2)
    assert roots.get_trajectories() == [[int(v) for v in row if v >= 0] for row in traj]


def test_parity_traverse_leaves_error_words_clean():
    """A parity-mode search through traverse / backprop sets no sticky error word (look-back timeout,
    draw-table overflow)."""
    B, S, A = 256, 30, 2
    tr = random_transcript(B, S, A, seed=5)
    gt = GpuTree(B, A, S)
    from oracle.oracle import legal_from_mask
    legal, cnt = legal_from_mask(tr["legal_mask"])
    gt.set_legal(legal, cnt)
    gt.set_delta(np.float32(0.01))
    gt.prepare(np.float32(0.25), tr["noises"], tr["root_reward"], tr["root_logits"], tr["to_play"])
    for k in range(S):
        o = gt.traverse(19652, np.float32(1.25), np.float32(0.997), int(tr["seeds"][k]), tr["to_play"])
        gt.backprop(k + 1, np.float32(0.997), tr["resp_reward"][k], tr["resp_value"][k], tr["resp_logits"][k], o[3])
    gt.t.check_errors()  # raises on a look-back timeout / draw-table overflow (sticky err words)
