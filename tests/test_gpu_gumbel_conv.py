"""GPU: the one-launch Gumbel MuZero search of the conv MuZeroModel (lzm_search_conv_gumbel: search_conv_kernel's
Gumbel instantiation) behind GumbelMuZeroMCTSCtree with cfg.fused_conv_search set.

Every case builds a conv MuZeroModel (tests/test_gpu_conv_shapes.make_model("mz", ...): observation 4 x 64 x 64,
64 x 8 x 8 latent, BatchNorm with non-trivial statistics), feeds the search random non-negative root latents, random
root logits, root values and Dirichlet noises, and runs it twice with the same model and inputs, each on a tree of
its own reserved for 64 simulations:

  * one launch (cfg.fused_conv_search=True), asserting last_path == "fused-conv" and the plan the library reports
    (DeviceTree.search_conv_gumbel_plan, the function the launch decides with): workgroups, slices, roots per slice
    and LDS bytes <= 160 KiB;
  * the generic eager per-simulation path (the key absent), asserting "generic" with the native trunk.

It asserts equality by bits of the visit distributions, root values, improved policies, children's completed Q,
trajectories, min-max pairs, every simulation's request (x, action, search_len, vtp), decoded {reward, value}, policy
logits and the whole latent pool; test_gpu_gumbel.assert_matches_restatement on the one-launch result (the host
restatement pinned to the reference's transcripts); and, on one case, the decoded values against the torch module
(test_gpu_conv.torch_replay with its own bounds). Nothing else here has a tolerance.

Seeds: every case uses the first seed of 1, 2, ... whose one-launch search reaches search_len >= min(2, S) at some
root (>= 3 in the depth case), found on the GPU; the test asserts the condition. Sequential halving revisits a root
child as soon as the considered visit count rises above 0 or no legal child has it, so seed 1 met it in every case
(the 1,030-root case, two simulations over two actions, through its two one-action roots: see CASES).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_gumbel as tg  # noqa: E402
import test_gpu_gumbel_fused as tf  # noqa: E402
from lightzero_amd import _lib  # noqa: E402
from tests.test_gpu_conv import torch_replay  # noqa: E402
from tests.test_gpu_conv_shapes import make_model  # noqa: E402

DEV = torch.device("cuda", 0)
LDS_LIMIT = 160 * 1024
RAGGED9 = [[3], [1, 7], list(range(9)), [8, 2, 5], [4, 6, 0, 1, 2]]  # one action; two and three < m = 4; unsorted


def sharpen(model, k):
    """the last linear layer of the policy, value and reward heads times k (test_gpu_gumbel.sharpen_heads for the
    conv model's head names)"""
    with torch.no_grad():
        for head in (model.prediction_network.fc_policy, model.prediction_network.fc_value,
                     model.dynamics_network.fc_reward_head):
            last = [mod for mod in head.modules() if isinstance(mod, torch.nn.Linear)][-1]
            last.weight.mul_(k)
            last.bias.mul_(k)
    return model


def value_scale(model, categorical):
    return (model.prediction_network.fc_value[-1].out_features - 1) // 2 if categorical else 1


def inputs(B, A, legal, seed):
    rng = np.random.default_rng(1000 + seed)
    lat0 = torch.from_numpy(np.maximum(rng.standard_normal((B, 64, 8, 8)), 0).astype(np.float32)).to(DEV)
    legal = [list(range(A))] * B if legal is None else [list(l) for l in legal]
    noises = np.zeros((B, A), np.float32)
    for i, l in enumerate(legal):
        noises[i, :len(l)] = rng.dirichlet([0.3] * len(l)).astype(np.float32)
    return dict(lat0=lat0, logits0=rng.standard_normal((B, A)).astype(np.float32), legal=legal, noises=noises,
                root_value=rng.normal(size=B).astype(np.float32))


def make_mcts(S, m, scale, discount=0.997, categorical=True, fused=True, max_roots=0, record=True, graph=False):
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    cfg = dict(num_simulations=S, max_num_considered_actions=m, discount_factor=discount, device=DEV,
               use_hip_graph=graph, env_type='not_board_games', sliced_search_max_roots=max_roots,
               model=dict(support_scale=scale, categorical_distribution=categorical))
    if fused:  # (the generic side leaves the key absent: the default)
        cfg["fused_conv_search"] = True
    mcts = GumbelMuZeroMCTSCtree(EasyDict(cfg))
    mcts.record = record
    return mcts


prepare = tf.prepare  # (roots, inputs, noise, to_play): Roots.prepare / prepare_no_noise from the host lists


def run(model, x, S, m, fused, noise=True, discount=0.997, categorical=True, to_play=None, max_roots=0, reserve=64,
        path=None):
    """one search of `model` over the inputs `x` on a tree of its own; path: what last_path must be (default: the
    one launch when fused, else the generic path)"""
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    from lightzero_amd.tree import DeviceTree
    B, A = len(x["legal"]), model.action_space_size
    to_play = [-1] * B if to_play is None else list(to_play)
    mcts = make_mcts(S, m, value_scale(model, categorical), discount, categorical, fused, max_roots)
    roots = GumbelMuZeroMCTSCtree.roots(B, x["legal"])
    roots.tree = DeviceTree(B, A, reserve, gumbel=True, device=DEV)
    prepare(roots, x, noise, to_play)
    mcts.search(roots, model, x["lat0"], to_play)
    assert mcts.last_path == (path or ("fused-conv" if fused else "generic")), mcts.last_path
    roots.tree.check_errors()  # (raises on a split-range error of the trunk)
    net = mcts._folded.get(model)
    assert net.native is not None  # both sides: the split-precision trunk on the latent pool
    disc = float(np.float32(discount))
    scale = value_scale(model, categorical)
    return dict(out=tg.device_outputs(roots, disc, A, S), roots=roots, mcts=mcts, legal=x["legal"],
                noises=x["noises"] if noise else None, root_value=x["root_value"], logits0=x["logits0"], disc=disc,
                to_play=to_play, rec=mcts.last_record.numpy(), model=model, pool=mcts._buf.pool.clone(),
                mm=roots._last_minmax[:, :2].cpu().numpy().copy(), plan=mcts.last_plan, net=net, lat0=x["lat0"],
                scale=scale, scales=(scale, scale), categorical=categorical)


def finish(*rs):
    for r in rs:
        t = r["roots"].tree
        r["roots"].tree = None
        t.close()


def assert_plan(plan, B, max_roots=0):
    per = min(B, 1024, max_roots or 1024)
    n = -(-B // per)
    assert plan["supported"] and plan["code"] == 0, plan
    assert plan["workgroups"] == per and plan["slices"] == n and plan["slice_roots"] == per, plan
    assert plan["last_slice_roots"] == B - (n - 1) * per, plan
    assert 0 < plan["lds_bytes"] <= LDS_LIMIT, plan


def f_slices(B, max_roots=0):
    """(slices, roots per slice, roots in the last slice) of lzm_conv_slice_roots' MuZero rule"""
    per = min(B, 1024, max_roots or 1024)
    n = -(-B // per)
    return n, per, B - (n - 1) * per


def assert_same_bits(f, g):
    """everything the two paths leave behind, by bits"""
    for k in ("dist", "traj"):
        assert np.array_equal(f["out"][k], g["out"][k]), k
    for k in ("values", "policies", "children"):
        assert tg.same_bits(f["out"][k], g["out"][k]), k
    assert tg.same_bits(f["mm"], g["mm"]), "minmax"
    for k in ("x", "action", "search_len", "vtp"):
        assert np.array_equal(f["rec"][k], g["rec"][k]), k
    for k in ("decoded", "policy_logits"):
        assert tg.same_bits(f["rec"][k], g["rec"][k]), k
    assert torch.equal(f["pool"].view(torch.int32), g["pool"].view(torch.int32)), "latent pool"


def both(model, B, A, S, m, seed=1, legal=None, max_roots=0, min_len=2, **kw):
    x = inputs(B, A, legal, seed)
    f = run(model, x, S, m, True, max_roots=max_roots, **kw)
    g = run(model, x, S, m, False, **kw)
    assert_plan(f["plan"], B, max_roots)
    assert g["plan"] is None
    assert_same_bits(f, g)
    tg.assert_matches_restatement(f, A, S, m)
    deepest = int(f["rec"]["search_len"].max())
    print(f"B={B} A={A} S={S} m={m} seed={seed}: deepest search_len {deepest}, plan {f['plan']}")
    assert deepest >= min(min_len, S), deepest
    return f, g


# ------------------------------------------------------------------------------------------- shapes
def c(id, B, A, S, m, model=None, search=None, **extra):
    return pytest.param(dict(B=B, A=A, S=S, m=m, model=model or {}, search=search or {}, **extra), id=id)


CASES = [
    c("atari-heads", 5, 4, 8, 4, torch=True),
    c("blocks0", 5, 4, 8, 4, dict(blocks=0)),
    c("blocks2", 5, 4, 8, 4, dict(blocks=2)),
    c("one-simulation", 7, 6, 1, 4),
    c("m1", 4, 6, 12, 1),
    c("m-above-S-and-A", 4, 3, 5, 16),
    c("one-action", 6, 1, 8, 4),
    c("depth", 7, 2, 16, 2, min_len=3),
    c("support601-A18", 5, 18, 20, 16),
    c("ragged-A9", 5, 9, 12, 4, search=dict(legal=RAGGED9)),
    c("to-play", 4, 4, 8, 4, search=dict(to_play=[1, 2, 2, 1])),
    c("discount1", 4, 4, 8, 4, search=dict(discount=1.0)),
    c("no-noise", 4, 4, 8, 4, search=dict(noise=False)),
    c("scalar-heads", 4, 4, 8, 4, dict(cat=False), dict(categorical=False), out_rounds=1),
    c("n2-768", 4, 4, 8, 4, dict(Vr=383, Vv=381), out_rounds=1),
    c("n2-769", 4, 5, 8, 4, dict(Vr=383, Vv=381), out_rounds=2),   # the second round holds one column
    c("zero-heads", 5, 4, 8, 4, zero=True),
    c("heads-x30", 5, 4, 8, 4, sharpen=30),     # (measured: the policy logits spread 9.8 at most: no zero prior yet)
    c("heads-x400", 5, 4, 8, 4, sharpen=400),   # spread past 104: expf underflows, priors that are exact zeros
    c("more-roots-than-cus", 300, 2, 4, 2),
    c("three-slices", 8, 4, 8, 4, max_roots=3),
    # two simulations over two legal actions with m = 2 visit each child once, whatever the inputs: the first and
    # the last root (one in either slice) hold one action, so their second walk goes below the child
    c("default-slice-rule", 1030, 2, 2, 2, search=dict(legal=[[1]] + [[0, 1]] * 1028 + [[0]])),
]


@pytest.mark.parametrize("case", CASES)
def test_one_launch_equals_generic_and_restatement(case):
    B, A, S, m = case["B"], case["A"], case["S"], case["m"]
    model = make_model("mz", 101 + B + A, zero=case.get("zero", False), A=A, **case["model"])
    if case.get("sharpen"):
        sharpen(model, case["sharpen"])
    kw = dict(case["search"])
    if B == 1030:
        assert f_slices(B) == (2, 1024, 6)
    f, g = both(model, B, A, S, m, max_roots=case.get("max_roots", 0), min_len=case.get("min_len", 2), **kw)
    rec = f["rec"]
    hp = f["net"].heads  # the output loop's rounds of 768 columns over [reward | value | policy]
    assert f["plan"]["out_rounds"] == -(-(hp["Vr"] + hp["Vv"] + A) // 768) == case.get("out_rounds", 2)
    if "to_play" in kw:  # passes through: every request and every expanded node carry the root's
        assert rec["vtp"].tolist() == [kw["to_play"]] * S
    if case.get("zero"):  # every tie to the first legal action: the walks are the restatement's all the same
        assert np.all(rec["policy_logits"] == rec["policy_logits"][..., :1]) and np.all(rec["decoded"] == 0)
    if case.get("sharpen"):
        assert np.all(np.isfinite(rec["decoded"])) and np.all(np.isfinite(rec["policy_logits"]))
        spread = float(np.ptp(rec["policy_logits"], axis=-1).max())
        print(f"heads x{case['sharpen']}: policy logit spread per row, max {spread}")
        if case["sharpen"] >= 400:
            assert spread > 104, spread
    if kw.get("legal") is RAGGED9:
        dist = f["out"]["dist"]
        assert dist[0, 0] == S and dist[0, 1:].max() <= 0          # the one-action root
        assert dist[1, :2].sum() == S and dist[3, :3].sum() == S   # fewer legal actions than m: legal[0] fallback
    if case.get("torch"):
        torch_replay("mz", f, B, S)
    finish(f, g)


# ------------------------------------------------------------------------------------------- the LDS boundary
def largest_supported_S(B, A, net):
    """the largest S whose plan the library accepts on a tree reserved for exactly S simulations (the plan grows
    with the reservation: doubling, then bisection; host queries only)"""
    from lightzero_amd.tree import DeviceTree

    def ok(S):
        t = DeviceTree(B, A, S, gumbel=True, device=DEV)
        plan = t.search_conv_gumbel_plan(net, S)
        t.close()
        assert plan["supported"] or plan["code"] == _lib.LZM_ERR_ARG, plan
        return plan["supported"]
    lo = 8
    assert ok(lo)
    hi = 2 * lo
    while ok(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def test_lds_boundary():
    """A = 18: the largest S the plan accepts runs as one launch; S + 1 is refused for its LDS need (LZM_ERR_ARG from
    the plan), takes the generic path without raising and still matches the restatement"""
    B, A, m = 2, 18, 16
    model = make_model("mz", 77, A=A)
    probe = run(model, inputs(B, A, None, 1), 8, m, True)
    S = largest_supported_S(B, A, probe["net"])
    finish(probe)
    print("largest S the plan accepts at A = 18:", S)
    x = inputs(B, A, None, 1)
    f = run(model, x, S, m, True, reserve=S)
    assert_plan(f["plan"], B)
    assert f["plan"]["lds_bytes"] > LDS_LIMIT - 1024 - 18 * 36 - 64  # within one simulation's nodes of the limit
    tg.assert_matches_restatement(f, A, S, m)
    g = run(model, x, S + 1, m, True, reserve=S + 1, path="generic")
    assert g["plan"]["supported"] is False and g["plan"]["code"] == _lib.LZM_ERR_ARG and "LDS" in g["plan"]["reason"]
    tg.assert_matches_restatement(g, A, S + 1, m)
    finish(f, g)


# ------------------------------------------------------------------------------------------- refusals
def conv_args(net, S, m, mm, vtp, pool, max_roots=0):
    """lzm_search_conv_gumbel's arguments after the handle"""
    p, hp = _lib.ptr, net.heads
    return (S, m, 0.997, p(mm), p(vtp), p(pool), p(net.native), p(net.actmap), int(net.n_dres), int(net.n_pres),
            int(net.r_ch), int(net.h_ch), p(hp["w1t"]), p(hp["b1"]), p(hp["w2q"]), p(hp["b2"]), int(hp["Kr"]),
            int(hp["Khd"]), int(hp["off_policy"]), int(hp["Vr"]), int(hp["Vv"]), 1, None, None, None, None, None,
            max_roots, _lib.stream_ptr())


def test_refusals_before_any_launch():
    from lightzero_amd.tree import DeviceTree
    B, A, S, m = 4, 4, 8, 4
    model = make_model("mz", 5, A=A)
    x = inputs(B, A, None, 1)
    r = run(model, x, S, m, True, reserve=S)   # a searched Gumbel tree: its bytes must survive every refusal
    net, gt = r["net"], r["roots"].tree
    mt = DeviceTree(B, A, S, device=DEV)
    sentinel = torch.full((B, 4), 7.0, device=DEV)
    mm = sentinel.clone()
    vtp = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    pool = torch.zeros((S + 2, B, 64, 8, 8), device=DEV)
    seeds = torch.zeros(S + 1, dtype=torch.int32, device=DEV)
    L, p = _lib.load(), _lib.ptr

    def snapshot():
        return {k: v.copy() for k, v in tg.device_outputs(r["roots"], r["disc"], A, S).items()}

    def gumbel(h, sims=S, considered=m, max_roots=0):
        rc = L.lzm_search_conv_gumbel(h, *conv_args(net, sims, considered, mm, vtp, pool, max_roots))
        return rc, L.lzm_last_error().decode()

    before = snapshot()
    assert gt.search_conv_gumbel_plan(net, S)["supported"]
    # a MuZero handle to lzm_search_conv_gumbel (and to its plan)
    plan = mt.search_conv_gumbel_plan(net, S)
    assert plan["code"] == _lib.LZM_ERR_STATE and plan["slices"] == 0 and not plan["supported"], plan
    rc, msg = gumbel(mt.h)
    assert rc == _lib.LZM_ERR_STATE and msg.startswith("lzm_search_conv_gumbel:"), (rc, msg)
    with pytest.raises(_lib.LzmError):
        mt.search_conv_gumbel(net, S, m, mm, vtp, pool)
    # a Gumbel handle to lzm_search_conv
    hp = net.heads
    rc = L.lzm_search_conv(gt.h, S, 19652, 1.25, 0.997, p(mm), p(seeds), p(vtp), p(pool), p(net.native), p(net.actmap),
                           int(net.n_dres), int(net.n_pres), int(net.r_ch), int(net.h_ch), p(hp["w1t"]), p(hp["b1"]),
                           p(hp["w2q"]), p(hp["b2"]), int(hp["Kr"]), int(hp["Khd"]), int(hp["off_policy"]),
                           int(hp["Vr"]), int(hp["Vv"]), 1, None, None, None, None, None, _lib.stream_ptr())
    assert rc == _lib.LZM_ERR_STATE
    with pytest.raises(_lib.LzmError):
        gt.search_conv(net, S, mm, seeds, vtp, pool)
    # S above the reservation
    rc, msg = gumbel(gt.h, sims=S + 1)
    assert rc == _lib.LZM_ERR_CAPACITY and msg.startswith("lzm_search_conv_gumbel:"), (rc, msg)
    assert gt.search_conv_gumbel_plan(net, S + 1)["code"] == _lib.LZM_ERR_CAPACITY
    # S <= 0, m < 0, max_roots < 0
    for kw in (dict(sims=0), dict(considered=-1), dict(max_roots=-1)):
        rc, msg = gumbel(gt.h, **kw)
        assert rc == _lib.LZM_ERR_ARG and msg.startswith("lzm_search_conv_gumbel:"), (rc, msg)
    # collect-step mode: there is no Gumbel collect step
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    dist = torch.zeros((B, A), dtype=torch.int32, device=DEV)
    vals = torch.zeros(B, device=DEV)
    gt.set_step(count, 0, True, dist, vals, True, 0.01)
    rc, msg = gumbel(gt.h)
    assert rc == _lib.LZM_ERR_STATE and msg.startswith("lzm_search_conv_gumbel:"), (rc, msg)
    assert gt.search_conv_gumbel_plan(net, S)["code"] == _lib.LZM_ERR_STATE
    gt.set_step()
    # nothing ran: the min-max rows, the counter, the pool and the tree are as they were
    torch.cuda.synchronize()
    assert torch.equal(mm, sentinel) and int(count.item()) == 0 and not pool.any()
    after = snapshot()
    for k in before:
        assert np.array_equal(before[k].view(np.uint32) if before[k].dtype == np.float32 else before[k],
                              after[k].view(np.uint32) if after[k].dtype == np.float32 else after[k]), k
    assert int(mt.distributions().clamp(min=0).sum().item()) == 0
    mt.close()
    finish(r)


# ------------------------------------------------------------------------------------------- graph capture
def test_captured_search_replayed_on_reprepared_roots_equals_eager():
    """the search with to_play and latents on the device captures as launches only (the considered-visits row is in
    place after the eager pass); replayed on re-prepared roots it gives the eager bits"""
    B, A, S, m = 6, 4, 10, 4
    model = make_model("mz", 9, A=A)
    x = inputs(B, A, None, 1)
    eager = run(model, x, S, m, True)
    mcts, roots = eager["mcts"], eager["roots"]
    mcts.record = False
    vt = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    prepare(roots, x, True, [-1] * B)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        mcts.search(roots, model, x["lat0"], vt)  # (warm: the record-free path's buffers)
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert mcts.last_path == "fused-conv"
    prepare(roots, x, True, [-1] * B)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mcts.search(roots, model, x["lat0"], vt)
    assert mcts.last_path == "fused-conv"
    for _ in range(2):  # the second replay starts from roots prepared again, as a collect step's
        prepare(roots, x, True, [-1] * B)
        graph.replay()
        torch.cuda.synchronize()
        roots.tree.searched()
        out = tg.device_outputs(roots, eager["disc"], A, S)
        for k in ("dist", "traj"):
            assert np.array_equal(out[k], eager["out"][k]), k
        for k in ("values", "policies", "children"):
            assert tg.same_bits(out[k], eager["out"][k]), k
        assert tg.same_bits(roots._last_minmax[:, :2].cpu().numpy(), eager["mm"])
        assert torch.equal(mcts._buf.pool.view(torch.int32), eager["pool"].view(torch.int32))
    del graph
    finish(eager)
