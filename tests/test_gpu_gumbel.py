"""GPU: the Gumbel MuZero tree (lzm_gumbel.h) and GumbelMuZeroMCTSCtree.

Everything is compared bit for bit (uint32 views of the floats): against the reference's recorded transcripts
tests/golden/gumbel/gmz_*.npz through the gmz_tree module API, and against the host restatement
(tests/gumbel_oracle.py, itself pinned to those transcripts by tests/test_gumbel_oracle.py) fed the network
outputs the search recorded.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gumbel_oracle as go  # noqa: E402
from lightzero_amd import _lib  # noqa: E402

DEV = torch.device("cuda", 0)
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(go.GOLDEN, "gmz_*.npz"))
               if not p.endswith(("gmz_tables.npz", "gmz_visits_full.npz")))
RAGGED = [[0, 1, 2, 3], [1, 3], [2]]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def device_outputs(roots, disc, A, S):
    t = roots.tree
    return dict(dist=t.distributions().cpu().numpy(), values=t.values().cpu().numpy(),
                traj=t.trajectories(S + 2).cpu().numpy(), policies=t.policies(disc).cpu().numpy(),
                children=t.children_values(disc).cpu().numpy())


def oracle_outputs(ot, disc, A, S):
    return dict(dist=go.pad(ot.distributions(), A), values=np.array(ot.values(), np.float32),
                traj=go.pad(ot.trajectories(), S + 2), policies=ot.policies(disc), children=ot.children_values(disc))


def assert_same_outputs(dv, orc):
    for k in ("dist", "traj"):
        assert np.array_equal(dv[k], orc[k]), k
    for k in ("values", "policies", "children"):
        assert same_bits(dv[k], orc[k]), k


# ------------------------------------------------------------------------------------------- transcripts
@pytest.mark.parametrize("name", CASES)
def test_module_api_replays_reference_transcript(name):
    from lightzero_amd.ctree import gmz_tree
    g = np.load(os.path.join(go.GOLDEN, name + ".npz"))
    B, S, A, m, noise = (int(v) for v in g["meta"])
    disc, nw = float(g["consts"][0]), float(g["consts"][1])
    legal = go.legal_lists(g)  # in the order the reference was given them: lane j is legal position j
    to_play = g["to_play"].tolist()
    roots = gmz_tree.Roots(B, legal)
    if noise:
        roots.prepare(nw, [g["noises"][i, :len(legal[i])].tolist() for i in range(B)], g["root_reward"].tolist(),
                      g["root_value"].tolist(), g["root_logits"].tolist(), to_play)
    else:
        roots.prepare_no_noise(g["root_reward"].tolist(), g["root_value"].tolist(), g["root_logits"].tolist(), to_play)
    mms = gmz_tree.MinMaxStatsList(B)
    mms.set_delta(0.01)
    for k in range(S):
        res = gmz_tree.ResultsWrapper(B)
        x, y, a, vtp = gmz_tree.batch_traverse(roots, S, m, disc, res, list(to_play))
        assert x == g["req_x"][k].tolist() and y == g["req_y"][k].tolist(), k
        assert a == g["req_a"][k].tolist() and vtp == g["req_vtp"][k].tolist(), k
        assert res.get_search_len() == g["req_len"][k].tolist(), k
        gmz_tree.batch_back_propagate(k + 1, disc, g["resp_reward"][k].tolist(), g["resp_value"][k].tolist(),
                                      g["resp_logits"][k].tolist(), mms, res, vtp)
    dist = roots.get_distributions()
    assert go.pad(dist, A).tolist() == g["out_dist"].tolist()
    tw = g["out_traj"].shape[1]
    assert np.array_equal(go.pad(roots.get_trajectories(), tw)[:, :tw], g["out_traj"])
    assert same_bits(roots.get_values(), g["out_values"])
    pol, cv = roots.get_policies(disc, A), roots.get_children_values(disc, A)
    assert all(isinstance(r, list) and len(r) == A for r in pol + cv)
    assert same_bits(pol, g["out_policies"])
    assert same_bits(cv, g["out_children_values"])
    # the min-max pair (the reference has no getter: the restatement, pinned to the same transcript, supplies it)
    ot, _ = go.replay(g)
    assert same_bits(mms._buf[:, :2].cpu().numpy(), np.array(ot.minmax, np.float32))
    # a wider action space only appends illegal actions
    wide = roots.get_policies(disc, A + 2)
    assert all(len(r) == A + 2 and r[A:] == [0.0, 0.0] for r in wide)
    roots.clear()


@pytest.mark.parametrize("name", CASES)
def test_decode_backprop_traverse_replays_transcripts(name):
    """the launch the search loop really uses (gumbel_decode_backprop_traverse; gumbel_decode_backprop for the last
    simulation) over every transcript's inputs: the scripted reward / value go in as scalar-head outputs, so the
    kernel decodes them (the inverse scalar transform) and the restatement is fed what the kernel decoded"""
    from lightzero_amd.tree import DeviceTree, new_minmax
    g = np.load(os.path.join(go.GOLDEN, name + ".npz"))
    B, S, A, m, noise = (int(v) for v in g["meta"])
    disc, nw = float(g["consts"][0]), float(g["consts"][1])
    lists = go.legal_lists(g)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    vtp = d(g["to_play"], np.int32)
    t = DeviceTree(B, A, S, gumbel=True, device=DEV)
    t.prepare(d(go.pad(lists, A), np.int32), d([len(l) for l in lists], np.int32),
              d(g["noises"], np.float32) if noise else None, nw if noise else 0.0, d(g["root_reward"], np.float32),
              d(g["root_logits"], np.float32), vtp)
    t.set_root_values(d(g["root_value"], np.float32))
    mm = new_minmax(B, 0.01, DEV)
    r, v = d(g["resp_reward"][..., None], np.float32), d(g["resp_value"][..., None], np.float32)
    p = d(g["resp_logits"], np.float32)
    decoded = torch.zeros((S, B, 2), dtype=torch.float32, device=DEV)
    req = torch.zeros((S, 5, B), dtype=torch.int32, device=DEV)
    t.gumbel_traverse(S, m, disc, vtp)
    for k in range(S):
        req[k] = torch.stack([t.x, t.y, t.action, t.vtp, t.search_len])
        args = (k + 1, disc, mm, r[k], v[k], False, p[k], t.vtp)
        if k + 1 < S:
            t.gumbel_decode_backprop_traverse(*args, S, m, vtp, out_decoded=decoded[k])
        else:
            t.gumbel_decode_backprop(*args, out_decoded=decoded[k])
    dec, req = decoded.cpu().numpy(), req.cpu().numpy()
    assert np.all(np.isfinite(dec))
    ot, want = go.replay(g, dict(resp_reward=dec[..., 0], resp_value=dec[..., 1], resp_logits=g["resp_logits"]))
    for j, key in enumerate(("x", "y", "a", "vtp", "len")):
        assert np.array_equal(req[:, j], want[key]), key
    dv = dict(dist=t.distributions().cpu().numpy(), values=t.values().cpu().numpy(),
              traj=t.trajectories(S + 2).cpu().numpy(), policies=t.policies(disc).cpu().numpy(),
              children=t.children_values(disc).cpu().numpy())
    mmv = mm[:, :2].cpu().numpy()
    t.close()
    assert_same_outputs(dv, oracle_outputs(ot, disc, A, S))
    assert same_bits(mmv, np.array(ot.minmax, np.float32))


# ------------------------------------------------------------------------------------------- the search
def sharpen_heads(model, k):
    """the weights and bias of the last linear layer of the policy, value and reward heads times k: at k = 30 the
    policy logits spread past 104 (expf underflows: priors that are exact zeros) and the categorical heads collapse
    onto single support bins (decoded values on a sparse, wide grid with many exact ties)"""
    with torch.no_grad():
        for head in (model.prediction_network.fc_policy_head, model.prediction_network.fc_value_head,
                     model.dynamics_network.fc_reward_head):
            last = [mod for mod in head.modules() if isinstance(mod, torch.nn.Linear)][-1]
            last.weight.mul_(k)
            last.bias.mul_(k)
    return model


def mlp_model(A, H=32, zero_heads=False, categorical=True, seed=0, support_scale=10, sharpen=None):
    from lightzero_amd.model_mlp import MuZeroModelMLP
    torch.manual_seed(seed)
    V = 2 * support_scale + 1
    m = MuZeroModelMLP(observation_shape=4, action_space_size=A, latent_state_dim=H,
                       categorical_distribution=categorical, reward_support_size=V, value_support_size=V,
                       last_linear_layer_init_zero=zero_heads, norm_type='BN')
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
    if sharpen is not None:
        sharpen_heads(m, sharpen)
    return m.to(DEV).eval()


def run_search(model, B, A, S, m, legal=None, noise=True, discount=0.997, categorical=True, graph=False, record=True,
               seed=0, support_scale=10, mcts=None, obs_shape=(4,), to_play=None):
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    rng = np.random.default_rng(100 + seed)
    obs = torch.from_numpy(rng.random(size=(B,) + tuple(obs_shape)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        out = model.initial_inference(obs)
    lat0 = out.latent_state
    logits0 = out.policy_logits.float().cpu().numpy()
    legal = [list(range(A))] * B if legal is None else [list(l) for l in legal]
    noises = np.zeros((B, A), np.float32)
    for i, l in enumerate(legal):
        noises[i, :len(l)] = rng.dirichlet([0.3] * len(l)).astype(np.float32)
    root_value = rng.normal(size=B).astype(np.float32)
    to_play = [-1] * B if to_play is None else to_play
    cfg = EasyDict(dict(num_simulations=S, max_num_considered_actions=m, discount_factor=discount, device=DEV,
                        use_hip_graph=graph, env_type='not_board_games',
                        model=dict(support_scale=support_scale, categorical_distribution=categorical)))
    mcts = GumbelMuZeroMCTSCtree(cfg) if mcts is None else mcts
    mcts.record = record
    roots = GumbelMuZeroMCTSCtree.roots(B, legal)
    if noise:
        roots.prepare(0.25, [noises[i, :len(l)].tolist() for i, l in enumerate(legal)], [0.0] * B, root_value.tolist(),
                      logits0.tolist(), to_play)
    else:
        roots.prepare_no_noise([0.0] * B, root_value.tolist(), logits0.tolist(), to_play)
    mcts.search(roots, model, lat0, to_play)
    assert mcts.last_path == "generic"
    disc = float(np.float32(discount))
    res = dict(out=device_outputs(roots, disc, A, S), roots=roots, mcts=mcts, legal=legal,
               noises=noises if noise else None, root_value=root_value, logits0=logits0, disc=disc, to_play=to_play,
               rec=None if mcts.last_record is None else mcts.last_record.numpy())
    return res


def assert_matches_restatement(r, A, S, m):
    """the restatement fed the recorded network outputs asks the same requests at every simulation and ends
    with the same five outputs"""
    rec, legal, B = r["rec"], r["legal"], len(r["legal"])
    ot = go.GumbelTree(legal, A)
    noises = None if r["noises"] is None else [r["noises"][i, :len(legal[i])] for i in range(B)]
    ot.prepare(0.25, noises, np.zeros(B, np.float32), r["root_value"], r["logits0"], r["to_play"])
    for k in range(S):
        x, y, a, vtp, ln = ot.traverse(S, m, r["disc"], r["to_play"])
        assert x == rec["x"][k].tolist(), ("x", k)
        assert a == rec["action"][k].tolist(), ("action", k)
        assert ln == rec["search_len"][k].tolist(), ("search_len", k)
        assert vtp == rec["vtp"][k].tolist(), ("vtp", k)
        ot.backprop(k + 1, r["disc"], rec["decoded"][k][:, 0], rec["decoded"][k][:, 1], rec["policy_logits"][k],
                    r["to_play"])
    assert_same_outputs(r["out"], oracle_outputs(ot, r["disc"], A, S))
    mm = r["roots"]._last_minmax[:, :2].cpu().numpy()
    assert same_bits(mm, np.array(ot.minmax, np.float32))


@pytest.mark.parametrize("B,A,S,m,kw", [
    (5, 2, 8, 4, {}),                               # a partial last workgroup (four roots per workgroup)
    (3, 4, 8, 4, dict(legal=RAGGED)),               # ragged: the legal[0] fallback at the two- and one-action roots
    (16, 18, 50, 16, {}),
    (2, 64, 33, 16, dict(H=64)),                    # the lane limit
    (7, 6, 1, 4, {}),                               # one simulation
    (4, 6, 12, 1, {}),                              # m = 1
    (4, 3, 5, 16, {}),                              # m > S and m > A
    (4, 4, 8, 4, dict(categorical=False)),          # scalar heads
    (4, 4, 8, 4, dict(discount=1.0)),
    (4, 4, 8, 4, dict(noise=False)),
    (130, 2, 8, 2, {}),                             # more than one workgroup and a partial last one
    (4, 4, 8, 4, dict(to_play=[1, 2, 2, 1])),       # to_play passes through: no sign flip
])
def test_search_matches_restatement(B, A, S, m, kw):
    kw = dict(kw)
    model = mlp_model(A, H=kw.pop("H", 32), categorical=kw.get("categorical", True), seed=B + A)
    r = run_search(model, B, A, S, m, seed=B + S, **kw)
    assert_matches_restatement(r, A, S, m)
    r["roots"].clear()


def test_ragged_case_reaches_the_fallback():
    """(3, 4, 8, 4) with RAGGED: table[4] for S = 8 is 0,0,0,0,1,1,2,2, so the two-legal root finds no child with
    visit count 0 at simulations 2 and 3 and takes legal[0]; the one-action root always has one choice."""
    model = mlp_model(4, seed=7)
    r = run_search(model, 3, 4, 8, 4, legal=RAGGED, seed=11)
    dist = r["out"]["dist"]
    assert dist[1, :2].sum() == 8 and dist[2, 0] == 8 and dist[0].sum() == 8
    assert_matches_restatement(r, 4, 8, 4)
    r["roots"].clear()


def test_zeroed_heads_all_ties():
    """the heads' last layers zeroed: every logit equal, every reward and value 0, every tie to the first legal
    action"""
    model = mlp_model(5, zero_heads=True, seed=3)
    r = run_search(model, 6, 5, 12, 4, legal=[[0, 1, 2, 3, 4], [2, 4], [1, 2, 3], [3], [0, 4], [0, 1, 2, 3, 4]], seed=5)
    assert np.all(r["rec"]["policy_logits"] == r["rec"]["policy_logits"][..., :1])
    assert_matches_restatement(r, 5, 12, 4)
    r["roots"].clear()


def test_eager_graph_and_replay_identical():
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    B, A, S, m = 9, 6, 10, 4
    model = mlp_model(A, seed=21)
    eager = run_search(model, B, A, S, m, seed=2, record=False)
    first = run_search(model, B, A, S, m, seed=2, record=False, graph=True)
    assert isinstance(first["mcts"], GumbelMuZeroMCTSCtree) and len(first["mcts"]._graphs) == 1
    # the same roots object prepared again, so the same tree: the second search replays the captured graph
    roots, mcts = first["roots"], first["mcts"]
    legal, rv, lg = first["legal"], first["root_value"], first["logits0"]
    roots.prepare(0.25, [first["noises"][i, :len(l)].tolist() for i, l in enumerate(legal)], [0.0] * B, rv.tolist(),
                  lg.tolist(), [-1] * B)
    rng = np.random.default_rng(102)
    obs = torch.from_numpy(rng.random(size=(B, 4)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        lat0 = model.initial_inference(obs).latent_state
    mcts.search(roots, model, lat0, [-1] * B)
    assert len(mcts._graphs) == 1
    second = device_outputs(roots, first["disc"], A, S)
    for other in (first["out"], second):
        assert_same_outputs(other, eager["out"])
    for r in (eager, first):
        r["roots"].clear()


def test_fused_launch_equals_backprop_then_traverse():
    from lightzero_amd.tree import DeviceTree, new_minmax
    B, A, S, m = 6, 5, 9, 4
    rng = np.random.default_rng(9)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    legal = np.tile(np.arange(A, dtype=np.int32), (B, 1))
    vtp = d(np.full(B, -1, np.int32), np.int32)
    trees, mms, reqs = [], [], [[], []]
    logits0 = rng.normal(size=(B, A)).astype(np.float32)
    values0 = rng.normal(size=B).astype(np.float32)
    for _ in range(2):
        t = DeviceTree(B, A, S, gumbel=True, device=DEV)
        t.prepare(d(legal, np.int32), d(np.full(B, A, np.int32), np.int32), None, 0.0, d(np.zeros(B), np.float32),
                  d(logits0, np.float32), vtp)
        t.set_root_values(d(values0, np.float32))
        trees.append(t)
        mms.append(new_minmax(B, 0.01, DEV))
    r = rng.normal(size=(S, B, 1)).astype(np.float32)
    v = rng.normal(size=(S, B, 1)).astype(np.float32)
    p = rng.normal(size=(S, B, A)).astype(np.float32)
    for j, t in enumerate(trees):
        t.gumbel_traverse(S, m, 0.997, vtp)
        for k in range(S):
            reqs[j].append(torch.stack([t.x, t.action, t.search_len]).cpu().numpy())
            args = (k + 1, 0.997, mms[j], d(r[k], np.float32), d(v[k], np.float32), False, d(p[k], np.float32), t.vtp)
            if j == 0:
                t.gumbel_decode_backprop(*args)
                if k + 1 < S:
                    t.gumbel_traverse(S, m, 0.997, vtp)
            elif k + 1 < S:
                t.gumbel_decode_backprop_traverse(*args, S, m, vtp)
            else:
                t.gumbel_decode_backprop(*args)
    assert np.array_equal(np.stack(reqs[0]), np.stack(reqs[1]))
    assert same_bits(mms[0].cpu().numpy(), mms[1].cpu().numpy())
    outs = []
    for t in trees:
        outs.append(dict(dist=t.distributions().cpu().numpy(), values=t.values().cpu().numpy(),
                         traj=t.trajectories(S + 2).cpu().numpy(), policies=t.policies(0.997).cpu().numpy(),
                         children=t.children_values(0.997).cpu().numpy()))
        t.close()
    assert_same_outputs(outs[0], outs[1])


def test_conv_model_native_trunk():
    from lightzero_amd.model_conv import atari_muzero_model
    torch.manual_seed(0)
    model = atari_muzero_model(last_linear_layer_init_zero=False).to(DEV).eval()
    A, B, S, m = model.action_space_size, 3, 6, 4
    r = run_search(model, B, A, S, m, seed=4, support_scale=300, obs_shape=(4, 64, 64))
    assert tuple(r["mcts"]._buf.pool.shape[2:]) == (64, 8, 8)
    assert r["mcts"]._folded.get(model).native is not None  # the step ran lzm_conv_trunk on the latent pool
    assert_matches_restatement(r, A, S, m)
    r["roots"].clear()


# ------------------------------------------------------------------------------------------- device logf
def host_logf(x):
    out = np.empty(x.shape, np.float32)
    f = go._libm.logf
    for i, v in enumerate(x.tolist()):
        out[i] = f(v)
    return out


def test_device_logf_equals_host_libm():
    """[1, 64]: a stride over every float there plus every power of two and its neighbours; beyond it the
    classes lzm_numerics.h claims: (0, 1), large values, subnormals, +-0, +-inf, NaN, negatives"""
    lo, hi = np.float32(1).view(np.uint32), np.float32(64).view(np.uint32)
    u = [np.arange(lo, hi + 1, 61, dtype=np.uint32)]
    for e in range(0, 7):
        c = np.float32(2.0 ** e).view(np.uint32)
        u.append(np.arange(max(int(c) - 4, int(lo)), min(int(c) + 5, int(hi) + 1), dtype=np.uint32))
    u.append(np.arange(0x00800000, 0x7f800000, 104729, dtype=np.uint32))  # positive normals
    u.append(np.arange(1, 0x00800000, 52361, dtype=np.uint32))           # subnormals
    u.append(np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xbf800000, 0x80000001, 0x3f7fffff,
                       0x3f800001], np.uint32))
    x = np.concatenate(u).view(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.empty_like(xd)
    _lib.call("lzm_debug_logf", _lib.ptr(xd), _lib.ptr(out), x.size, _lib.stream_ptr())
    got, want = out.cpu().numpy(), host_logf(x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    # expf(-inf) = +0: the policy output's exact zeros depend on it
    e = torch.empty(1, device=DEV)
    _lib.call("lzm_debug_expf", _lib.ptr(torch.tensor([-np.inf], device=DEV)), _lib.ptr(e), 1, _lib.stream_ptr())
    assert e.cpu().numpy().view(np.uint32)[0] == 0


# ------------------------------------------------------------------------------------------- wrong kind
def test_wrong_kind_calls_are_refused_before_any_launch():
    from lightzero_amd.tree import DeviceTree, new_minmax, seed_tensor
    B, A = 4, 3
    gt = DeviceTree(B, A, 8, gumbel=True, device=DEV)
    mt = DeviceTree(B, A, 8, device=DEV)
    mm = new_minmax(B, 0.01, DEV)
    vtp = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    f = torch.zeros((B, A), device=DEV)
    L = _lib.load()
    sp = _lib.stream_ptr()
    i32 = [_lib.ptr(t) for t in (gt.x, gt.y, gt.action)]
    # Gumbel entry points on a MuZero handle
    assert L.lzm_gumbel_traverse(mt.h, 8, 4, 0.997, _lib.ptr(vtp), *i32, None, _lib.ptr(gt.vtp),
                                 _lib.ptr(gt.search_len), sp) == _lib.LZM_ERR_STATE
    assert L.lzm_gumbel_get_policies(mt.h, 0.997, _lib.ptr(f), sp) == _lib.LZM_ERR_STATE
    assert L.lzm_gumbel_get_children_values(mt.h, 0.997, _lib.ptr(f), sp) == _lib.LZM_ERR_STATE
    assert L.lzm_gumbel_backprop(mt.h, 1, 0.997, _lib.ptr(mm), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(vtp),
                                 sp) == _lib.LZM_ERR_STATE
    for call_ in (lambda: mt.gumbel_traverse(8, 4, 0.997, vtp), lambda: mt.policies(0.997),
                  lambda: mt.gumbel_decode_backprop(1, 0.997, mm, f, f, False, f, vtp),
                  lambda: mt.gumbel_decode_backprop_traverse(1, 0.997, mm, f, f, False, f, vtp, 8, 4, vtp),
                  lambda: mt.set_root_values(f)):
        with pytest.raises(_lib.LzmError):
            call_()
    # MuZero entry points on a Gumbel handle
    assert L.lzm_traverse(gt.h, 19652, 1.25, 0.997, _lib.ptr(mm), _lib.ptr(seed_tensor(1, DEV)), _lib.ptr(vtp), *i32,
                          None, _lib.ptr(gt.vtp), _lib.ptr(gt.search_len), sp) == _lib.LZM_ERR_STATE
    for call_ in (lambda: gt.traverse(mm, seed_tensor(1, DEV), vtp),
                  lambda: gt.backprop(1, 0.997, mm, f, f, f, vtp),
                  lambda: gt.decode_backprop(1, 0.997, mm, f, f, False, f, vtp),
                  lambda: gt.decode_backprop_traverse(1, 0.997, mm, f, f, False, f, vtp, seed_tensor(1, DEV), vtp)):
        with pytest.raises(_lib.LzmError):
            call_()
    # out-of-range arguments are refused on the host
    with pytest.raises(ValueError):
        gt.gumbel_traverse(0, 4, 0.997, vtp)
    with pytest.raises(ValueError):
        gt.gumbel_traverse(8, -1, 0.997, vtp)
    with pytest.raises(_lib.LzmError):
        gt.gumbel_backprop(100, 0.997, mm, f, f, f, vtp)  # beyond the reserved capacity
    with pytest.raises(ValueError):
        DeviceTree(B, A, 8, gumbel=True, ez=True, device=DEV)
    # mixed kinds do not copy
    with pytest.raises(ValueError):
        gt.copy_roots_from(mt)
    torch.cuda.synchronize()
    gt.close()
    mt.close()
