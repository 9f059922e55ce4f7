"""GPU: the Stochastic MuZero tree (lzm_stochastic.h), the stochastic_mz_tree module and StochasticMuZeroMCTSCtree.

The yardstick is the host restatement tests/stochastic_oracle.py (pinned to the compiled reference's transcripts
by tests/test_stochastic_oracle.py) under the device's Philox draws. Tree state is compared bit for bit.
"""
import copy
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stochastic_oracle as so  # noqa: E402
from oracle.oracle import load_transcript  # noqa: E402
from stochastic_model import TwoBranchNet  # noqa: E402
from lightzero_amd import _lib  # noqa: E402

DEV = torch.device("cuda", 0)
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "stochastic", "stmz_*.npz")))
REQ = ("req_x", "req_y", "req_a", "req_vtp", "req_len", "req_is_chance")
PB_C = (19652, 1.25)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def scripted(B, S, A, C, players=1, noise=False, legal=None, disc=0.997, net="rand", seed=0):
    """a transcript-shaped case with GENERAL chance rows (random logits: every outcome has a non-zero prior)"""
    rng = np.random.default_rng(100 + seed)
    draw = (lambda *s: np.zeros(s, np.float32)) if net == "zero" else (
        lambda *s: rng.normal(0.0, 1.0, size=s).astype(np.float32))
    legal = legal or [list(range(A))] * B
    g = dict(legal_lists=so.pad(legal, A), noises=rng.dirichlet([0.3] * A, size=B).astype(np.float32),
             to_play=np.array([1 + (i * 7) % 2 for i in range(B)] if players == 2 else [-1] * B, np.int32),
             root_logits=draw(B, A), root_reward=draw(B), resp_d_reward=draw(S, B), resp_d_value=draw(S, B),
             resp_d_logits=draw(S, B, A), resp_c_value=draw(S, B),
             resp_c_logits=rng.normal(0.0, 2.0, size=(S, B, C)).astype(np.float32),
             seeds=rng.integers(0, 2 ** 31, size=S), meta=np.array([B, S, A, C, int(noise)], np.int64),
             consts=np.array([*PB_C, np.float32(disc), 0.01, 0.25], np.float64))
    return g


RAGGED = [[2, 0, 1], [1], [0, 2], [2, 1], [0, 1, 2]]
A64 = [list(range(64)), [a for a in range(64) if a % 3], [63, 5]]
SHAPES = {
    "b5_a3_c5_ragged_noise": dict(B=5, S=20, A=3, C=5, noise=True, legal=RAGGED),
    "b4_a2_c64": dict(B=4, S=16, A=2, C=64),
    "b3_a64_c2_ragged": dict(B=3, S=16, A=64, C=2, legal=A64, noise=True),
    "b3_a1_c1_s64_deep": dict(B=3, S=64, A=1, C=1),
    "b5_a3_c5_2p": dict(B=5, S=20, A=3, C=5, players=2),
    "b70_a3_c5": dict(B=70, S=12, A=3, C=5),
    "b4_a3_c5_disc0": dict(B=4, S=16, A=3, C=5, disc=0.0),
    "b4_a3_c5_disc1": dict(B=4, S=16, A=3, C=5, disc=1.0),
    "b5_a3_c5_zero_net": dict(B=5, S=20, A=3, C=5, net="zero", legal=RAGGED),
}


def run_kernels(g):
    """the launches the search loop uses (stochastic_traverse, then stochastic_decode_backprop with the next walk
    folded in) over g's scripted heads as scalar-head outputs; returns the recorded arrays and what the kernel
    decoded"""
    from lightzero_amd.tree import DeviceTree, new_minmax
    B, S, A, C, noise = (int(v) for v in g["meta"][:5])
    disc, W = float(g["consts"][2]), max(A, C)
    lists = so.legal_lists(g)
    t = DeviceTree(B, A, S, fast_rng=True, device=DEV, chance=C)
    vtp = dev(g["to_play"], np.int32)
    t.prepare(dev(so.pad(lists, W), np.int32), dev([len(l) for l in lists], np.int32),
              dev(np.pad(g["noises"], ((0, 0), (0, W - A))), np.float32) if noise else None, 0.25 if noise else 0.0,
              dev(g["root_reward"], np.float32), dev(np.pad(g["root_logits"], ((0, 0), (0, W - A))), np.float32), vtp)
    mm = new_minmax(B, 0.01, DEV)
    f = lambda k: dev(g[k], np.float32)
    cv, cp, dr, dv, dp = f("resp_c_value"), f("resp_c_logits"), f("resp_d_reward"), f("resp_d_value"), f("resp_d_logits")
    seeds = dev(np.asarray(g["seeds"], np.uint32).view(np.int32), np.int32)
    lat_c, lat_d = torch.full((B, 4), 1.0, device=DEV), torch.full((B, 4), 2.0, device=DEV)
    pool = torch.zeros((S + 1, B, 4), device=DEV)
    decoded = torch.zeros((S, B, 2), device=DEV)
    req = torch.zeros((S, 6, B), dtype=torch.int32, device=DEV)
    t.stochastic_traverse(mm, seeds[0:1], vtp, *PB_C, disc)
    for k in range(S):
        req[k] = torch.stack([t.x, t.y, t.action, t.vtp, t.search_len, t.is_chance])
        walk = (seeds[k + 1:k + 2], vtp, *PB_C) if k + 1 < S else None
        t.stochastic_decode_backprop(k + 1, disc, mm, (cv[k], cp[k], lat_c), (dr[k], dv[k], dp[k], lat_d), False,
                                     t.vtp, pool[k + 1], 4, walk=walk, out_decoded=decoded[k])
    out = {n: req[:, j].cpu().numpy() for j, n in enumerate(REQ)}
    out.update(out_dist=t.distributions().cpu().numpy()[:, :A], out_values=t.values().cpu().numpy(),
               out_traj=t.trajectories(S + 1).cpu().numpy())
    # the pool slot holds the row of the set each root's leaf kind picked
    assert np.array_equal(pool[1:, :, 0].cpu().numpy(), np.where(out["req_is_chance"] == 1, 1.0, 2.0))
    t.close()
    return out, decoded.cpu().numpy()


def assert_same(got, want, names=REQ + ("out_dist", "out_traj")):
    for n in names:
        assert np.array_equal(got[n], want[n]), n
    assert np.array_equal(bits(got["out_values"]), bits(want["out_values"]))


def with_decoded(g, decoded):
    """g with the kernel's decoded (h^-1) reward / value in place of the raw scalars, for the restatement"""
    g = dict(g)
    g["resp_d_reward"], g["resp_d_value"], g["resp_c_value"] = decoded[..., 0], decoded[..., 1], decoded[..., 1]
    return g


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_match_restatement_bit_for_bit(shape):
    g = scripted(seed=sorted(SHAPES).index(shape), **SHAPES[shape])
    got, decoded = run_kernels(g)
    want = so.replay(with_decoded(g, decoded), lambda k: so.philox_draws(g["seeds"][k]))
    assert_same(got, want)
    assert set(np.unique(got["req_is_chance"])) == {0, 1} and np.array_equal(got["req_is_chance"], got["req_len"] & 1)
    if "deep" in shape:
        assert got["req_len"].max() == 64


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_module_api_against_reference_transcripts(path):
    """stochastic_mz_tree driven the reference's way (split by kind, two batch_backpropagate calls with leaf_idx
    lists) over a transcript's one-hot chance rows: equal to the restatement under Philox on everything, and to the
    transcript on everything no tie draw touches — all of it when the search has no tie"""
    from lightzero_amd.ctree import stochastic_mz_tree as st
    g = load_transcript(path)
    B, S, A, C, noise = (int(v) for v in g["meta"][:5])
    disc, legal, to_play = float(g["consts"][2]), so.legal_lists(g), g["to_play"].tolist()
    roots = st.Roots(B, legal, C)
    if noise:
        roots.prepare(0.25, [g["noises"][i, :len(legal[i])].tolist() for i in range(B)], g["root_reward"].tolist(),
                      g["root_logits"].tolist(), to_play)
    else:
        roots.prepare_no_noise(g["root_reward"].tolist(), g["root_logits"].tolist(), to_play)
    mms = st.MinMaxStatsList(B)
    mms.set_delta(0.01)
    got = {n: np.zeros((S, B), np.int32) for n in REQ}
    for k in range(S):
        res = st.ResultsWrapper(B)
        ch, x, y, a, vtp = st.batch_traverse(roots, *PB_C, disc, mms, res, list(to_play), seed=int(g["seeds"][k]))
        for n, v in zip(REQ, (x, y, a, vtp, res.get_search_len(), ch)):
            got[n][k] = np.asarray(v, np.int32)
        for kind, rew, val, lg in ((True, np.ones(B, np.float32), g["resp_c_value"][k], g["resp_c_logits"][k]),
                                   (False, g["resp_d_reward"][k], g["resp_d_value"][k], g["resp_d_logits"][k])):
            idx = [i for i in range(B) if ch[i] == kind]
            if idx:  # (a chance leaf's reward, here 1, is overwritten by 0)
                st.batch_backpropagate(k + 1, disc, rew[idx].tolist(), val[idx].tolist(), lg[idx].tolist(), mms, res,
                                       vtp, [kind] * B, idx)
    got.update(out_dist=so.pad(roots.get_distributions(), A), out_values=np.array(roots.get_values(), np.float32),
               out_traj=so.pad(roots.get_trajectories(), S + 1))
    assert_same(got, so.replay(g, lambda k: so.philox_draws(g["seeds"][k])))
    if g["tie_free"][0]:
        assert_same(got, g)
    for n in ("req_x", "req_y", "req_len", "req_is_chance", "req_vtp"):  # the first walk stops below the root
        assert np.array_equal(got[n][0], g[n][0]), n
    assert np.array_equal(got["req_y"], g["req_y"]) and (got["out_dist"].clip(0).sum(axis=1) == S).all()
    roots.clear()


# ------------------------------------------------------------------------------------------- driver
B_DRV, S_DRV, A_DRV, C_DRV, LATENT, SUPPORT = 6, 12, 4, 32, 16, 21


def make_cfg(graph=False):
    from lightzero_amd.utils import EasyDict
    return EasyDict(num_simulations=S_DRV, discount_factor=0.997, device="cuda", use_hip_graph=graph,
                    model=EasyDict(support_scale=SUPPORT // 2, categorical_distribution=True))


@pytest.fixture(scope="module")
def driver():
    """one eager recorded search, shared: model, inputs, record and outputs"""
    from lightzero_amd import StochasticMuZeroMCTSCtree
    torch.manual_seed(0)
    model = TwoBranchNet(LATENT, A_DRV, C_DRV, SUPPORT).to(DEV).eval()
    rng = np.random.default_rng(5)
    d = dict(model=model, lat=rng.normal(size=(B_DRV, LATENT)).astype(np.float32),
             logits=rng.normal(size=(B_DRV, A_DRV)).astype(np.float32), reward=[0.0] * B_DRV,
             legal=[list(range(A_DRV))] * (B_DRV - 1) + [[3, 1]],
             seeds=torch.arange(11, 11 + S_DRV, dtype=torch.int32, device=DEV))
    d["eager"] = run_driver(StochasticMuZeroMCTSCtree(make_cfg()), d, True)
    return d


def run_driver(mcts, d, record):
    mcts.record = record
    roots = mcts.roots(B_DRV, d["legal"], C_DRV)
    roots.prepare_no_noise(d["reward"], d["logits"].tolist(), [-1] * B_DRV)
    mcts.search(roots, d["model"], d["lat"], [-1] * B_DRV, seeds=d["seeds"])
    out = dict(out_dist=so.pad(roots.get_distributions(), A_DRV), out_values=np.array(roots.get_values(), np.float32),
               out_traj=so.pad(roots.get_trajectories(), S_DRV + 1), path=mcts.last_path)
    if record:
        r = mcts.last_record
        out.update(req_x=r.x, req_a=r.action, req_len=r.search_len, req_vtp=r.vtp, req_is_chance=r.is_chance)
        out.update({k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v)})
    roots.clear()
    return out


def decode(logits, dtype):
    """InverseScalarTransform in `dtype` (scaling_transform.py:118-128)"""
    p = torch.softmax(logits.to(dtype), dim=-1)
    v = (p * torch.arange(-(SUPPORT // 2), SUPPORT // 2 + 1, dtype=dtype, device=logits.device)).sum(-1)
    return torch.sign(v) * (((torch.sqrt(1 + 4 * 0.001 * (v.abs() + 1 + 0.001)) - 1) / (2 * 0.001)) ** 2 - 1)


def host_loop(d, tree_api=None, dtype=torch.float32):
    """The reference's architecture: split by leaf kind, two sub-batch model calls, two backups with leaf_idx lists.
    tree_api None: the restatement under Philox with the network evaluated in `dtype` on the host."""
    st, device = tree_api, DEV if tree_api else "cpu"
    model = d["model"] if tree_api else copy.deepcopy(d["model"]).to("cpu", dtype)
    seeds = d["seeds"].cpu().numpy().view(np.uint32)
    pool = [torch.as_tensor(d["lat"], dtype=dtype, device=device)]
    if st:
        roots = st.Roots(B_DRV, d["legal"], C_DRV)
        roots.prepare_no_noise(d["reward"], d["logits"].tolist(), [-1] * B_DRV)
        mms = st.MinMaxStatsList(B_DRV)
        mms.set_delta(0.01)
    else:
        roots = so.Tree(d["legal"])
        roots.prepare(0.0, None, d["reward"], d["logits"], [-1] * B_DRV)
        mms = [so.MinMax(0.01) for _ in range(B_DRV)]
    req = {n: [] for n in ("req_is_chance", "req_x", "req_a", "req_len")}
    for k in range(S_DRV):
        if st:
            res = st.ResultsWrapper(B_DRV)
            ch, x, y, a, vtp = st.batch_traverse(roots, *PB_C, 0.997, mms, res, [-1] * B_DRV, seed=int(seeds[k]))
            lens = res.get_search_len()
        else:
            o = roots.traverse(*PB_C, 0.997, mms, [-1] * B_DRV, *so.philox_draws(seeds[k]))
            ch, x, a, vtp, lens = o["is_chance"], o["x"], o["a"], o["vtp"], o["len"]
        for n, v in zip(req, (ch, x, a, lens)):
            req[n].append(np.asarray(v, np.int32))
        nxt = torch.zeros((B_DRV, LATENT), dtype=dtype, device=device)
        for kind in (True, False):
            idx = [i for i in range(B_DRV) if bool(ch[i]) == kind]
            if not idx:
                continue
            lat = torch.stack([pool[x[i]][i] for i in idx])
            with torch.no_grad():
                o = model.recurrent_inference(lat, torch.tensor([a[i] for i in idx], device=device), afterstate=not kind)
            nxt[idx] = o.latent_state
            rew, val = decode(o.reward, dtype).float().tolist(), decode(o.value, dtype).float().tolist()
            lg = o.policy_logits.float().tolist()
            if st:
                st.batch_backpropagate(k + 1, 0.997, rew, val, lg, mms, res, vtp, [kind] * B_DRV, idx)
            else:
                roots.backprop(k + 1, 0.997, rew, val, lg, mms, vtp, idx)
        pool.append(nxt)
    out = {n: np.stack(v) for n, v in req.items()}
    dist, vals = (roots.get_distributions(), roots.get_values()) if st else (roots.distributions(), roots.values())
    out.update(out_dist=so.pad(dist, A_DRV), out_values=np.asarray(vals, np.float32))
    return out


def test_driver_against_split_batch_host_loop_and_float64(driver):
    from lightzero_amd.ctree import stochastic_mz_tree
    got = driver["eager"]
    assert got["path"] == "generic"
    ref = host_loop(driver, stochastic_mz_tree)
    names = ("req_is_chance", "req_x", "req_a", "req_len", "out_dist")
    for n in names:
        assert np.array_equal(got[n], ref[n]), n
    f64 = host_loop(driver, None, torch.float64)
    for n in names:
        assert np.array_equal(got[n], f64[n]), n
    # tests/test_gpu_numerics.py's bound of the generic path against float64: rtol 1e-5, atol 1e-5 * support_scale
    for other in (ref, f64):
        d = np.abs(got["out_values"].astype(np.float64) - other["out_values"])
        print("root value distance", d.max())
        np.testing.assert_allclose(got["out_values"], other["out_values"], rtol=1e-5, atol=1e-5 * (SUPPORT // 2))


def test_graph_replay_equals_eager(driver):
    from lightzero_amd import StochasticMuZeroMCTSCtree
    eager, mcts = driver["eager"], StochasticMuZeroMCTSCtree(make_cfg(graph=True))
    for _ in range(3):  # the capture's first replay, then replays of the cached graph
        got = run_driver(mcts, driver, False)
        for n in ("out_dist", "out_traj"):
            assert np.array_equal(got[n], eager[n]), n
        assert np.array_equal(bits(got["out_values"]), bits(eager["out_values"]))
    assert len(mcts._graphs) == 1


def test_refusals():
    import ctypes
    from lightzero_amd.tree import DeviceTree, new_minmax
    L, h = _lib.load(), ctypes.c_void_p()
    for a, c in ((4, 0), (4, 65), (0, 4), (65, 4)):
        assert L.lzm_stochastic_create(4, a, c, 8, 0, ctypes.byref(h)) == _lib.LZM_ERR_ARG
    assert L.lzm_stochastic_create(4, 4, 4, 8, _lib.LZM_TREE_EZ, ctypes.byref(h)) == _lib.LZM_ERR_ARG
    assert L.lzm_create(4, 4, 8, _lib.LZM_TREE_STOCHASTIC, ctypes.byref(h)) == _lib.LZM_ERR_ARG
    st, mz = DeviceTree(4, 3, 8, device=DEV, chance=5), DeviceTree(4, 3, 8, fast_rng=True, device=DEV)
    assert L.lzm_flags(st.h) & _lib.LZM_TREE_STOCHASTIC and L.lzm_action_space(st.h) == 5 and L.lzm_chance_space(st.h) == 5
    mm, seed, vtp = new_minmax(4, 0.01, DEV), torch.zeros(1, dtype=torch.int32, device=DEV), -torch.ones(4, dtype=torch.int32, device=DEV)
    z = torch.zeros((4, 5), device=DEV)
    for wrong in (lambda: st.traverse(mm, seed, vtp), lambda: st.backprop(1, 0.997, mm, z, z, z, vtp),
                  lambda: st.decode_backprop(1, 0.997, mm, z, z, False, z, vtp),
                  lambda: st.gumbel_traverse(8, 4, 0.997, vtp), lambda: mz.stochastic_traverse(mm, seed, vtp),
                  lambda: mz.stochastic_backprop(1, 0.997, mm, z, z, z, vtp),
                  lambda: mz.stochastic_decode_backprop(1, 0.997, mm, (z, z, z), (z, z, z, z), False, vtp, z, 5),
                  lambda: st.stochastic_backprop(1, 0.997, mm, z, z, z, vtp)):  # (before any stochastic traverse)
        with pytest.raises(_lib.LzmError, match=r"failed \(-4\)"):
            wrong()
    st.close(), mz.close()
