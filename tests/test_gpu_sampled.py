"""GPU: the Sampled EfficientZero tree (lzm_sampled.h), the ezs_tree module and SampledEfficientZeroMCTSCtree.

The yardstick is the host restatement tests/sampled_oracle.py (pinned to the compiled reference's transcripts by
tests/test_sampled_oracle.py) under the device's Philox draws. Tree state, slots and discrete actions are compared
bit for bit; continuous actions to one float32 ulp (both sides round a double result to float). On the fused path
the restatement is fed the value prefix and value the kernel decoded (scalar heads: h^-1 only), so the support decode
inside sampled_decode_kernel — decode_heads, shared with every other family and pinned by their tests — is checked
here only through the driver test's bound against the host loop, with categorical heads.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sampled_oracle as so  # noqa: E402
import sampled_search_time as tool  # noqa: E402  (the stand-in network's set-up and the host loop it times)
from lightzero_amd import _lib  # noqa: E402

DEV = torch.device("cuda", 0)
PB_C, HORIZON, DISC = so.PB_C, so.HORIZON, so.DISC
INTS = ("req_x", "req_y", "req_slot", "req_vtp", "req_len", "out_dist")


bits = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)  # noqa: E731
dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)  # noqa: E731


def same_actions(got, want, continuous):
    got = np.asarray(got).reshape(np.shape(want))  # (discrete: equal; continuous: within one float32 ulp)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)) if continuous else 0
    return bool(np.all(np.abs(got.astype(np.float64) - want) <= ulp))


def run_kernels(g, fused):
    """fused: the decode launch with the next walk folded in over g's tables as scalar heads (returns what the kernel
    decoded); else the raw-list path, sampled_traverse + sampled_backprop per simulation"""
    from lightzero_amd.tree import DeviceTree, new_minmax, seed_tensor
    B, S, K, dim, cont = (int(v) for v in g["meta"][:5])
    t = DeviceTree(B, dim, S, fast_rng=True, device=DEV, sampled=K, continuous=bool(cont))
    vtp, f = dev(g["to_play"], np.int32), lambda k: dev(g[k], np.float32)
    t.sampled_prepare(f("root_vp"), f("root_policy"), vtp, seed_tensor(g["root_seed"], DEV))
    mm, vp, val, pol = new_minmax(B, so.VDM, DEV), f("resp_vp"), f("resp_value"), f("resp_policy")
    seeds = dev(np.asarray(g["seeds"], np.uint32).view(np.int32), np.int32)
    decoded = torch.zeros((S, B, 2), device=DEV)
    req, acts = torch.zeros((S, 5, B), dtype=torch.int32, device=DEV), []
    t.sampled_traverse(mm, seeds[0:1], vtp, *PB_C, DISC)
    for k in range(S):
        req[k] = torch.stack([t.x, t.y, t.action, t.vtp, t.search_len])
        acts.append(t.last_actions.clone())
        reset = (t.search_len % HORIZON == 0).int()
        if fused:
            walk = (seeds[k + 1:k + 2], vtp, *PB_C) if k + 1 < S else None
            t.sampled_decode_backprop(k + 1, DISC, mm, vp[k], val[k], False, pol[k], t.vtp, seeds[k:k + 1], HORIZON,
                                      walk=walk, out_decoded=decoded[k])
            assert torch.equal(t.is_reset, reset)
        else:
            t.sampled_backprop(k + 1, DISC, mm, vp[k], val[k], pol[k], t.vtp, reset, seeds[k:k + 1])
            if k + 1 < S:
                t.sampled_traverse(mm, seeds[k + 1:k + 2], vtp, *PB_C, DISC)
    out = {n: req[:, j].cpu().numpy() for j, n in enumerate(INTS[:5])}
    out.update(out_dist=t.distributions().cpu().numpy(), out_values=t.values().cpu().numpy(),
               traj=t.trajectories(S + 1).cpu().numpy(), req_action=torch.stack(acts).cpu().numpy(),
               root_actions=t.sampled_actions().cpu().numpy())
    t.close()
    return out, decoded.cpu().numpy()


# B: 1, a partly filled workgroup, sixteen workgroups; K: 1 (a path as deep as S), 2, 20, every lane; D: 1, 3 (the
# dropped Box-Muller half), 6; discrete: K = A, K < A, every lane; S: 1, 12 (LSTM horizon 5 crossed); 1 and 2 players
SHAPES = {
    "c_b1_k1_d1_deep": dict(B=1, S=12, K=1, dim=1, cont=True),
    "c_b5_k2_d3_2p": dict(B=5, S=12, K=2, dim=3, cont=True, players=2),
    "c_b64_k20_d6": dict(B=64, S=12, K=20, dim=6, cont=True),
    "c_b5_k64_d3": dict(B=5, S=12, K=64, dim=3, cont=True),
    "c_b5_k20_d3_s1": dict(B=5, S=1, K=20, dim=3, cont=True),
    "d_b5_a4_k4": dict(B=5, S=12, K=4, dim=4, cont=False),
    "d_b64_a18_k5_2p": dict(B=64, S=12, K=5, dim=18, cont=False, players=2),
    "d_b1_a64_k64": dict(B=1, S=12, K=64, dim=64, cont=False),
    "d_b5_a18_k5_s1": dict(B=5, S=1, K=5, dim=18, cont=False, players=2),
}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "raw"])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_match_restatement(shape, fused):
    c = SHAPES[shape]
    g = so.scripted(seed=sorted(SHAPES).index(shape), **c)
    got, decoded = run_kernels(g, fused)
    if fused:
        g = dict(g, resp_vp=decoded[..., 0], resp_value=decoded[..., 1])
    sampler = lambda k: so.philox_sampler(g["root_seed"] if k < 0 else g["seeds"][k], c["K"], c["cont"])
    want = so.replay(g, lambda k: so.philox_draws(g["seeds"][k]), sampler)
    for n in INTS:
        assert np.array_equal(got[n], want[n]), n
    assert np.array_equal(bits(got["out_values"]), bits(want["out_values"]))
    assert [[a for a in row if a >= 0] for row in got["traj"].tolist()] == want["traj"]
    assert same_actions(got["root_actions"], want["root_actions"], c["cont"])
    assert same_actions(got["req_action"], want["req_action"], c["cont"])
    assert got["req_len"].max() == (c["S"] if c["K"] == 1 else got["req_len"].max())


# ------------------------------------------------------------------------------------------- driver
B_DRV, S_DRV, K_DRV, D_DRV = 6, 12, 5, 3


def search(d, graph):
    """one search of the shared inputs through tools/sampled_search_time.py's driver set-up; eager ones are recorded"""
    d[graph] = d.get(graph) or tool.class_search(B_DRV, S_DRV, K_DRV, D_DRV, True, graph, d["inputs"], record=not graph)
    roots, mcts = d[graph](d["seeds"], 77)
    out = dict(out_dist=np.array(roots.get_distributions(), np.int32), out_values=np.array(roots.get_values(), np.float32),
               traj=roots.get_trajectories(), sampled=np.array(roots.get_sampled_actions(), np.float32), mcts=mcts)
    if mcts.record:
        r = mcts.last_record
        out.update({n: v.cpu().numpy() for n, v in (("req_x", r.x), ("req_slot", r.action), ("req_len", r.search_len),
                                                    ("req_action", r.last_actions))})
    return out


@pytest.fixture(scope="module")
def driver():
    d = dict(inputs=tool.setup(B_DRV, D_DRV, True), seeds=torch.arange(11, 11 + S_DRV, dtype=torch.int32, device=DEV))
    d["eager"] = search(d, False)
    return d


def test_graph_replay_equals_eager(driver):
    eager = driver["eager"]
    for _ in range(3):  # the capture's first replay, then replays of the cached graph
        got = search(driver, True)
        assert np.array_equal(got["out_dist"], eager["out_dist"]) and got["traj"] == eager["traj"]
        assert np.array_equal(bits(got["out_values"]), bits(eager["out_values"]))
        assert np.array_equal(bits(got["sampled"]), bits(eager["sampled"]))
    assert len(got["mcts"]._graphs) == 1


def test_sampled_actions_are_the_rows_the_model_was_fed(driver):
    e = driver["eager"]
    assert e["sampled"].shape == (B_DRV, K_DRV, D_DRV) and np.all(np.abs(e["sampled"]) <= 1)
    k, i = np.nonzero(e["req_len"] == 1)  # walks that stop at a root child: every root's first, at the least
    assert len(k) >= B_DRV and np.array_equal(bits(e["req_action"][k, i]), bits(e["sampled"][i, e["req_slot"][k, i]]))


def test_driver_against_host_loop_through_ezs_tree(driver):
    """the reference's per-simulation loop (mcts_ctree_sampled.py:133-232) through the list API, as
    tools/sampled_search_time.py drives it"""
    got = driver["eager"]
    roots, trace = tool.host_search(B_DRV, S_DRV, K_DRV, D_DRV, True, driver["inputs"])(driver["seeds"].cpu().numpy(), 77)
    for j, n in enumerate(("req_x", "req_len")):
        assert np.array_equal(got[n], np.array([t[j] for t in trace])), n
    assert np.array_equal(bits(got["req_action"]), bits(np.array([t[2] for t in trace], np.float32)))
    assert np.array_equal(got["out_dist"], np.array(roots.get_distributions()))
    # tests/test_gpu_numerics.py's bound of the generic path: rtol 1e-5, atol 1e-5 * support_scale
    vals = np.array(roots.get_values(), np.float32)
    print("root value distance", np.abs(got["out_values"].astype(np.float64) - vals).max())
    np.testing.assert_allclose(got["out_values"], vals, rtol=1e-5, atol=1e-5 * (tool.SUPPORT // 2))


def test_refusals():
    from lightzero_amd.tree import DeviceTree, new_minmax
    # K > 64, D > 32, K > A, A > 64, another family's flag
    for dim, K, cont, flags in ((3, 65, 1, 0), (33, 4, 1, 0), (4, 5, 0, 0), (65, 4, 0, 0), (3, 4, 1, _lib.LZM_TREE_EZ)):
        assert _lib.load().lzm_sampled_create(4, dim, K, cont, 8, flags, ctypes.byref(ctypes.c_void_p())) == _lib.LZM_ERR_ARG
    sm, ez = DeviceTree(4, 3, 8, device=DEV, sampled=5, continuous=True), DeviceTree(4, 5, 8, ez=True, fast_rng=True, device=DEV)
    mm, seed, vtp = new_minmax(4, 0.01, DEV), torch.zeros(1, dtype=torch.int32, device=DEV), -torch.ones(4, dtype=torch.int32, device=DEV)
    z, ez.last_actions = torch.zeros((4, 6), device=DEV), torch.zeros((4, 3), device=DEV)
    dec = (1, DISC, mm, z, z, False, z, vtp)
    for tree, call, args in (
            (sm, "traverse", (mm, seed, vtp)), (sm, "backprop", (1, DISC, mm, z, z, z, vtp)), (sm, "decode_backprop", dec),
            (sm, "gumbel_traverse", (8, 4, DISC, vtp)), (sm, "stochastic_traverse", (mm, seed, vtp)),
            (ez, "sampled_prepare", (z, z, vtp, seed)), (ez, "sampled_traverse", (mm, seed, vtp)),
            (ez, "sampled_backprop", (1, DISC, mm, z, z, z, vtp, vtp, seed)),
            (ez, "sampled_decode_backprop", dec + (seed, HORIZON)), (ez, "sampled_actions", ()),
            (sm, "sampled_backprop", (1, DISC, mm, z, z, z, vtp, vtp, seed)),  # (before any sampled traverse)
            (sm, "sampled_decode_backprop", dec + (seed, HORIZON))):
        with pytest.raises(_lib.LzmError, match=r"failed \(-4\)"):
            getattr(tree, call)(*args)
    with pytest.raises(_lib.LzmError, match=r"failed \(-4\)"):  # the fused entry point, wrong family
        ez.sampled_decode_backprop(*dec, seed, HORIZON, walk=(seed, vtp, *PB_C))
    sm.close(), ez.close()
