"""GPU: the one-launch conv Gumbel search (cfg.fused_conv_search) under the collect step and the collector on
Breakout: DeviceSearchStep / DeviceCollector(algo="gumbel", fused_conv=True) against the same objects with
fused_conv=False (the default: the per-simulation loop captured in the step's graph, which
test_gpu_gumbel_collect.test_device_collector_gumbel_breakout pins). Same model weights, same seed: everything the
step leaves behind is compared by bits, so nothing here has a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench  # noqa: E402
import test_gpu_gumbel as tg  # noqa: E402

DEV = torch.device("cuda", 0)
STEP_KEYS = ("action", "improved_policy", "completed_q", "distributions", "values")


def collector(fused_conv, n=3, S=6, m=2, **kw):
    from lightzero_amd.collector import DeviceCollector
    args = dict(device=DEV, seed=3, graph=True, poll_every=3, episode_slots=4, max_episode_steps=5, env="breakout",
                algo="gumbel", max_num_considered_actions=m)
    args.update(kw)
    if fused_conv is not None:  # None: the keyword absent
        args["fused_conv"] = fused_conv
    return DeviceCollector(bench.build_conv_model(DEV, seed=3), n, S, **args)


def step_outputs(col):
    col.step()
    torch.cuda.synchronize()
    out = {k: col.search.out[k].cpu().numpy().copy() for k in STEP_KEYS}
    out["env_state"] = col.env.state.cpu().numpy().copy()
    return out


def assert_same_step(a, b, what):
    for k in a:
        if a[k].dtype == np.float32:
            assert tg.same_bits(a[k], b[k]), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def test_collect_step_fused_conv_equals_generic_and_follows_a_weight_change():
    """three envs, six simulations: two steps, then the same weight change in both models (picked up by
    refresh_weights before the captured graph replays: the packed trunk and heads are rewritten in place), then
    two more steps — the one-launch step equals the per-simulation one throughout"""
    cols = {f: collector(f) for f in (True, False)}
    assert cols[True].search.graph is not None and cols[False].search.graph is not None
    assert cols[True].search.mcts._cfg.fused_conv_search is True
    assert cols[False].search.mcts._cfg.fused_conv_search is False
    for k in range(2):
        outs = {f: step_outputs(c) for f, c in cols.items()}
        assert cols[True].search.mcts.last_path == "fused-conv"
        assert cols[False].search.mcts.last_path == "generic"
        assert_same_step(outs[True], outs[False], f"step {k}")
        assert (outs[True]["distributions"].sum(1) == 6).all()
    plan = cols[True].search.mcts.last_plan
    assert plan["supported"] and plan["workgroups"] == 3 and plan["slices"] == 1 and plan["lds_bytes"] <= 160 * 1024
    net = cols[True].search.mcts._folded.get(cols[True].search.model)
    packed = {"native": net.native, "w2q": net.heads["w2q"], "w1t": net.heads["w1t"]}
    old = {k: v.clone() for k, v in packed.items()}
    before = outs[True]
    for c in cols.values():
        with torch.no_grad():
            for p in c.search.model.parameters():
                p.mul_(1.01)
    for k in range(2, 4):
        outs = {f: step_outputs(c) for f, c in cols.items()}
        assert_same_step(outs[True], outs[False], f"step {k} (after the weight change)")
    assert cols[True].search.mcts.last_path == "fused-conv"
    net2 = cols[True].search.mcts._folded.get(cols[True].search.model)
    assert net2 is net
    for k, v in packed.items():  # the same tensors (the captured launches point at them), new contents
        now = net.native if k == "native" else net.heads[k]
        assert now.data_ptr() == v.data_ptr() and not torch.equal(now, old[k]), k
    assert not tg.same_bits(before["values"], outs[True]["values"])


def test_device_collector_fused_conv_episodes_equal_generic():
    """2 envs x 4 simulations, episodes of three steps: the collected episodes are the default path's"""
    got = {}
    for f in (True, None):
        col = collector(f, n=2, S=4, max_episode_steps=3)
        episodes, stats = col.collect(2)
        assert col.search.mcts.last_path == ("fused-conv" if f else "generic")
        got[f] = episodes
    assert len(got[True]) == len(got[None]) >= 2
    for a, b in zip(got[True], got[None]):
        assert set(a) == set(b)
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape, k
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y), k
        assert (a["visits"].sum(1) == 4).all() and len(a["action_segment"]) == 3
