"""GPU: the one-launch conv searches over root slices (cfg.sliced_search: lzm_search_conv_sliced /
lzm_search_conv_ez_sliced — one launch per slice of roots, enqueued one after another, for batches past what a
single launch takes).

Every case runs the same roots, model and seeds through the sliced search and the generic per-simulation path
and asserts array equality of every recorded request (latent index, action, search_len), decoded {reward,
value}, policy logits, (EZ) is_reset, visit counts, root values and trajectories; in glibc mode the oracle
replay bit for bit; the path taken and the slice fields of the plan. Small caps (sliced_search_max_roots) make
slices out of batches of 130 / 300 roots: roots >= 256 of the MuZero case look back over two 256-root chunks
that span three launches, the EfficientZero cases end in a slice of one row block with two live rows.

Mutants of the sliced launches these tests catch (each run once; none faults or hangs, the waits are bounded):
  * the epoch advanced by every slice: the later slices wait for the lower roots' flags of an epoch nobody
    publishes any more, the bounded waits give up — MuZero: check_errors raises (test_mz_slices_*);
    EfficientZero: the guard re-runs the generic path, last_path is not "fused (3 slices)" (test_ez_slices_*);
  * hand-off flags neither global nor cleared (tflags / pflags by the slice's own tile index): the second slice
    reads the first slice's words as published: every EfficientZero case fails (visit counts differ), Philox too;
  * a look-back that sums only the slice's own roots: the draws of every slice but the first differ from the
    reference's stream: every glibc case fails (visit counts and root values differ from the generic path);
  * step_count advanced per slice: the counter ends at 8, not 6 (test_step_glue_three_slices).
The first and third are also caught by tests/test_gpu_reanalyze_conv.py (both models), the second by its
EfficientZero case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_conv import (DEV, captured_search_equals_eager_generic, oracle_replay,  # noqa: E402
                                 run_search)
from tests.test_gpu_conv_shapes import assert_same_search, make_model, ragged_legal, search_kwargs  # noqa: E402


def mcts_for(kind, S, scale, sliced=True, max_roots=0, horizon=5, fused=True, **extra):
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree, MuZeroMCTSCtree
    from lightzero_amd.utils import EasyDict
    cfg = EasyDict(dict(num_simulations=S, discount_factor=0.997, device=DEV, lstm_horizon_len=horizon,
                        fused_search=fused, sliced_search=sliced, sliced_search_max_roots=max_roots,
                        model=dict(support_scale=scale, categorical_distribution=True), **extra))
    return (EfficientZeroMCTSCtree if kind == "ez" else MuZeroMCTSCtree)(cfg)


_MODELS = {}


def model_for(kind, H=128):
    key = (kind, H)
    if key not in _MODELS:
        _MODELS[key] = make_model(kind, 41, **(dict(H=H) if kind == "ez" else {}))
    return _MODELS[key]


def run(kind, B, S, model, sliced, max_roots=0, fused=True, seed=3, rng="glibc", horizon=5, mcts=None, **search):
    kw = search_kwargs(dict(search=search, B=B, seed=seed), model)
    m = mcts or mcts_for(kind, S, kw["scales"][0], sliced, max_roots, horizon, fused)
    res = run_search(kind, B, S, seed, model=model, mcts=m, rng=rng, horizon=horizon, direct=True, check=True,
                     fresh_tree=True, **kw)
    res["mcts"] = m
    return res


def slice_fields(plan):
    return plan["slices"], plan["slice_roots"], plan["last_slice_roots"]


def test_mz_slices_128_128_44():
    """MuZero, 300 roots in slices of 128, 128, 44 = the generic path = the single launch = the oracle"""
    B, S = 300, 8
    model = model_for("mz")
    a = run("mz", B, S, model, True, 128)
    b = run("mz", B, S, model, False, fused=False)
    one = run("mz", B, S, model, False)
    assert (a["path"], b["path"], one["path"]) == ("fused-conv (3 slices)", "generic", "fused-conv")
    assert a["plan"]["supported"] and slice_fields(a["plan"]) == (3, 128, 44) and a["plan"]["workgroups"] == 128
    # the head-weight copy in LDS is decided by the slice's roots (128: a CU each), not the batch's (300: no)
    print("pinned half-heads: sliced", a["plan"]["pinned"], "single launch", one["plan"]["pinned"])
    assert a["plan"]["pinned"] >= one["plan"]["pinned"] and "slices" not in one["plan"]
    assert_same_search("mz", a, b)
    assert_same_search("mz", a, one)
    assert a["rec"]["search_len"].max() >= 3
    oracle_replay("mz", a, B, S)


def test_ez_slices_64_64_2():
    """EfficientZero (H = 128), 130 roots in slices of 64, 64, 2 (the last: one row block with two live rows) =
    the generic path = the single launch (which fits at this shape) = the oracle"""
    B, S = 130, 8
    model = model_for("ez")
    a = run("ez", B, S, model, True, 64)
    b = run("ez", B, S, model, False, fused=False)
    one = run("ez", B, S, model, False)
    assert (a["path"], b["path"], one["path"]) == ("fused (3 slices)", "generic", "fused")
    assert a["plan"]["supported"] and slice_fields(a["plan"]) == (3, 64, 2)
    assert a["plan"]["workgroups"] == 64 and a["plan"]["lstm_tiles"] == 8
    assert one["plan"]["workgroups"] == 130 and one["plan"]["lstm_tiles"] == 24
    assert_same_search("ez", a, b)
    assert_same_search("ez", a, one)
    assert a["rec"]["search_len"].max() >= 3
    oracle_replay("ez", a, B, S)
    # without a cap the sliced plan is the single launch's own
    whole = run("ez", B, S, model, True, 0)
    assert whole["path"] == "fused" and slice_fields(whole["plan"]) == (1, 130, 130)
    assert {k: whole["plan"][k] for k in one["plan"] if k != "reason"} == \
        {k: v for k, v in one["plan"].items() if k != "reason"}
    assert_same_search("ez", whole, b)


def test_ez_refused_grid_runs_as_two_slices():
    """130 roots at LSTM width 1024 (384 workgroups: the grid the single launch refuses): with the key on, two
    slices of 128 and 2 roots; with the key off the generic path and a counted fallback, as before"""
    from lightzero_amd import _lib
    B, S = 130, 8
    model = model_for("ez", 1024)
    a = run("ez", B, S, model, True)
    off = run("ez", B, S, model, False)
    assert a["path"] == "fused (2 slices)" and slice_fields(a["plan"]) == (2, 128, 2), (a["path"], a["plan"])
    assert a["plan"]["supported"] and a["plan"]["workgroups"] == 256 and a["plan"]["lstm_tiles"] == 128
    assert a["mcts"].residency_fallbacks == 0 and a["mcts"].timeout_fallbacks == 0
    assert off["path"] == "generic (co-residency refused)" and off["mcts"].residency_fallbacks == 1
    assert off["plan"]["code"] == _lib.LZM_ERR_RESIDENCY and "slices" not in off["plan"]
    assert_same_search("ez", a, off)
    oracle_replay("ez", a, B, S)


@pytest.mark.parametrize("kind", ["mz", "ez"])
def test_two_players_ragged_legal_sets(kind):
    """two players (the first slice holds player 1 only, the others both) and ragged legal sets"""
    B, S = 130, 8
    model = model_for(kind)
    to_play = [1] * 64 + np.random.default_rng(5).integers(1, 3, size=B - 64).tolist()
    legal = ragged_legal(B, model.action_space_size, 7)
    a = run(kind, B, S, model, True, 64, to_play=to_play, legal=legal)
    b = run(kind, B, S, model, False, fused=False, to_play=to_play, legal=legal)
    assert a["path"] == ("fused (3 slices)" if kind == "ez" else "fused-conv (3 slices)") and b["path"] == "generic"
    assert_same_search(kind, a, b)
    oracle_replay(kind, a, B, S)


def test_one_player_slice_in_a_two_player_batch():
    """the players verdict (cnode.cpp:776-781: max to_play == -1 means one player) is over the whole batch: the
    first slices hold only -1 roots, the last one a root that plays 1"""
    B, S = 130, 8
    model = model_for("mz")
    to_play = [-1] * (B - 1) + [1]
    a = run("mz", B, S, model, True, 64, to_play=to_play)
    b = run("mz", B, S, model, False, fused=False, to_play=to_play)
    assert a["path"] == "fused-conv (3 slices)" and b["path"] == "generic"
    assert_same_search("mz", a, b)
    oracle_replay("mz", a, B, S)


def test_ez_horizon_3():
    B, S = 130, 8
    model = model_for("ez")
    a = run("ez", B, S, model, True, 64, horizon=3)
    b = run("ez", B, S, model, False, fused=False, horizon=3)
    assert a["path"] == "fused (3 slices)" and b["path"] == "generic"
    assert a["rec"]["is_reset"].any() and not a["rec"]["is_reset"].all()
    assert_same_search("ez", a, b)
    oracle_replay("ez", a, B, S)


@pytest.mark.parametrize("kind", ["mz", "ez"])
def test_philox(kind):
    B, S = 130, 8
    model = model_for(kind)
    a = run(kind, B, S, model, True, 64, rng="philox")
    b = run(kind, B, S, model, False, fused=False, rng="philox")
    assert a["path"] == ("fused (3 slices)" if kind == "ez" else "fused-conv (3 slices)") and b["path"] == "generic"
    assert_same_search(kind, a, b)


@pytest.mark.parametrize("kind", ["mz", "ez"])
def test_back_to_back_on_one_handle(kind):
    """two sliced searches, then an unsliced one, on the same tree handle (its look-back and hand-off words
    carry the earlier searches' epochs): each equals the generic path from the same roots and seeds"""
    from lightzero_amd.tree import DeviceTree, SequentialSeeds, set_seed_source
    B, S = 130, 8
    model = model_for(kind)
    A = model.action_space_size
    scale = search_kwargs(dict(search={}, B=B, seed=1), model)["scales"][0]
    cls = type(mcts_for(kind, S, scale))
    tree = DeviceTree(B, A, 64, ez=(kind == "ez"), device=DEV)
    rng = np.random.default_rng(9)
    try:
        for n, (sliced, cap, want) in enumerate([(True, 64, 3), (True, 64, 3), (False, 0, 1)]):
            lat0 = torch.from_numpy(np.maximum(rng.standard_normal((B, 64, 8, 8)), 0).astype(np.float32)).to(DEV)
            logits0 = rng.standard_normal((B, A)).astype(np.float32)
            hidden0 = tuple(torch.from_numpy((0.5 * rng.standard_normal((1, B, 128))).astype(np.float32)).to(DEV)
                            for _ in range(2))
            out = []
            for m, t in ((mcts_for(kind, S, scale, sliced, cap), tree), (mcts_for(kind, S, scale, fused=False), None)):
                roots = cls.roots(B, [list(range(A))] * B)
                if t is not None:
                    roots.tree = t
                roots.prepare_no_noise([0.0] * B, logits0.tolist(), [-1] * B)
                set_seed_source(SequentialSeeds(100 + n))
                try:
                    if kind == "ez":
                        m.search(roots, model, lat0, hidden0, [-1] * B)
                    else:
                        m.search(roots, model, lat0, [-1] * B)
                finally:
                    set_seed_source(None)
                rt = roots.tree
                out.append((m.last_path, rt.distributions().cpu().numpy(), rt.values().cpu().numpy(),
                            rt.trajectories(S + 2).cpu().numpy()))
                assert rt.check_errors() is not None
                if t is None:
                    roots.clear()
                else:
                    roots.tree = None  # (kept for the next search: not returned to the pool)
            name = "fused" if kind == "ez" else "fused-conv"
            assert out[0][0] == (name if want == 1 else f"{name} ({want} slices)") and out[1][0] == "generic", out[0][0]
            for x, y in zip(out[0][1:], out[1][1:]):
                assert np.array_equal(x, y), n
            assert (out[0][1].sum(axis=1) == S).all()
    finally:
        tree.close()


@pytest.mark.parametrize("kind", ["mz", "ez"])
def test_step_glue_three_slices(kind):
    """the collect step's glue in the kernel over three slices: the device counter advances once, and the dist /
    values outputs (so the seeds, which every slice derives from the counter) equal those of the same collect
    step run as one launch"""
    B, S = 130, 8
    model = model_for(kind)
    A = model.action_space_size
    scale = search_kwargs(dict(search={}, B=B, seed=1), model)["scales"][0]
    rng = np.random.default_rng(11)
    lat0 = torch.from_numpy(np.maximum(rng.standard_normal((B, 64, 8, 8)), 0).astype(np.float32)).to(DEV)
    logits0 = rng.standard_normal((B, A)).astype(np.float32)
    hidden0 = tuple(torch.from_numpy((0.5 * rng.standard_normal((1, B, 128))).astype(np.float32)).to(DEV)
                    for _ in range(2))
    tp = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    outs = []
    for sliced, want in ((True, 3), (False, 1), (False, 0)):  # (0: the generic path, the glue as launches around it)
        m = mcts_for(kind, S, scale, sliced, 64, fused=want > 0)
        roots = type(m).roots(B, [list(range(A))] * B)
        roots.prepare_no_noise([0.0] * B, logits0.tolist(), [-1] * B)
        count = torch.full((1,), 5, dtype=torch.int64, device=DEV)
        dist = torch.full((B, A), -7, dtype=torch.int32, device=DEV)
        values = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
        step = dict(count=count, base=17, dist=dist, values=values)
        if kind == "ez":
            m.search(roots, model, lat0, hidden0, tp, step=step)
        else:
            m.search(roots, model, lat0, tp, step=step)
        name = "fused" if kind == "ez" else "fused-conv"
        assert m.last_path == ("generic" if want == 0 else name if want == 1 else f"{name} ({want} slices)"), m.last_path
        assert int(count.item()) == 6
        assert torch.equal(dist, roots.tree.distributions()) and (dist.sum(dim=1) == S).all()
        assert torch.equal(values, roots.tree.values())
        assert roots.tree.check_errors() is not None
        outs.append((dist.cpu().numpy(), values.cpu().numpy()))
        roots.clear()
    for other in outs[1:]:
        assert np.array_equal(outs[0][0], other[0]) and np.array_equal(outs[0][1], other[1])


def test_sliced_ez_search_inside_a_callers_capture():
    """a sliced EfficientZero search (three launches) captured by the caller and replayed = the eager generic
    search"""
    B, S = 130, 8
    model = model_for("ez")
    kw = search_kwargs(dict(search={}, B=B, seed=3), model)
    mcts = mcts_for("ez", S, kw["scales"][0], True, 64)
    w = run_search("ez", B, S, 3, model=model, mcts=mcts, record=False, direct=True, **kw)  # buffers, packed network
    assert w["path"] == "fused (3 slices)"
    captured_search_equals_eager_generic(mcts, model, B, S, w["logits0"], w["lat0"], w["hidden0"])
    assert mcts.last_path == "fused (3 slices)" and mcts.residency_fallbacks == 0 and mcts.timeout_fallbacks == 0
