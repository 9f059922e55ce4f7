"""The Gumbel MuZero tree's pure-host pieces: the library's Gumbel table and considered-visits rows against the
recorded reference tables, the gmz_tree module's Cython-style type errors, the search class's config surface.
None of these touches a GPU."""
import ctypes
import os

import numpy as np
import pytest

from lightzero_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gumbel")


@pytest.fixture(scope="module")
def tables():
    return np.load(os.path.join(GOLDEN, "gmz_tables.npz"))


def test_gumbel_table_matches_reference_bits(tables):
    L = _lib.load()
    out = (ctypes.c_float * 64)()
    assert L.lzm_gumbel_table(10.0, 64, out) == _lib.LZM_OK
    assert np.array_equal(np.array(out, np.float32).view(np.uint32), tables["gumbel"].view(np.uint32))
    # a shorter table is a prefix (every root cuts the same table to its legal count, cnode.cpp:89)
    short = (ctypes.c_float * 5)()
    assert L.lzm_gumbel_table(10.0, 5, short) == _lib.LZM_OK
    assert np.array_equal(np.array(short, np.float32).view(np.uint32), tables["gumbel"][:5].view(np.uint32))
    assert L.lzm_gumbel_table(10.0, 4, None) == _lib.LZM_ERR_ARG


def test_considered_visits_rows(tables):
    L = _lib.load()
    ms = [tuple(int(v) for v in r) for r in tables["ms"]]
    assert any(m <= 1 for m, _ in ms) and any(m > S for m, S in ms)
    for m, S in ms:
        out = (ctypes.c_int32 * S)()
        assert L.lzm_gumbel_considered_visits(m, S, out) == _lib.LZM_OK
        assert list(out) == tables[f"row_{m}_{S}"].tolist(), (m, S)
    # a worked example: four considered actions over eight simulations
    out = (ctypes.c_int32 * 8)()
    L.lzm_gumbel_considered_visits(4, 8, out)
    assert list(out) == [0, 0, 0, 0, 1, 1, 2, 2]
    assert L.lzm_gumbel_considered_visits(4, 0, out) == _lib.LZM_ERR_ARG
    assert L.lzm_gumbel_considered_visits(-1, 8, out) == _lib.LZM_ERR_ARG
    assert L.lzm_gumbel_considered_visits(4, 8, None) == _lib.LZM_ERR_ARG


def test_considered_visits_every_row():
    """every reference row m in [0, 66] x S in {1..64, 100, 200}: m = 0, m no power of two, m > S"""
    full = np.load(os.path.join(GOLDEN, "gmz_visits_full.npz"))
    rows, index = full["rows"], full["index"]
    assert len(index) == 4422
    L = _lib.load()
    for m, S, off in index.tolist():
        out = (ctypes.c_int32 * S)()
        assert L.lzm_gumbel_considered_visits(m, S, out) == _lib.LZM_OK, (m, S)
        assert list(out) == rows[off:off + S].tolist(), (m, S)


def test_gmz_tree_surface_and_type_errors():
    from lightzero_amd.ctree import gmz_tree
    assert sorted(gmz_tree.__all__) == sorted(
        ["MinMaxStatsList", "ResultsWrapper", "Roots", "batch_traverse", "batch_back_propagate"])
    for name in ("prepare", "prepare_no_noise", "get_trajectories", "get_distributions", "get_children_values",
                 "get_policies", "get_values", "clear", "num"):
        assert hasattr(gmz_tree.Roots, name), name
    roots = gmz_tree.Roots(2, [[0, 1], [1]])
    assert roots.num == 2
    ok = dict(noises=[[0.5, 0.5], [1.0]], value_prefix_pool=[0.0, 0.0], value_pool=[0.1, 0.2],
              policy_logits_pool=[[0.0, 0.0], [0.0, 0.0]])
    for bad in ok:  # arguments typed `list` in gmz_tree.pyx:36-40
        kw = dict(ok, **{bad: tuple(ok[bad])})
        with pytest.raises(TypeError, match=f"Argument '{bad}' has incorrect type \\(expected list, got tuple\\)"):
            roots.prepare(0.25, kw["noises"], kw["value_prefix_pool"], kw["value_pool"], kw["policy_logits_pool"],
                          [-1, -1])
        if bad != "noises":
            with pytest.raises(TypeError, match=f"Argument '{bad}' has incorrect type"):
                roots.prepare_no_noise(kw["value_prefix_pool"], kw["value_pool"], kw["policy_logits_pool"], [-1, -1])
    res, mm = gmz_tree.ResultsWrapper(2), gmz_tree.MinMaxStatsList(2)
    with pytest.raises(TypeError, match="Argument 'virtual_to_play_batch' has incorrect type \\(expected list"):
        gmz_tree.batch_traverse(roots, 8, 4, 0.997, res, (-1, -1))
    with pytest.raises(TypeError, match="Argument 'roots' has incorrect type"):
        gmz_tree.batch_traverse(object(), 8, 4, 0.997, res, [-1, -1])
    with pytest.raises(TypeError, match="Argument 'results' has incorrect type"):
        gmz_tree.batch_traverse(roots, 8, 4, 0.997, object(), [-1, -1])
    with pytest.raises(TypeError, match="an integer is required"):
        gmz_tree.batch_traverse(roots, 8.5, 4, 0.997, res, [-1, -1])
    for pos, name in ((2, "value_prefixs"), (3, "values"), (4, "policies"), (7, "to_play_batch")):
        args = [1, 0.997, [0.0, 0.0], [0.0, 0.0], [[0.0, 0.0]] * 2, mm, res, [-1, -1]]
        args[pos] = tuple(args[pos])
        with pytest.raises(TypeError, match=f"Argument '{name}' has incorrect type \\(expected list"):
            gmz_tree.batch_back_propagate(*args)
    with pytest.raises(TypeError, match="Argument 'min_max_stats_lst' has incorrect type"):
        gmz_tree.batch_back_propagate(1, 0.997, [0.0, 0.0], [0.0, 0.0], [[0.0, 0.0]] * 2, object(), res, [-1, -1])
    assert res.get_search_len() == []


def test_search_class_surface():
    import lightzero_amd
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree, _MCTSCtree
    assert lightzero_amd.GumbelMuZeroMCTSCtree is GumbelMuZeroMCTSCtree
    assert issubclass(GumbelMuZeroMCTSCtree, _MCTSCtree)
    cfg = GumbelMuZeroMCTSCtree.default_config()
    # lzero/mcts/tree_search/mcts_ctree.py:969-978
    assert dict(cfg) == dict(num_simulations=50, root_dirichlet_alpha=0.3, root_noise_weight=0.25,
                             value_delta_max=0.01, cfg_type="GumbelMuZeroMCTSCtreeDict")
    assert not hasattr(GumbelMuZeroMCTSCtree, "search_with_reuse")
    assert hasattr(GumbelMuZeroMCTSCtree, "search") and hasattr(GumbelMuZeroMCTSCtree, "roots")


def test_package_does_not_import_the_restatement():
    pkg = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "lightzero_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "gumbel_oracle" not in open(os.path.join(root, f)).read(), f
