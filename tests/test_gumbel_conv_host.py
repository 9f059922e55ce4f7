"""CPU: the one-launch Gumbel MuZero search of the conv MuZeroModel (lzm_search_conv_gumbel,
lzm_search_conv_gumbel_plan) as far as a host without a GPU can see it: the header's declarations, the library's
exports and the binding table agree argument by argument, a null handle is refused before anything else with the
entry point's name in front of the message and the plan's output words untouched, and the search class reads
cfg.fused_conv_search — a key of its own, not in the class's config — with the default off."""
import ctypes

import pytest

from lightzero_amd import _lib
from tests.test_gumbel_fused_host import declared_args

NAMES = ("lzm_search_conv_gumbel", "lzm_search_conv_gumbel_plan")


@pytest.mark.parametrize("name", NAMES)
def test_header_library_and_binding_table_agree(name):
    L = _lib.load()
    assert hasattr(L, name)
    assert _lib.SIGNATURES[name] == declared_args(name)
    assert getattr(L, name).restype is ctypes.c_int


def test_argument_lists_are_the_documented_ones():
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    # lzm_search_conv_sliced's list without pb_c_base, pb_c_init and seeds, with max_num_considered_actions after
    # num_simulations: (h, S, m, discount, minmax, vtp_in, latent_pool, <trunk and heads>, rec_*, max_roots, stream)
    sliced = list(_lib.SIGNATURES["lzm_search_conv_sliced"])
    assert sliced[:7] == [p, i, i, f, f, p, p]  # (h, S, pb_c_base, pb_c_init, discount, minmax, seeds)
    assert declared_args(NAMES[0]) == [p, i, i, f, p] + sliced[7:]
    # the shape arguments of lzm_search_conv_sliced_plan without (ez, H, horizon), then max_roots and out[11]
    plan = list(_lib.SIGNATURES["lzm_search_conv_sliced_plan"])
    assert declared_args(NAMES[1]) == plan[:2] + plan[5:] == [p] + [i] * 12 + [p]


def test_null_handle_is_refused_with_the_name_in_front():
    L = _lib.load()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_int32 * 11)(*([7] * 11))
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    L.lzm_set_reuse(None, None, None)  # a known message first: a refusal that sets none cannot pass on a stale one
    assert L.lzm_last_error().startswith(b"lzm_set_reuse:")
    assert L.lzm_search_conv_gumbel(None, 8, 4, 0.997, ptr, ptr, ptr, ptr, ptr, 1, 1, 2, 4, ptr, ptr, ptr, ptr, 128,
                                    256, 128, 21, 21, 1, None, None, None, None, None, 0, None) == _lib.LZM_ERR_ARG
    assert L.lzm_last_error().startswith(b"lzm_search_conv_gumbel:")
    L.lzm_set_reuse(None, None, None)
    assert L.lzm_search_conv_gumbel_plan(None, 8, 1, 1, 2, 4, 128, 256, 128, 21, 21, 1, 0, out) == _lib.LZM_ERR_ARG
    assert L.lzm_last_error().startswith(b"lzm_search_conv_gumbel_plan:")
    assert list(out) == [7] * 11  # nothing written


def test_fused_conv_search_is_a_key_of_its_own_and_opt_in():
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    cfg = GumbelMuZeroMCTSCtree.default_config()
    assert "fused_conv_search" not in cfg and "fused_conv_search" not in GumbelMuZeroMCTSCtree.config
    assert callable(getattr(GumbelMuZeroMCTSCtree, "_fused_conv"))

    class Tree:  # (what _native_conv_net reads before it looks at the model)
        ez = False

    cfg.update(num_simulations=4, max_num_considered_actions=2, discount_factor=0.997, device="cpu",
               model=dict(support_scale=10, categorical_distribution=True), fused_search=True)
    mcts = GumbelMuZeroMCTSCtree(cfg)
    # read with default off: cfg.fused_search (DeviceSearchStep(algo="gumbel") sets it) does not turn it on, and
    # nothing past the key is looked at — the model is never touched
    assert mcts._fused_conv(object(), Tree(), (64, 8, 8), 4) is None and mcts.last_plan is None
