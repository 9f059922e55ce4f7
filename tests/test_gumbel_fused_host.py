"""CPU: the one-launch Gumbel MuZero search's two entry points (lzm_search_mlp_gumbel, lzm_search_mlp_gumbel_plan)
as far as a host without a GPU can see them: the header's declarations, the library's exports and the binding
table agree argument by argument, a null handle is refused before anything else with the entry point's name in
front of the message, and the search class reads cfg.fused_search with the default off."""
import ctypes
import os
import re

import pytest

from lightzero_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lzmcts.h")
NAMES = ("lzm_search_mlp_gumbel", "lzm_search_mlp_gumbel_plan")
CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float}


def declared_args(name):
    """the ctypes argument list the header's declaration of `name` implies (pointers are void pointers)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        out.append(ctypes.c_void_p if "*" in arg else CTYPE[arg.replace("const ", "").split(" ")[0]])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_header_library_and_binding_table_agree(name):
    L = _lib.load()
    assert hasattr(L, name)
    assert _lib.SIGNATURES[name] == declared_args(name)
    assert getattr(L, name).restype is ctypes.c_int


def test_argument_lists_are_the_documented_ones():
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    # (h, hidden, head_hidden, support, res_dynamics, weights, S, m, discount, minmax, vtp_in, latent_pool,
    #  rec_x, rec_a, rec_len, rec_decoded, rec_logits, stream)
    assert declared_args(NAMES[0]) == [p, i, i, i, i, p, i, i, f, p, p, p, p, p, p, p, p, p]
    # the four plan words of lzm_search_mlp_plan, the same argument list
    assert declared_args(NAMES[1]) == _lib.SIGNATURES["lzm_search_mlp_plan"] == [p, i, i, i, i, i, p]


def test_null_handle_is_refused_with_the_name_in_front():
    L = _lib.load()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    L.lzm_set_reuse(None, None, None)  # a known message first: a refusal that sets none cannot pass on a stale one
    assert L.lzm_last_error().startswith(b"lzm_set_reuse:")
    assert L.lzm_search_mlp_gumbel(None, 32, 32, 21, 0, ptr, 8, 4, 0.997, ptr, ptr, ptr, None, None, None, None, None,
                                   None) == _lib.LZM_ERR_ARG
    assert L.lzm_last_error().startswith(b"lzm_search_mlp_gumbel:")
    L.lzm_set_reuse(None, None, None)
    assert L.lzm_search_mlp_gumbel_plan(None, 8, 32, 32, 21, 0, out) == _lib.LZM_ERR_ARG
    assert L.lzm_last_error().startswith(b"lzm_search_mlp_gumbel_plan:")
    assert list(out) == [7, 7, 7, 7]  # nothing written


def test_fused_search_is_opt_in():
    from lightzero_amd.mcts_ctree import GumbelMuZeroMCTSCtree
    cfg = GumbelMuZeroMCTSCtree.default_config()
    assert not cfg.get("fused_search", False)
    assert callable(getattr(GumbelMuZeroMCTSCtree, "_fused"))
