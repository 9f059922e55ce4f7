"""GPU: the refusals of the generic search path's entry points (lzm_traverse, lzm_backprop, lzm_decode_backprop,
lzm_decode_backprop_traverse and the lzm_gumbel_* entry points), through the C ABI itself so that both the
return code and lzm_last_error() are pinned.

Every case starts from a call whose arguments are all acceptable and breaks exactly one condition, so no case
depends on the order of the checks. Nothing here launches a search: every call is refused before its kernel.
A refusal's message starts with the public entry point's name, with one exception that is part of the
contract as it stands: the capacity check (cur = 0, or cur beyond the reserved simulations) reports
"latent index <cur> outside reserved capacity ..." whichever entry point ran it.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from lightzero_amd import _lib  # noqa: E402
from lightzero_amd._lib import (LZM_ERR_ARG, LZM_ERR_CAPACITY, LZM_ERR_STATE, LZM_OK, LZM_RNG_FAST,  # noqa: E402
                                LZM_TREE_GUMBEL)

DEV = torch.device("cuda", 0)
B, A, SIMS, V = 2, 2, 4, 5  # node capacity 1 + A * (SIMS + 1) = 11: cur = 5 needs 13


def _i32(n):
    return torch.zeros(n, dtype=torch.int32, device=DEV)


def _f32(n):
    return torch.zeros(n, dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def bufs():
    """one set of device buffers for every case (never written: every call is refused)"""
    names_i = ["seed", "vtp_in", "out_x", "out_y", "out_a", "out_vtp", "out_len", "to_play", "reuse_action"]
    d = {k: _i32(B) for k in names_i}
    d.update(minmax=_f32(4 * B), rewards=_f32(B), values=_f32(B), logits=_f32(B * A), reward_logits=_f32(B * V),
             value_logits=_f32(B * V), policy_logits=_f32(B * A), reuse_value=_f32(B), out=_f32(B * A))
    return d


@pytest.fixture
def make():
    """make(flags) -> a tiny handle, destroyed after the test"""
    L = _lib.load()
    made = []

    def _make(flags=0):
        h = ctypes.c_void_p()
        assert L.lzm_create(B, A, SIMS, flags, ctypes.byref(h)) == LZM_OK
        made.append(h)
        return h
    yield _make
    for h in made:
        L.lzm_destroy(h)


_WALK = ["vtp_in", "out_x", "out_y", "out_a", "out_a64", "out_vtp", "out_len"]
_DECODE = ["cur", "discount", "minmax", "reward_logits", "value_logits", "support_len", "categorical",
           "policy_logits", "to_play"]
_FILING = ["next_latent", "pool_slot", "row_elems", "out_decoded"]
# argument names in ABI order (include/lzmcts.h), after the handle and before the stream
ARGS = {
    "lzm_traverse": ["pb_c_base", "pb_c_init", "discount", "minmax", "seed"] + _WALK,
    "lzm_backprop": ["cur", "discount", "minmax", "rewards", "values", "logits", "to_play", "is_reset"],
    "lzm_decode_backprop": _DECODE + ["lstm_horizon", "out_is_reset"] + _FILING,
    "lzm_decode_backprop_traverse": _DECODE + ["lstm_horizon", "out_is_reset"] + _FILING +
                                    ["pb_c_base", "pb_c_init", "seed"] + _WALK,
    "lzm_gumbel_traverse": ["num_simulations", "max_considered", "discount"] + _WALK,
    "lzm_gumbel_backprop": ["cur", "discount", "minmax", "rewards", "values", "logits", "to_play"],
    "lzm_gumbel_decode_backprop": _DECODE + _FILING,
    "lzm_gumbel_decode_backprop_traverse": _DECODE + _FILING + ["num_simulations", "max_considered"] + _WALK,
    "lzm_gumbel_get_children_values": ["discount", "out"],
    "lzm_gumbel_get_policies": ["discount", "out"],
    "lzm_gumbel_set_root_values": ["values"],
}
SCALARS = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, cur=1, support_len=V, categorical=1, lstm_horizon=0,
               row_elems=0, num_simulations=SIMS, max_considered=2)
OPTIONAL = {"out_a64", "is_reset", "out_is_reset", "next_latent", "pool_slot", "out_decoded"}  # null is accepted
PLAIN = ["lzm_traverse", "lzm_backprop", "lzm_decode_backprop", "lzm_decode_backprop_traverse"]
GUMBEL = ["lzm_gumbel_traverse", "lzm_gumbel_backprop", "lzm_gumbel_decode_backprop",
          "lzm_gumbel_decode_backprop_traverse"]
GUMBEL_ALL = GUMBEL + ["lzm_gumbel_get_children_values", "lzm_gumbel_get_policies", "lzm_gumbel_set_root_values"]
DECODES = ["lzm_decode_backprop", "lzm_decode_backprop_traverse", "lzm_gumbel_decode_backprop",
           "lzm_gumbel_decode_backprop_traverse"]
TRAVERSES = ["lzm_traverse", "lzm_decode_backprop_traverse"]
WITH_CUR = ["lzm_backprop", "lzm_gumbel_backprop"] + DECODES


def _flags(name):
    return LZM_TREE_GUMBEL if name.startswith("lzm_gumbel_") else 0


def _required(name):
    return [a for a in ARGS[name] if a not in SCALARS and a not in OPTIONAL]


def refused(name, h, bufs, **override):
    """calls `name` on handle h with acceptable arguments except `override`; returns (code, message)"""
    L = _lib.load()
    L.lzm_set_reuse(None, None, None)  # a known message first: a refusal that sets none cannot pass on a stale one
    assert L.lzm_last_error().startswith(b"lzm_set_reuse:")
    vals = []
    for a in ARGS[name]:
        if a in override:
            v = override[a]
        elif a in SCALARS:
            v = SCALARS[a]
        elif a in OPTIONAL:
            v = None
        else:
            v = bufs[a]
        vals.append(ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v)
    rc = getattr(L, name)(h, *vals, None)
    return rc, L.lzm_last_error().decode()


def assert_refused(got, code, prefix):
    rc, msg = got
    assert rc == code, (rc, msg)
    assert msg.startswith(prefix), msg


@pytest.mark.parametrize("name,arg", [(n, a) for n in PLAIN + GUMBEL for a in ["handle"] + _required(n)] +
                         [(n, "handle") for n in GUMBEL_ALL[len(GUMBEL):]])
def test_null_required_pointer(name, arg, make, bufs):
    h = make(_flags(name))
    got = refused(name, None, bufs) if arg == "handle" else refused(name, h, bufs, **{arg: None})
    assert_refused(got, LZM_ERR_ARG, name + ":")


@pytest.mark.parametrize("name,arg", [("lzm_gumbel_get_children_values", "out"), ("lzm_gumbel_get_policies", "out"),
                                      ("lzm_gumbel_set_root_values", "values")])
def test_null_output_of_gumbel_getters(name, arg, make, bufs):
    # (these return the code without a message of their own)
    rc, _ = refused(name, make(LZM_TREE_GUMBEL), bufs, **{arg: None})
    assert rc == LZM_ERR_ARG


@pytest.mark.parametrize("name", PLAIN)
def test_gumbel_handle_on_plain_entry_point(name, make, bufs):
    assert_refused(refused(name, make(LZM_TREE_GUMBEL), bufs), LZM_ERR_STATE, name + ":")


@pytest.mark.parametrize("name", GUMBEL_ALL)
def test_plain_handle_on_gumbel_entry_point(name, make, bufs):
    assert_refused(refused(name, make(0), bufs), LZM_ERR_STATE, name + ":")


def test_plain_handle_on_gumbel_set_considered(make):
    L = _lib.load()
    assert L.lzm_gumbel_set_considered(make(0), SIMS, 2) == LZM_ERR_STATE
    assert L.lzm_last_error().startswith(b"lzm_gumbel_set_considered:")


@pytest.mark.parametrize("name", DECODES)
def test_even_support_len(name, make, bufs):
    assert_refused(refused(name, make(_flags(name)), bufs, support_len=4), LZM_ERR_ARG, name + ":")


@pytest.mark.parametrize("name", DECODES)
def test_even_value_support(name, make, bufs):
    h = make(_flags(name))
    assert _lib.load().lzm_set_value_support(h, 4) == LZM_OK
    assert_refused(refused(name, h, bufs), LZM_ERR_ARG, name + ":")


@pytest.mark.parametrize("name", TRAVERSES)
def test_pb_c_base_zero(name, make, bufs):
    assert_refused(refused(name, make(0), bufs, pb_c_base=0), LZM_ERR_ARG, name + ":")


@pytest.mark.parametrize("name", WITH_CUR)
@pytest.mark.parametrize("cur", [0, SIMS + 1])
def test_cur_outside_capacity(name, cur, make, bufs):
    assert_refused(refused(name, make(_flags(name)), bufs, cur=cur), LZM_ERR_CAPACITY,
                   f"latent index {cur} outside reserved capacity")


def test_fast_rng_handle_on_fused_decode_traverse(make, bufs):
    name = "lzm_decode_backprop_traverse"
    assert_refused(refused(name, make(LZM_RNG_FAST), bufs), LZM_ERR_ARG, name + ":")


def test_reuse_on_fast_rng_traverse(make, bufs):
    h = make(LZM_RNG_FAST)
    L = _lib.load()
    assert L.lzm_set_reuse(h, ctypes.c_void_p(bufs["reuse_action"].data_ptr()),
                           ctypes.c_void_p(bufs["reuse_value"].data_ptr())) == LZM_OK
    assert_refused(refused("lzm_traverse", h, bufs), LZM_ERR_ARG, "lzm_traverse:")
