"""CPU: the slice rule of the one-launch conv searches (lzm_conv_slice_roots, host arithmetic only) against
hand-derived values, and the sliced plan's argument checks (before any HIP call)."""
import ctypes

import pytest

from lightzero_amd import _lib

ARG, RESIDENCY = _lib.LZM_ERR_ARG, _lib.LZM_ERR_RESIDENCY

# (ez, B, H, resident workgroups R, max_roots) -> roots per slice. EfficientZero: T = ceil(B / 64) * H / 16 tiles
# for the whole batch, 2 m H / 16 tile halves for a slice of 64 m roots.
RULE = [
    # 1,536 roots: past 256, so slices of 64 m with max(64 m, 64 m) <= 256: m = 4 (6 slices)
    ((1, 1536, 512, 256, 0), 256),
    # 130 roots, H = 1024: whole 2 T = 2 * 3 * 64 = 384 > 256; max(64 m, 128 m) <= 256: m = 2
    ((1, 130, 1024, 256, 0), 128),
    # 130 roots, H = 128, R = 64: whole max(130, 48) > 64; m = 1: max(64, 16) = 64 fits, m = 2 does not (64, 64, 2)
    ((1, 130, 128, 64, 0), 64),
    # 21 roots fit whole (max(21, 16) <= 40) although no 64-root slice would
    ((1, 21, 128, 40, 0), 21),
    # not even m = 1 (max(64, 128) > 8)
    ((1, 130, 1024, 8, 0), RESIDENCY),
    # a cap below one row block on a batch that needs slices (130 > cap)
    ((1, 130, 128, 256, 32), ARG),
    ((0, 1536, 0, 0, 0), 1024),
    ((0, 300, 0, 0, 128), 128),
    ((0, 600, 0, 0, 0), 600),
]


@pytest.mark.parametrize("args,want", RULE)
def test_slice_rule(args, want):
    assert _lib.load().lzm_conv_slice_roots(*args) == want


def test_slice_rule_further_cases():
    f = _lib.load().lzm_conv_slice_roots
    assert f(1, 130, 128, 256, 0) == 130  # fits the single launch: no slicing without a cap
    assert f(1, 130, 128, 256, 64) == 64 and f(1, 130, 128, 256, 100) == 64 and f(1, 130, 128, 256, 128) == 128
    assert f(1, 64, 128, 256, 64) == 64 and f(1, 20, 128, 256, 32) == 20  # within the cap: the single launch
    assert f(1, 257, 128, 512, 0) == 256  # past 256 roots whatever is resident
    assert f(1, 1536, 512, 100, 0) == 64  # max(64 m, 64 m) <= 100: m = 1
    assert f(0, 2048, 0, 0, 0) == 1024 and f(0, 2048, 0, 0, 4096) == 1024 and f(0, 5, 0, 0, 1) == 1
    for bad in ((0, 0, 0, 0, 0), (1, -4, 128, 256, 0), (0, 8, 0, 0, -1), (1, 8, 0, 256, 0), (1, 8, 100, 256, 0)):
        assert f(*bad) == ARG, bad
    assert b"lzm_conv_slice_roots" in _lib.load().lzm_last_error()


def test_default_config_lists_the_keys_off():
    from lightzero_amd.mcts_ctree import EfficientZeroMCTSCtree, MuZeroMCTSCtree
    for cls in (MuZeroMCTSCtree, EfficientZeroMCTSCtree):
        cfg = cls.default_config()
        assert cfg.sliced_search is False and cfg.sliced_search_max_roots == 0


def test_sliced_plan_validates_on_the_host():
    """lzm_search_conv_sliced_plan refuses a null handle, a null output, no simulations and a negative cap
    before any HIP call (LZM_ERR_ARG) and leaves `out` alone"""
    L = _lib.load()
    out = (ctypes.c_int32 * 11)(*([7] * 11))
    fake = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first
    shape = (0, 0, 1, 1, 1, 16, 32, 1024, 2048, 1024, 601, 601, 1)
    assert L.lzm_search_conv_sliced_plan(None, 10, *shape, 0, out) == ARG
    assert b"lzm_search_conv_sliced_plan" in L.lzm_last_error()
    assert L.lzm_search_conv_sliced_plan(fake, 10, *shape, 0, None) == ARG
    assert L.lzm_search_conv_sliced_plan(fake, 0, *shape, 0, out) == ARG
    assert L.lzm_search_conv_sliced_plan(fake, -3, *shape, 0, out) == ARG
    assert L.lzm_search_conv_sliced_plan(fake, 10, *shape, -1, out) == ARG
    assert list(out) == [7] * 11
