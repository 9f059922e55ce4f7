"""GPU: the register walk's mean-q settle (lzm_search_res.h settle_chain, lzm_numerics.h div_small).

- lzm_debug_div_small against numpy float32 division, bit for bit, on a strided sweep of the 2^32
  patterns and the special values, for each divisor 1, 2, 3.
- lzm_debug_settle_chain (one wave running the walk's own settle on a synthetic path) against the
  sequential float32 recurrence, bit for bit, at path lengths around the 16-lane row and 32-lane
  boundaries a DPP shift crosses, with tv == 0 at the root, tq == -0.0, an inf, a NaN and an
  overflowing sum (the serial fallback).
- Whole fused searches against OracleTree fed the recorded network outputs
  (tests/test_gpu_fused.check_tree_exact), over the regimes that settle: random heads, heads
  sharpened x30 (mid-walk settles), zero heads (settle, then the resumed walk), two players, the
  longest search the register walk serves; selection modes 4 and 5 against each other.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lightzero_amd._lib import call, ptr, stream_ptr  # noqa: E402
from tests import test_gpu_fused as tf  # noqa: E402
from tests.test_gpu_fused import check_tree_exact  # noqa: E402
from tests.test_gpu_walk_regs import assert_both_endings, heads, midwalk_settles, patch_model  # noqa: E402

DEV = torch.device("cuda", 0)
A, H = 2, 128
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001,
                    0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x3f800000], np.uint32)


def same_bits(got, want):
    """bit-equal where want is a number, NaN where it is NaN"""
    nan = np.isnan(want)
    return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and bool(np.isnan(got[nan]).all())


@pytest.fixture(scope="module")
def sweep():
    bits = np.concatenate([np.arange(0, 1 << 32, 1021, dtype=np.uint64).astype(np.uint32), SPECIAL])  # about 2^22
    return bits.view(np.float32)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_div_small_equals_division(sweep, d):
    x = torch.from_numpy(sweep).to(DEV)
    dv = torch.full((len(sweep),), d, dtype=torch.int32, device=DEV)
    out = torch.empty_like(x)
    call("lzm_debug_div_small", ptr(x), ptr(dv), ptr(out), len(sweep), stream_ptr())
    got = out.cpu().numpy()
    with np.errstate(all="ignore"):
        want = sweep / np.float32(d)
    assert want.dtype == np.float32
    assert np.array_equal(got, want, equal_nan=True)
    assert same_bits(got, want)  # (array_equal takes -0 for +0)


def chain_reference(tq, tv):
    """q_0 = tq_0 / tv_0 when tv_0 > 0, else (0 + tq_0) / 1; q_l = (q_{l-1} + tq_l) / (tv_l + 1): float32"""
    out = np.empty(len(tq), np.float32)
    q = np.float32(0.0)
    with np.errstate(all="ignore"):
        for l in range(len(tq)):
            if l == 0 and tv[0] > 0:
                q = np.float32(tq[0]) / np.float32(tv[0])
            else:
                q = (q + np.float32(tq[l])) / np.float32(tv[l] + 1)
            out[l] = q
    return out


def dev_chain(tq, tv):
    n = len(tq)
    a = torch.from_numpy(np.ascontiguousarray(tq, np.float32)).to(DEV)
    b = torch.from_numpy(np.ascontiguousarray(tv, np.int32)).to(DEV)
    out = torch.full((n,), -12345.0, dtype=torch.float32, device=DEV)
    call("lzm_debug_settle_chain", ptr(a), ptr(b), n, ptr(out), stream_ptr())
    return out.cpu().numpy()


LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63]


def chain_inputs(n, seed, root_tv):
    rng = np.random.default_rng(seed)
    tq = (rng.normal(size=n) * rng.choice([1e-3, 1.0, 300.0], size=n)).astype(np.float32)
    tv = rng.integers(0, 3, size=n).astype(np.int32)
    tv[0] = root_tv
    return tq, tv


@pytest.mark.parametrize("root_tv", [0, 1, 2])
@pytest.mark.parametrize("n", LENGTHS)
def test_settle_chain_equals_sequential_recurrence(n, root_tv):
    tq, tv = chain_inputs(n, 100 * n + root_tv, root_tv)
    assert same_bits(dev_chain(tq, tv), chain_reference(tq, tv))


@pytest.mark.parametrize("n", LENGTHS)
def test_settle_chain_negative_zero(n):
    """tq == -0.0 at the root (tv 0 and 2: 0 + -0 = +0 against -0 / 2 = -0), in mid-path and after a -0 value"""
    for root_tv in (0, 2):
        tq, tv = chain_inputs(n, 7 * n + root_tv, root_tv)
        tq[0] = -0.0
        if n > 1:
            tq[1] = -0.0
        if n > 20:
            tq[20] = -0.0
        want = chain_reference(tq, tv)
        if root_tv == 2:
            assert want.view(np.uint32)[0] == 0x80000000
        assert same_bits(dev_chain(tq, tv), want)


@pytest.mark.parametrize("what", ["inf", "nan", "overflow", "subnormal"])
@pytest.mark.parametrize("n", [17, 33, 63])
def test_settle_chain_non_finite_mid_path(n, what):
    tq, tv = chain_inputs(n, 13 * n, 1)
    k = n // 2
    if what == "inf":
        tq[k] = -np.inf
    elif what == "nan":
        tq[k] = np.nan
    elif what == "overflow":  # finite terms, an infinite sum: the check after the pass
        tq[k - 1] = tq[k] = np.float32(3.0e38)
        tv[k - 1] = tv[k] = 0
    else:
        tq[k - 1:k + 2] = np.array([1e-44, -3e-45, 1.4e-45], np.float32)
        tq[:k - 1] = 0.0
    want = chain_reference(tq, tv)
    if what == "nan":
        assert np.isnan(want[k:]).all() and not np.isnan(want[:k]).any()
    if what in ("inf", "overflow"):
        assert np.isinf(want[k])
    assert same_bits(dev_chain(tq, tv), want)


# ---- whole searches: B, S, A, H, zero_heads, players, fast
def sharpen(m):
    for lin in heads(m):
        lin.weight.mul_(30.0)
        lin.bias.mul_(30.0)


@pytest.mark.parametrize("case", [(8, 50, A, H, False, 1, False), (1, 10, A, H, False, 1, False),
                                  (8, 25, A, H, False, 2, False), (2, 62, A, H, False, 1, False)], ids=tf._case_id)
def test_search_random_heads(case):
    check_tree_exact(case)


def test_search_sharpened_heads_settle_in_mid_walk(monkeypatch):
    patch_model(monkeypatch, sharpen)
    r = check_tree_exact((8, 50, A, H, False, 1, False))
    n = midwalk_settles(r["rec"])
    print(f"simulations crossing a one-visited-child node above their last level: {n}")
    assert n >= 1, "no walk crossed a node with one visited child and continued"


def test_search_zero_heads_settle_then_resume():
    r = check_tree_exact((8, 25, A, H, True, 1, False))
    assert r["diag"][2] > 0, "no tie between visited children was resolved through depth speculation"


@pytest.mark.parametrize("sharp", [False, True], ids=["rand", "sharp"])
def test_modes_4_and_5_agree(sharp, monkeypatch):
    if sharp:
        patch_model(monkeypatch, sharpen)
    out = {}
    for mode in ("4", "5"):
        monkeypatch.setenv("LZM_RES_SELECT", mode)
        out[mode] = check_tree_exact((8, 50, A, H, False, 1, False))
    for f in ("x", "action", "search_len"):
        assert np.array_equal(out["4"]["rec"][f], out["5"]["rec"][f]), f
    for f in ("dist", "values", "traj"):
        assert np.array_equal(out["4"][f], out["5"][f]), f
    if not sharp:
        assert_both_endings(out["5"]["rec"])
