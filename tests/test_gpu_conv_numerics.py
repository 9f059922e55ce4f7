"""GPU: the conv path's kernels against float64, one shape at a time — lzm_conv_trunk_p (split-fp16 and exact f32),
lzm_conv_trunk_xin_p, lzm_conv_heads and lzm_ez_lstm_step at the block counts, plane counts, head widths,
supports, LSTM widths and batch sizes the Atari configs never reach (tests/test_gpu_conv_shapes.py shows the
one-launch searches equal these kernels bit for bit; this file shows the kernels are right).

The yardstick is tests/test_gpu_split_range._check, unchanged: against a float64 restatement of the same operation,
|err| <= 2^-16 A element-wise (A: the same network with every weight, bias and input replaced by its absolute
value and every ReLU by the identity), the relative error's 99th percentile <= max(1e-5, 2 x torch-f32's) and its
max <= max(1e-3, 4 x torch-f32's). The worst figures per kernel are printed (pytest -s) and quoted in DESIGN.md §3.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lightzero_amd import _lib  # noqa: E402
from tests.test_gpu_split_range import DEV, _check, _trunk64  # noqa: E402

P = _lib.ptr


# ---- the recurrent trunk ------------------------------------------------------------------------------------
def raw_trunk(n_dres, n_pres, r_ch, h_ch, A, seed):
    """folded-trunk tensors (conv_infer.fold_tensors' names) with random values of a folded network's size:
    conv rows of unit L2 norm scaled by 0.7, biases ~0.1 — any block and plane count, which the models cannot
    all express (they share one num_res_blocks)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"dyn_w": r(64, 64, 3, 3) * (0.7 / 24), "dyn_actmap": r(A, 64, 8, 8) * 0.3}
    for name, n in (("dres", n_dres), ("pres", n_pres)):
        for i in range(n):
            t[f"{name}{i}_w1"], t[f"{name}{i}_b1"] = r(64, 64, 3, 3) * (0.7 / 24), r(64) * 0.1
            t[f"{name}{i}_w2"], t[f"{name}{i}_b2"] = r(64, 64, 3, 3) * (0.7 / 24), r(64) * 0.1
    t["rw_w"], t["rw_b"] = r(r_ch, 64, 1, 1) * (0.7 / 8), r(r_ch) * 0.1
    t["head_w"], t["head_b"] = r(h_ch, 64, 1, 1) * (0.7 / 8), r(h_ch) * 0.1
    return {k: v.float().contiguous() for k, v in t.items()}


def pack_trunk(t, n_dres, n_pres, r_ch, h_ch, prec):
    """lzm_conv_trunk_prepare_p on the raw weights in the order the C entry documents (FoldedConvNet._pack_native)"""
    parts = [t["dyn_w"]]
    for name, n in (("dres", n_dres), ("pres", n_pres)):
        if name == "pres":
            parts += [t["rw_w"], t["rw_b"]]
        for i in range(n):
            parts += [t[f"{name}{i}_w1"], t[f"{name}{i}_b1"], t[f"{name}{i}_w2"], t[f"{name}{i}_b2"]]
    parts += [t["head_w"], t["head_b"]]
    raw = np.ascontiguousarray(torch.cat([p.reshape(-1) for p in parts]).numpy(), dtype=np.float32)
    L = _lib.load()
    n = L.lzm_conv_trunk_floats_p(n_dres, n_pres, prec)
    assert n > 0
    host = np.zeros(n, np.float32)
    _lib.check(L.lzm_conv_trunk_prepare_p(prec, n_dres, n_pres, r_ch, h_ch, raw.ctypes.data, host.ctypes.data), "prepare")
    if prec == 1:
        _lib.check(L.lzm_conv_trunk_actmap_bound(n_dres, n_pres, float(t["dyn_actmap"].abs().max()), host.ctypes.data),
                   "actmap_bound")
    return torch.from_numpy(host).to(DEV)


TRUNK_CASES = [  # (n_dres, n_pres, r_ch, h_ch, B, A)
    (0, 0, 16, 32, 45, 18),
    (2, 2, 2, 4, 1, 1),
    (3, 1, 16, 32, 1, 18),
    (2, 2, 1, 1, 45, 1),
    (0, 0, 32, 32, 45, 18),
    (3, 1, 2, 4, 45, 1),
]
WORST = {}


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"worst max |err| / A so far, {family}: {WORST[family]:.2e} (bound {2.0 ** -16:.2e})")


@pytest.mark.parametrize("prec", ["split", "f32"])
@pytest.mark.parametrize("n_dres,n_pres,r_ch,h_ch,B,A", TRUNK_CASES)
def test_trunk_shapes_vs_float64(prec, n_dres, n_pres, r_ch, h_ch, B, A):
    """lzm_conv_trunk_p at 0 .. 3 residual blocks per network (unequal counts too), 1 .. 32 reward / head planes
    (partial and full 1x1 output tiles), 1 and 45 envs, 1 and 18 actions: next latent, reward planes and head
    planes element-wise against float64; no range error.
    A launch of one env writes 128 reward-plane values at 2 planes, half of them ReLU zeros: too few for _check's
    99th percentile, which is then the largest one or two elements (measured so, one launch, split, 2/2 blocks,
    2/4 planes: |err| / A 2.6e-7 as everywhere, but p99 1.43e-5 against 1e-5 on an element whose |ref| is 1/50 of
    its A). So the B = 1 cases launch the one-env grid 45 times on different latents and pool the outputs: the
    same launches, the same bounds, the statistic on as many values as the B = 45 cases.
    These cases found the exact-f32 trunk summing each 3 x 3 convolution's K = 576 in one chain of 288 MFMA steps:
    relative error 1.5 times torch-f32's in the median, three cases over the bounds (p99 6.68e-5 against 2 x
    2.32e-5 and 2.68e-5 against 2 x 1.19e-5, max 0.0400 against 4 x 0.0082). It now sums per tap in two fresh
    accumulators (lzm_conv.h conv_tile): 0.75 times torch-f32's in the median, every case inside."""
    t = raw_trunk(n_dres, n_pres, r_ch, h_ch, A, seed=n_dres * 100 + r_ch)
    p = {"f32": 0, "split": 1}[prec]
    blob = pack_trunk(t, n_dres, n_pres, r_ch, h_ch, p)
    g = torch.Generator().manual_seed(B + A)
    reps = 45 if B == 1 else 1
    N = B * reps
    lat = torch.relu(torch.randn(N, 64, 8, 8, generator=g))
    act = torch.randint(0, A, (N,), generator=g)
    d = lambda z, dt=torch.float32: z.to(DEV, dt).contiguous()
    out, r, h = torch.empty(N, 64, 8, 8, device=DEV), torch.empty(N, r_ch * 64, device=DEV), \
        torch.empty(N, h_ch * 64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pool, x, a32, amap = d(lat), torch.zeros(B, dtype=torch.int32, device=DEV), d(act, torch.int32), \
        d(t["dyn_actmap"])
    for i in range(reps):  # (pool [1][B][64][8][8] = rows i B .. of the latents)
        s = slice(i * B, (i + 1) * B)
        _lib.call("lzm_conv_trunk_p", p, B, n_dres, n_pres, r_ch, h_ch, P(blob), P(amap), P(pool[s]), P(x), P(a32[s]),
                  P(out[s]), P(r[s]), P(h[s]), P(err), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    ref = _trunk64(t, lat.double(), act, n_dres, n_pres)
    Ab = _trunk64(t, lat.double(), act, n_dres, n_pres, absolute=True)
    f32 = _trunk64(t, lat, act, n_dres, n_pres, dtype=torch.float32)
    for name, got, y, z, w in zip(("latent", "reward planes", "head planes"), (out, r, h), ref, Ab, f32):
        _note(f"trunk {prec}", _check(f"trunk {prec} {n_dres}/{n_pres} blocks {r_ch}/{h_ch} planes B {B} A {A} {name}",
                                      got.reshape(y.shape), y, z, w))


@pytest.mark.parametrize("H", [128, 1024])
def test_trunk_xin_row_and_scale(H):
    """lzm_conv_trunk_xin_p writes the EfficientZero LSTM input row [reward planes | hpool[x[b]][b]] and its
    scale exponent: the reward planes against float64 (the trunk's yardstick), the hidden part the pool row
    bit for bit, xscale = 14 - floor(log2(max(row's largest reward plane value, 1))) (lzm_conv.h ls_row_exp),
    the other outputs equal to lzm_conv_trunk_p's"""
    n_dres, n_pres, r_ch, h_ch, B, A, slots = 2, 2, 6, 10, 21, 6, 3
    t = raw_trunk(n_dres, n_pres, r_ch, h_ch, A, seed=H)
    g = torch.Generator().manual_seed(H + 1)
    pool = torch.relu(torch.randn(slots, B, 64, 8, 8, generator=g))
    pool[:, ::2] *= 3.0
    hpool = torch.tanh(torch.randn(slots, B, H, generator=g))
    x = torch.randint(0, slots, (B,), generator=g)
    act = torch.randint(0, A, (B,), generator=g)
    # the reward 1x1 (weights and bias: ReLU is positively homogeneous) rescaled so that the rows' largest reward
    # plane value has median 2: rows below 2 (exponent 14, the floor max(., 1) included) and rows from 2 up (<= 13)
    m = _trunk64(t, pool[x, torch.arange(B)], act, n_dres, n_pres, dtype=torch.float32)[1].amax(dim=1).median() / 2
    t["rw_w"], t["rw_b"] = t["rw_w"] / m, t["rw_b"] / m
    blob = pack_trunk(t, n_dres, n_pres, r_ch, h_ch, 1)
    Kr = r_ch * 64
    d = lambda z, dt=torch.float32: z.to(DEV, dt).contiguous()
    out, xin, hd = torch.empty(B, 64, 8, 8, device=DEV), torch.full((B, Kr + H), float("nan"), device=DEV), \
        torch.empty(B, h_ch * 64, device=DEV)
    xscale = torch.full((B,), -999, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    dp, dh, dx, da, amap = d(pool), d(hpool), d(x, torch.int32), d(act, torch.int32), d(t["dyn_actmap"])
    _lib.call("lzm_conv_trunk_xin_p", 1, B, n_dres, n_pres, r_ch, h_ch, P(blob), P(amap), P(dp), P(dx), P(da), P(out),
              P(xin), Kr + H, P(dh), H, P(xscale), P(hd), P(err), _lib.stream_ptr())
    out2, r2, h2 = torch.empty_like(out), torch.empty(B, Kr, device=DEV), torch.empty_like(hd)
    _lib.call("lzm_conv_trunk_p", 1, B, n_dres, n_pres, r_ch, h_ch, P(blob), P(amap), P(dp), P(dx), P(da), P(out2),
              P(r2), P(h2), P(err), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    rows = torch.arange(B)
    lat = pool[x, rows]
    ref = _trunk64(t, lat.double(), act, n_dres, n_pres)
    Ab = _trunk64(t, lat.double(), act, n_dres, n_pres, absolute=True)
    f32 = _trunk64(t, lat, act, n_dres, n_pres, dtype=torch.float32)
    _note("trunk xin", _check(f"xin H {H} reward planes", xin[:, :Kr], ref[1], Ab[1], f32[1]))
    assert torch.equal(xin[:, Kr:].cpu(), hpool[x, rows])
    assert torch.equal(xin[:, :Kr], r2) and torch.equal(out, out2) and torch.equal(hd, h2)
    rmax = xin[:, :Kr].cpu().double().amax(dim=1).clamp_min(1.0)
    exp = (14 - torch.floor(torch.log2(rmax))).to(torch.int32)
    assert torch.equal(xscale.cpu(), exp), (xscale.cpu(), exp)
    assert exp.min() < 14 and exp.max() == 14  # rows on both sides of 2


# ---- the head MLPs ------------------------------------------------------------------------------------------
def pack_w1t(W):
    """[96][1024] (three heads' hidden layers, zero past each head's K) -> lzm_conv_heads' w1t [3][8][32][32][4]"""
    return W.reshape(3, 32, 8, 32, 4).permute(0, 2, 3, 1, 4).contiguous()


HEAD_CASES = [  # (Kr, Kv, Kp, Vr, Vv, A, B, form: "mz" r as is / "ez" relu(r * scale + shift) / "pred" r = NULL)
    (128, 128, 128, 1, 1, 1, 1, "mz"),
    (384, 128, 1024, 2, 255, 18, 2, "ez"),
    (1024, 384, 128, 256, 257, 256, 3, "mz"),
    (128, 1024, 384, 767, 768, 1, 3, "ez"),
    (1024, 1024, 1024, 768, 2, 18, 1, "mz"),
    (384, 384, 384, 255, 256, 256, 2, "pred"),
    (1024, 128, 384, 257, 767, 18, 3, "pred"),
    (128, 384, 1024, 769, 1024, 18, 3, "ez"),   # the four-columns-per-thread form (supports past 768)
    (1024, 1024, 128, 1024, 769, 1, 2, "mz"),
]


@pytest.mark.parametrize("Kr,Kv,Kp,Vr,Vv,A,B,form", HEAD_CASES)
def test_heads_shapes_vs_float64(Kr, Kv, Kp, Vr, Vv, A, B, form):
    """lzm_conv_heads (plain f32 FMA) at head widths 128 / 384 / 1024 (dead K-parts, whose weights are NaN here:
    they must not be read), supports
    1 .. 1024 on either side of the 256-, 768-column steps, 1 / 18 / 256 actions, 1 .. 3 envs (the two-env
    workgroup with a missing second row), with the EfficientZero input affine map, without, and without a reward
    head: every output element-wise against float64; the verdict words for rows that do not and that do sum to 1"""
    g = torch.Generator().manual_seed(Kr + Vv + A)
    rn = lambda *s: torch.randn(*s, generator=g)
    pred = form == "pred"
    Khd = Kv + Kp
    r = torch.relu(rn(B, Kr)) if form == "mz" else rn(B, Kr)
    hd = torch.relu(rn(B, Khd))
    scale, shift = torch.rand(Kr, generator=g) + 0.5, rn(Kr) * 0.2
    # past each head's K the K-parts are dead and never read: NaN there instead of the packed layout's zeros
    W = torch.full((96, 1024), float("nan"))
    for hh, K in enumerate((Kr, Kv, Kp)):
        W[32 * hh:32 * hh + 32, :K] = rn(32, K) / K ** 0.5
    b1 = rn(96) * 0.1
    N2 = Vr + Vv + A
    d = lambda z: z.to(DEV).contiguous()
    for normalised in (False, True):
        if normalised:  # exactly normalised reward / value rows: zero weights, bias 1 / V
            w2 = torch.cat([torch.zeros(Vr + Vv, 32), rn(A, 32) / 32 ** 0.5])
            b2 = torch.cat([torch.full((Vr,), 1.0 / Vr), torch.full((Vv,), 1.0 / Vv), rn(A) * 0.1])
        else:
            w2, b2 = rn(N2, 32) / 32 ** 0.5, rn(N2) * 0.1
        outs = [torch.full((B, n), float("nan"), device=DEV) for n in (Vr, Vv, A)]
        nparts = (B + 1) // 2
        words = torch.full((2 * nparts,), -7, dtype=torch.int32, device=DEV)
        dev = [d(z) for z in (r, scale, shift, hd, pack_w1t(W), b1, w2.t(), b2)]
        _lib.call("lzm_conv_heads", B, 0 if pred else Kr, Khd, Kv, None if pred else P(dev[0]),
                  P(dev[1]) if form == "ez" else None, P(dev[2]) if form == "ez" else None, P(dev[3]), P(dev[4]),
                  P(dev[5]), P(dev[6]), P(dev[7]), Vr, Vv, A, None if pred else P(outs[0]), P(outs[1]), P(outs[2]),
                  None if pred else P(words), _lib.stream_ptr())
        torch.cuda.synchronize()

        def net(dt, absolute=False):
            f = (lambda z: z.abs()) if absolute else (lambda z: z)
            relu = (lambda z: z) if absolute else (lambda z: z.relu())
            c = lambda z: f(z.to(dt))
            xr = c(r)
            if form == "ez":
                xr = relu(xr * c(scale) + c(shift))
            ins = (xr, c(hd)[:, :Kv], c(hd)[:, Kv:])
            res, j = [], 0
            for hh, (K, V) in enumerate(((Kr, Vr), (Kv, Vv), (Kp, A))):
                hid = relu(ins[hh] @ c(W[32 * hh:32 * hh + 32, :K]).t() + c(b1[32 * hh:32 * hh + 32]))
                res.append(hid @ c(w2[j:j + V]).t() + c(b2[j:j + V]))
                j += V
            return res
        ref, Ab, f32 = net(torch.float64), net(torch.float64, True), net(torch.float32)
        for hh, name in enumerate(("reward", "value", "policy")):
            if pred and hh == 0:
                continue
            _note("heads", _check(f"heads {form} K {Kr}/{Kv}/{Kp} V {Vr}/{Vv} A {A} B {B} {name}"
                                  f"{' normalised' if normalised else ''}", outs[hh], ref[hh], Ab[hh], f32[hh]))
        if not pred:
            w = words.cpu().numpy().reshape(nparts, 2)
            for hh in (0, 1):
                ok = np.abs(outs[hh].sum(dim=1).cpu().numpy() - 1.0) <= 2e-5
                exp = np.array([int(ok[2 * q:2 * q + 2].all()) for q in range(nparts)], np.int32)
                assert np.array_equal(w[:, hh], exp), (normalised, hh, w)
            assert bool(w.all()) == normalised, w


# ---- the EfficientZero LSTM step ------------------------------------------------------------------------------
LSTM_CASES = [  # (H, Kr, B, horizon, workspace)
    (128, 128, 1, 1, True),
    (128, 1024, 63, 3, False),
    (128, 128, 130, 3, True),
    (256, 1024, 64, 1, True),
    (256, 128, 65, 3, False),
    (1024, 128, 65, 3, True),
    (1024, 1024, 130, 1, False),
    (1024, 1024, 1, 3, True),
]


@pytest.mark.parametrize("H,Kr,B,horizon,workspace", LSTM_CASES)
def test_lstm_step_shapes_vs_float64(H, Kr, B, horizon, workspace):
    """lzm_ez_lstm_step (split-fp16 gate GEMM + cell) at LSTM widths 128 / 256 / 1024, K = 128 + H and 1024 + H,
    1 .. 130 rows (row blocks of 64 holding one live row), with the split-K workspace and without: the new h / c
    element-wise against a float64 LSTM cell, the state slots = the new state zeroed where search_len % horizon
    == 0 (bit for bit), no hand-off or range error.
    One case found the form without a workspace summing K = 1,152 in one chain: absolute error 1.5 times
    torch-f32's over the output and, on a cell state that cancels to -4.8e-6, relative error max 0.0316 against
    4 x 0.0035. The kernel now sums the two K halves apart in that form too (the split form's order), so both
    forms give the same bits, which is asserted."""
    K, slots = Kr + H, 3
    g = torch.Generator().manual_seed(H + Kr + B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    xin64 = torch.cat([torch.relu(rn(B, Kr)), torch.tanh(rn(B, H))], dim=1).float().double()
    W64 = (rn(4 * H, K) / K ** 0.5).float().double()
    b64 = (rn(4 * H) * 0.1).float().double()
    cpool64 = (rn(slots, B, H) * 0.5).float().double()
    x = torch.randint(0, slots, (B,), generator=g)
    slen = torch.randint(1, 7, (B,), generator=g)
    if B > 1:
        slen[0], slen[1] = 3, 4  # a multiple of both horizons; a multiple of 1 only
    L = _lib.load()
    host = np.zeros(L.lzm_ez_lstm_frag_floats(K, H), np.float32)
    Wn = np.ascontiguousarray(W64.float().numpy())
    _lib.check(L.lzm_ez_lstm_prepare(K, H, Wn.ctypes.data, host.ctypes.data), "prepare")
    frag = torch.from_numpy(host).to(DEV)
    d = lambda z, dt=torch.float32: z.to(DEV, dt).contiguous()
    xin, bias, cpool, dx, dl = d(xin64), d(b64), d(cpool64), d(x, torch.int32), d(slen, torch.int32)
    rmax = xin64[:, :Kr].amax(dim=1).clamp_min(1.0)
    xscale = d(14 - torch.floor(torch.log2(rmax)), torch.int32)
    outs = [torch.full((B, H), float("nan"), device=DEV) for _ in range(4)]
    ws = torch.zeros((int(L.lzm_ez_lstm_workspace_bytes(B, H)) + 15) // 16 * 4, device=DEV) if workspace else None
    werr = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("lzm_ez_lstm_step", B, K, H, P(xin), P(xscale), P(frag), P(bias), P(cpool), P(dx), P(dl), horizon,
              P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), P(ws), P(werr), P(werr[1:]), _lib.stream_ptr())
    # the other form (without the workspace / with it): the K halves are summed apart either way, the same bits
    other = [torch.full((B, H), float("nan"), device=DEV) for _ in range(4)]
    ws2 = None if workspace else torch.zeros((int(L.lzm_ez_lstm_workspace_bytes(B, H)) + 15) // 16 * 4, device=DEV)
    _lib.call("lzm_ez_lstm_step", B, K, H, P(xin), P(xscale), P(frag), P(bias), P(cpool), P(dx), P(dl), horizon,
              P(other[0]), P(other[1]), P(other[2]), P(other[3]), P(ws2), P(werr), P(werr[1:]), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert werr.tolist() == [0, 0]
    for a, b in zip(outs, other):
        assert torch.equal(a, b)
    c0 = cpool64[x, torch.arange(B)]

    def cell(xi, W, b, c):
        gi, gf, gg, go = (xi @ W.t() + b).chunk(4, dim=1)
        c1 = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        return torch.sigmoid(go) * torch.tanh(c1), c1
    h1, c1 = cell(xin64, W64, b64, c0)
    h32, c32 = cell(xin64.float(), W64.float(), b64.float(), c0.float())
    Ag = xin64.abs() @ W64.abs().t() + b64.abs()
    Ab = torch.stack(Ag.chunk(4, dim=1)).amax(dim=0) * (1 + c0.abs())
    name = f"lstm H {H} K {K} B {B}{' split-K' if workspace else ''}"
    _note("lstm", _check(name + " h1", outs[0], h1, Ab, h32))
    _note("lstm", _check(name + " c1", outs[1], c1, Ab, c32))
    keep = (slen % horizon != 0).to(DEV).unsqueeze(1)
    assert torch.equal(outs[2], torch.where(keep, outs[0], torch.zeros_like(outs[0])))
    assert torch.equal(outs[3], torch.where(keep, outs[1], torch.zeros_like(outs[1])))
    if B > 1:
        assert not keep[0] and bool(keep[1]) == (horizon == 3)
