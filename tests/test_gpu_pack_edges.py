"""GPU: episodes_scan_kernel / episodes_pack_kernel (csrc/lzm_traj.h) at the edges no collector run has launched.

The suite compared the device packing with trajectory.pack_episodes at n = 24, E = 6, T = 100 and frames of 16 B
and 4,096 B. Here no env runs: the record buffers hold seeded finite values and the three counters (ep_count,
consumed, ep_len) are written directly, so that one launch sees a scan with more than one env per thread
(n > 1024) and threads whose range is empty, envs with no new episode, with ep_count < consumed, with E - 1 new
ones and slots that wrap, episodes longer than the pack kernel's 256-thread stride, the byte-copy path
(frame_bytes not a multiple of 16, an unaligned output), every column layout, and the overflow flag.

Compared, all exact: index, frames and scalars with trajectory.pack_episodes on the same buffers (torch.equal),
env_ep_off / env_row_off with the host's exclusive sums, totals, consumed == ep_count afterwards, and canary tails
behind every output. The counters and offsets are allocated up to the scan's whole thread range (1024 x the envs
per thread) with a canary tail of their own, so a thread that runs past n shows there.

Every ep_len here is <= T, the contract of lzm_episodes_pack (include/lzmcts.h): a longer slot would be read
outside the record buffers.
"""
import numpy as np
import pytest
import torch

from lightzero_amd.trajectory import pack_episodes, scalar_width

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TAIL = 3            # canary rows / episodes behind the outputs
OFF_CANARY = -7
SCAN_THREADS = 1024


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pack(n, E, T, A, fb, new, consumed, lens, has_pred=True, gumbel=False, ret=True, seed=0, unaligned_out=False,
          over=0):
    """new [n]: ep_count - consumed per env (may be negative or beyond E); lens [n][E]: every slot's ep_len"""
    from lightzero_amd._lib import call, ptr, stream_ptr
    rng = np.random.default_rng(seed)
    new, consumed, lens = np.asarray(new, np.int64), np.asarray(consumed, np.int64), np.asarray(lens, np.int32)
    assert lens.shape == (n, E) and lens.min() >= 1 and lens.max() <= T and (consumed + new >= 0).all()
    ep_count = consumed + new
    # ---- the record buffers: seeded finite values
    rec_frames = _dev(rng.integers(0, 256, (n, E, T + 1, fb), dtype=np.uint8))
    rec_action = _dev(rng.integers(0, A, (n, E, T)).astype(np.int32))
    rec_visits = _dev(rng.integers(0, 51, (n, E, T, A)).astype(np.int32))
    rec_reward, rec_value, rec_pred, rec_cq = (_dev(rng.normal(size=(n, E, T)).astype(np.float32)) for _ in range(4))
    rec_policy = _dev(rng.random((n, E, T, A), dtype=np.float32))
    ep_return = _dev((rng.normal(size=(n, E)) * 30).astype(np.float32))
    # ---- the counters, allocated over the scan's whole thread range; behind n they describe one more new episode
    # per env, which a scan that runs past n would count
    NP = SCAN_THREADS * ((n + SCAN_THREADS - 1) // SCAN_THREADS)
    pad = lambda a, v: np.concatenate([a, np.full((NP - n,) + a.shape[1:], v, a.dtype)])
    d_count, d_cons = _dev(pad(ep_count.astype(np.int32), 1)), _dev(pad(consumed.astype(np.int32), 0))
    d_len = _dev(pad(lens, 1))
    ep_off = torch.full((NP,), OFF_CANARY, dtype=torch.int32, device=DEV)
    row_off = torch.full((NP,), OFF_CANARY, dtype=torch.int64, device=DEV)
    totals = torch.full((3,), OFF_CANARY, dtype=torch.int64, device=DEV)
    call("lzm_episodes_scan", n, E, ptr(d_count), ptr(d_cons), ptr(d_len), ptr(ep_off), ptr(row_off), ptr(totals),
         stream_ptr())
    # ---- the host's list: env-major, each env's episodes in finishing order, the counts clamped to [0, E]
    nw = np.clip(new, 0, E)
    episodes = [(i, int((consumed[i] + k) % E), int(lens[i, (consumed[i] + k) % E])) for i in range(n)
                for k in range(int(nw[i]))]
    rows_per_env = np.zeros(n, np.int64)
    for i, _, L in episodes:
        rows_per_env[i] += L + 1
    n_ep, rows = len(episodes), int(rows_per_env.sum())
    assert totals.cpu().tolist() == [n_ep, rows, over]
    assert np.array_equal(ep_off[:n].cpu().numpy(), np.cumsum(nw) - nw)
    assert np.array_equal(row_off[:n].cpu().numpy(), np.cumsum(rows_per_env) - rows_per_env)
    assert (ep_off[n:] == OFF_CANARY).all() and (row_off[n:] == OFF_CANARY).all()
    # ---- outputs sized from totals, plus a canary tail
    W = scalar_width(A, has_pred, gumbel)
    raw = torch.full(((rows + TAIL) * fb + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    out_frames = raw[1:1 + (rows + TAIL) * fb] if unaligned_out else raw[:(rows + TAIL) * fb]
    out_scalars = torch.full((rows + TAIL, W), -123.0, device=DEV)
    out_index = torch.full((n_ep + TAIL, 3), -9, dtype=torch.int64, device=DEV)
    common = [n, E, T, A, int(has_pred), fb, ptr(d_count), ptr(d_len), ptr(d_cons), ptr(ep_off), ptr(row_off),
              ptr(rec_frames), ptr(rec_action), ptr(rec_reward), ptr(rec_visits), ptr(rec_value),
              ptr(rec_pred) if has_pred else None]
    outs = [ptr(ep_return) if ret else None, ptr(out_frames), ptr(out_scalars), ptr(out_index), stream_ptr()]
    if gumbel:
        call("lzm_episodes_pack_gumbel", *common, ptr(rec_policy), ptr(rec_cq), *outs)
    else:
        call("lzm_episodes_pack", *common, *outs)
    torch.cuda.synchronize()
    ref = pack_episodes(rec_frames, rec_action, rec_reward, rec_visits, rec_value, episodes,
                        rec_pred if has_pred else None, 1.0, ep_return=ep_return if ret else None,
                        rec_policy=rec_policy if gumbel else None, rec_cq=rec_cq if gumbel else None)
    assert ref.scalars.shape == (rows, W) and ref.frames.shape == (rows, fb)
    assert torch.equal(out_index[:n_ep].cpu(), ref.index)
    assert torch.equal(out_frames[:rows * fb].reshape(rows, fb), ref.frames)
    assert torch.equal(out_scalars[:rows], ref.scalars)
    if rows:  # row L of every episode: zeros but for the return
        last = ref.index[:, 2] + ref.index[:, 1]
        z = out_scalars[last.to(DEV)]
        assert (z[:, 0] == 0).all() and (z[:, 2:] == 0).all() and (ret or (z[:, 1] == 0).all())
    assert (out_frames[rows * fb:] == 0xEE).all() and (raw[-15:] == 0xEE).all()
    assert not unaligned_out or (raw[0] == 0xEE and out_frames.data_ptr() % 16 == 1)  # the byte before the view
    assert (out_scalars[rows:] == -123.0).all() and (out_index[n_ep:] == -9).all()
    assert torch.equal(d_cons[:n], d_count[:n]) and (d_cons[n:] == 0).all()
    return n_ep, rows


def _mixed(n, E, rng):
    """per env: no new episode, ep_count < consumed, 1, E - 1, with consumed values whose slots wrap"""
    new = np.tile([0, -1, 1, E - 1, 1, -3, E - 1, 0], n // 8 + 1)[:n] if n > 1 else np.array([E - 1])
    consumed = 3 + rng.integers(0, 3 * E, n)  # (>= 3: the negative counts stay >= 0)
    return new, consumed


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_scan_chunks_and_empty_ranges(n):
    """scan chunks of 1, 2 and 3 envs per thread, with trailing threads whose range is empty"""
    E, T = 3, 5
    rng = np.random.default_rng(n)
    new, consumed = _mixed(n, E, rng)
    n_ep, _ = _pack(n, E, T, 2, 16, new, consumed, rng.integers(1, T + 1, (n, E)), seed=n)
    assert n_ep == int(np.clip(new, 0, E).sum())
    assert n == 1 or ((new == E - 1) & (consumed % E == E - 1)).any()  # slots E - 1, 0: a wrap


def test_overflow_is_flagged_and_clamped():
    E, T, n = 3, 5, 5
    rng = np.random.default_rng(2)
    n_ep, _ = _pack(n, E, T, 2, 16, [E, E + 2, 1, 0, E - 1], [4, 5, 0, 2, 7], rng.integers(1, T + 1, (n, E)), over=1)
    assert n_ep == E + E + 1 + 0 + E - 1


def test_episode_lengths_around_the_pack_stride():
    """L of 1, 255, 256, 257 and 600 = T: the row loop's second and third trip, row L behind the stride"""
    E, T, n = 3, 600, 3
    lens = np.array([[1, 255, 7], [256, 257, 9], [600, 3, 2]], np.int32)
    n_ep, rows = _pack(n, E, T, 2, 16, [2, 2, 1], [0, 3, 6], lens, seed=4)
    assert n_ep == 5 and rows == 1 + 255 + 256 + 257 + 600 + 5


@pytest.mark.parametrize("fb,unaligned", [(16, False), (4096, False), (4, False), (20, False), (20, True)])
def test_frame_bytes_vector_and_byte_paths(fb, unaligned):
    E, T, n = 3, 5, 5
    rng = np.random.default_rng(fb)
    new, consumed = _mixed(n, E, rng)
    _pack(n, E, T, 2, fb, new, consumed, rng.integers(1, T + 1, (n, E)), seed=fb, unaligned_out=unaligned)


@pytest.mark.parametrize("has_pred,gumbel,ret", [(0, 0, 1), (1, 0, 1), (0, 1, 0), (1, 1, 1), (1, 0, 0)])
@pytest.mark.parametrize("A", [1, 2, 6, 64])
def test_column_layouts(A, has_pred, gumbel, ret):
    E, T, n = 3, 5, 6
    rng = np.random.default_rng(A)
    new, consumed = _mixed(n, E, rng)
    _pack(n, E, T, A, 16, new, consumed, rng.integers(1, T + 1, (n, E)), has_pred=bool(has_pred), gumbel=bool(gumbel),
          ret=bool(ret), seed=A)


def test_misaligned_buffer_is_refused_at_vector_frame_sizes():
    from lightzero_amd._lib import LZM_ERR_ARG, load, ptr, stream_ptr
    n, E, T, A = 2, 2, 3, 2
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    frames, out = z((n * E * (T + 1) * 16 + 16,), torch.uint8), torch.full((1024,), 0xEE, dtype=torch.uint8, device=DEV)
    count, cons, ln = z((n,), torch.int32) + 1, z((n,), torch.int32), z((n, E), torch.int32) + 1
    off, roff = z((n,), torch.int32), z((n,), torch.int64)
    ri, rf = z((n, E, T, A), torch.int32), z((n, E, T, A), torch.float32)
    sc, ix = torch.full((64, 8), -123.0, device=DEV), torch.full((8, 3), -9, dtype=torch.int64, device=DEV)
    for src, dst in ((frames, out[1:]), (frames[1:], out)):
        rc = load().lzm_episodes_pack(n, E, T, A, 0, 16, ptr(count), ptr(ln), ptr(cons), ptr(off), ptr(roff), ptr(src),
                                      ptr(ri), ptr(rf), ptr(ri), ptr(rf), None, None, ptr(dst), ptr(sc), ptr(ix),
                                      stream_ptr())
        assert rc == LZM_ERR_ARG
    torch.cuda.synchronize()
    assert (out == 0xEE).all() and (sc == -123.0).all() and (ix == -9).all() and (cons == 0).all()  # nothing ran
