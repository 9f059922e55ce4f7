"""CPU: what Gumbel MuZero collection adds above the search — the Gumbel TrajBlock columns and their marker, the
GameSegment's improved policies through the segment cut and pad_over, and the numpy-stream order of
GumbelMuZeroCollectPolicy (the search stubbed: no GPU).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lightzero_amd.trajectory import LAYOUT_GUMBEL, LAYOUT_PRED, TrajBlock, flatten_block, pack_episodes, \
    scalar_width, unflatten_block, unpack_episodes, wire_bytes

N, E, T = 3, 2, 4
EPISODES = [(0, 0, 4), (0, 1, 2), (1, 0, 1), (2, 1, 3)]  # (env, slot, L)


def records(A, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = dict(frames=torch.rand((N, E, T + 1, 4), generator=g),
             action=torch.randint(0, A, (N, E, T), generator=g, dtype=torch.int32),
             reward=torch.rand((N, E, T), generator=g),
             visits=torch.randint(0, 9, (N, E, T, A), generator=g, dtype=torch.int32),
             value=torch.randn((N, E, T), generator=g), pred=torch.randn((N, E, T), generator=g),
             policy=torch.softmax(torch.randn((N, E, T, A), generator=g), dim=-1),
             cq=torch.rand((N, E, T), generator=g), ret=torch.rand((N, E), generator=g) * 10)
    return r


def pack(r, pred, gumbel):
    return pack_episodes(r["frames"], r["action"], r["reward"], r["visits"], r["value"], EPISODES,
                         rec_pred=r["pred"] if pred else None, ep_return=r["ret"],
                         rec_policy=r["policy"] if gumbel else None, rec_cq=r["cq"] if gumbel else None)


def wire(block):
    """flatten_block -> unflatten_block with the marker the header exchange carries"""
    buf = flatten_block(block)
    assert buf.numel() == wire_bytes(block)
    return unflatten_block(buf, block.rows, block.num_episodes, tuple(block.frames.shape[1:]), block.frames.dtype,
                           block.scalars.shape[1], block.frame_scale, block.layout)


@pytest.mark.parametrize("pred", [False, True])
@pytest.mark.parametrize("A", [1, 2, 5])
def test_gumbel_block_round_trip(A, pred):
    r = records(A, seed=A)
    block = pack(r, pred, True)
    assert block.layout == (LAYOUT_GUMBEL | (LAYOUT_PRED if pred else 0))
    assert block.scalars.shape == (sum(L + 1 for _, _, L in EPISODES), 4 + 2 * A + int(pred))
    assert scalar_width(A, pred, True) == 4 + 2 * A + int(pred)
    got = wire(block)
    assert got.layout == block.layout and torch.equal(got.scalars, block.scalars)
    eps = unpack_episodes(got, A)
    assert len(eps) == len(EPISODES)
    for e, (i, s, L) in zip(eps, EPISODES):
        n = lambda k: r[k][i, s, :L].numpy()
        assert e["env_id"] == i and len(e["action_segment"]) == L
        assert np.array_equal(e["obs_segment"], r["frames"][i, s, :L + 1].numpy())
        assert np.array_equal(e["action_segment"], n("action").astype(np.int64))
        assert np.array_equal(e["reward_segment"], n("reward"))
        assert np.array_equal(e["visits"], n("visits").astype(np.int64))
        assert np.array_equal(e["root_value_segment"], n("value"))
        assert e["episode_return"] == float(r["ret"][i, s])
        assert ("pred_value_segment" in e) == pred
        if pred:
            assert np.array_equal(e["pred_value_segment"], n("pred"))
        assert e["improved_policy_segment"].dtype == np.float32 and e["improved_policy_segment"].shape == (L, A)
        assert np.array_equal(e["improved_policy_segment"], n("policy"))
        assert np.array_equal(e["completed_value_segment"], n("cq"))
        assert e["completed_value"] == float(np.mean(n("cq").astype(np.float64)))
    # row L of every episode: zeros but for the return
    for _, L, r0 in block.index.tolist():
        last = block.scalars[r0 + L]
        assert last[1] != 0 and torch.count_nonzero(last) == 1


def test_width_ambiguity_at_one_action():
    """A = 1, all four kinds of block (plain / Gumbel, without / with predicted values): each comes back as what it
    was packed as, because the marker says what the columns are; a marker that does not fit the width is refused,
    and only an unmarked block is read by its width"""
    r = records(1, seed=9)
    plain_pred, plain = pack(r, True, False), pack(r, False, False)
    gz, gz_pred = pack(r, False, True), pack(r, True, True)
    assert [b.scalars.shape[1] for b in (plain, plain_pred, gz, gz_pred)] == [4, 5, 6, 7]
    for b, pred, gumbel in ((plain, False, False), (plain_pred, True, False), (gz, False, True), (gz_pred, True, True)):
        e = unpack_episodes(wire(b), 1)[0]
        assert ("pred_value_segment" in e) == pred and ("improved_policy_segment" in e) == gumbel
    # a 5-wide row is [.. | pred] when marked PRED and is refused as a Gumbel row (6 or 7 wide at one action)
    relabelled = TrajBlock(plain_pred.frames, plain_pred.scalars, plain_pred.index, 1.0, LAYOUT_GUMBEL)
    with pytest.raises(ValueError):
        unpack_episodes(relabelled, 1)
    # without the marker the width rule of before holds: 5 wide = predicted values
    unmarked = TrajBlock(plain_pred.frames, plain_pred.scalars, plain_pred.index, 1.0)
    assert "pred_value_segment" in unpack_episodes(unmarked, 1)[0]
    # the width alone says nothing across action counts: two actions with predicted values are as wide as one
    # action with the Gumbel columns
    assert pack(records(2), True, False).scalars.shape[1] == gz.scalars.shape[1]


@pytest.mark.parametrize("pred", [False, True])
@pytest.mark.parametrize("A", [1, 2, 5])
def test_plain_block_bytes_unchanged(A, pred):
    """a non-Gumbel block's flat bytes, restated from the layout's description: rows of [action | reward | visits (A)
    | root value (| pred)] float32 with row L zero but for the return, frames / scalars / index back to back, each
    part on a 16-byte boundary"""
    r = records(A, seed=20 + A)
    block = pack(r, pred, False)
    W = 3 + A + int(pred)
    rows = sum(L + 1 for _, _, L in EPISODES)
    frames = np.zeros((rows, 4), np.float32)
    sc = np.zeros((rows, W), np.float32)
    index = np.zeros((len(EPISODES), 3), np.int64)
    r0 = 0
    for k, (i, s, L) in enumerate(EPISODES):
        index[k] = (i, L, r0)
        frames[r0:r0 + L + 1] = r["frames"][i, s, :L + 1].numpy()
        sc[r0:r0 + L, 0] = r["action"][i, s, :L].numpy()
        sc[r0:r0 + L, 1] = r["reward"][i, s, :L].numpy()
        sc[r0:r0 + L, 2:2 + A] = r["visits"][i, s, :L].numpy()
        sc[r0:r0 + L, 2 + A] = r["value"][i, s, :L].numpy()
        if pred:
            sc[r0:r0 + L, 3 + A] = r["pred"][i, s, :L].numpy()
        # row L: the torch restatement zeroes it by multiplying step 0's fields by 0, so a negative root value or
        # predicted value leaves -0.0 there (the device packing stores +0.0; both are the layout's zero)
        sc[r0 + L, 2 + A] = r["value"][i, s, 0].numpy() * np.float32(0)
        if pred:
            sc[r0 + L, 3 + A] = r["pred"][i, s, 0].numpy() * np.float32(0)
        sc[r0 + L, 1] = r["ret"][i, s]
        r0 += L + 1
    al = lambda n: (n + 15) // 16 * 16
    want = np.zeros(al(frames.nbytes) + al(sc.nbytes) + index.nbytes, np.uint8)
    want[:frames.nbytes] = frames.reshape(-1).view(np.uint8)
    want[al(frames.nbytes):al(frames.nbytes) + sc.nbytes] = sc.reshape(-1).view(np.uint8)
    want[al(frames.nbytes) + al(sc.nbytes):] = index.reshape(-1).view(np.uint8)
    assert np.array_equal(flatten_block(block).numpy(), want)
    e = unpack_episodes(wire(block), A)[0]
    assert "improved_policy_segment" not in e and "completed_value" not in e


# ------------------------------------------------------------------------------------------- GameSegment
def _cfg(gsl, U, TD, A):
    from lightzero_amd.policy import gumbel_policy_config
    return gumbel_policy_config(game_segment_length=gsl, num_unroll_steps=U, td_steps=TD,
                                model=dict(action_space_size=A, observation_shape=4, frame_stack_num=1))


def test_policy_config_defaults():
    from lightzero_amd.policy import gumbel_policy_config, policy_config
    cfg = gumbel_policy_config()
    assert cfg.type == 'gumbel_muzero' and cfg.gumbel_algo is True and cfg.max_num_considered_actions == 4
    assert policy_config().gumbel_algo is False and 'max_num_considered_actions' not in policy_config()


def test_from_arrays_takes_improved_policies():
    from lightzero_amd.game_segment import GameSegment
    cfg = _cfg(3, 1, 1, 2)
    pol = np.arange(8, dtype=np.float32).reshape(4, 2)
    z = np.zeros
    seg = GameSegment.from_arrays(SimpleNamespace(n=2), 3, cfg, z((4, 4), np.float32), z(3, np.int64), z(3), z((3, 2)),
                                  z(3), np.ones((3, 2), np.int8), np.full(3, -1), improved_policy=pol)
    assert np.array_equal(seg.improved_policy_probs, pol)
    seg = GameSegment.from_arrays(SimpleNamespace(n=2), 3, cfg, z((4, 4), np.float32), z(3, np.int64), z(3), z((3, 2)),
                                  z(3), np.ones((3, 2), np.int8), np.full(3, -1))
    assert seg.improved_policy_probs.shape == (0,)


def test_segment_cut_and_pad_over_carry_improved_policies():
    """game_segment_length 3, num_unroll_steps + td_steps = 2, an episode of 7 steps: segments [0, 3), [3, 6), [6, 7).
    The first is padded with the second's first two policies, the second (padded at the episode's end with the
    third, which holds one step) with that one policy, the third is saved unpadded — and the host loop's
    store_search_stats / pad_over build the same arrays."""
    from lightzero_amd.game_segment import GameSegment
    from lightzero_amd.worker.segments import episode_segments
    A, L = 2, 7
    cfg = _cfg(3, 1, 1, A)
    rng = np.random.default_rng(3)
    pol = rng.random((L, A)).astype(np.float32)
    obs = rng.random((L + 1, 4)).astype(np.float32)
    visits = rng.integers(1, 5, (L, A))
    out = episode_segments(cfg, SimpleNamespace(n=A), obs, np.zeros(L, np.int64), np.ones(L), visits,
                           np.zeros(L, np.float32), None, 0, np.ones(A, np.int8), -1, improved_policy=pol)
    segs = [s for _, _, s, _, _ in out]
    want = [np.concatenate([pol[0:3], pol[3:5]]), np.concatenate([pol[3:6], pol[6:7]]), pol[6:7]]
    assert len(segs) == 3
    for s, w in zip(segs, want):
        assert np.array_equal(s.improved_policy_probs, w)
        assert len(s.improved_policy_probs) == len(s.root_value_segment)  # cut and padded like the root values
    # the host loop's way: store_search_stats + append per step, pad_over at the rollover
    host, cur, last = [], GameSegment(SimpleNamespace(n=A), 3, cfg), None
    cur.reset([obs[0]])
    U, TD = 1, 1

    def pad_and_save(last, cur):
        last.pad_over(cur.obs_segment[1:1 + U], cur.reward_segment[:U + TD - 1], cur.root_value_segment[:U + TD],
                      cur.child_visit_segment[:U], next_segment_improved_policy=cur.improved_policy_probs[:U + TD])
        last.game_segment_to_array()
        host.append(last)

    for t in range(L):
        cur.store_search_stats(visits[t].tolist(), 0.0, improved_policy=pol[t])
        cur.append(0, obs[t + 1], 1.0, np.ones(A, np.int8), -1)
        if cur.is_full():
            if last is not None:
                pad_and_save(last, cur)
            last, cur = cur, GameSegment(SimpleNamespace(n=A), 3, cfg)
            cur.reset([obs[t + 1]])
    pad_and_save(last, cur)
    cur.game_segment_to_array()
    host.append(cur)
    for s, w in zip(host, want):
        assert np.array_equal(np.asarray(s.improved_policy_probs), w)
    # without policies the segments end with the empty array, as before
    plain = episode_segments(cfg, SimpleNamespace(n=A), obs, np.zeros(L, np.int64), np.ones(L), visits,
                             np.zeros(L, np.float32), None, 0, np.ones(A, np.int8), -1)
    assert all(s.improved_policy_probs.shape == (0,) for _, _, s, _, _ in plain)


# ------------------------------------------------------------------------------------------- the policy's draws
class _StubRoots:
    def __init__(self, n, legal):
        self.n, self.legal, self.prepared = n, legal, None

    def prepare(self, noise_weight, noises, rewards, values, logits, to_play):
        assert [len(x) for x in noises] == [len(l) for l in self.legal] and len(values) == self.n
        self.prepared = "noise"

    def prepare_no_noise(self, rewards, values, logits, to_play):
        self.prepared = "no_noise"

    def get_distributions(self):
        return [[3 + j for j in range(len(l))] for l in self.legal]

    def get_values(self):
        return [0.5] * self.n

    def get_children_values(self, disc, A):
        return [[1.0 if a in l else float("-inf") for a in range(A)] for l in self.legal]

    def get_policies(self, disc, A):
        return [[(1.0 + a) / sum(1.0 + b for b in l) if a in l else 0.0 for a in range(A)] for l in self.legal]

    def clear(self):
        pass


def _stub_policy(A, masks):
    from lightzero_amd.policy import GumbelMuZeroCollectPolicy, gumbel_policy_config
    n = len(masks)
    model = SimpleNamespace(eval=lambda: None, initial_inference=lambda d: SimpleNamespace(
        latent_state=torch.zeros(n, 8), reward=[0.0] * n, value=torch.zeros(n, 21), policy_logits=torch.zeros(n, A)))
    cfg = gumbel_policy_config(device='cpu', num_simulations=4, model=dict(action_space_size=A, support_scale=10))
    pol = GumbelMuZeroCollectPolicy(cfg, model)
    pol.inverse_scalar_transform_handle = lambda v: torch.zeros(v.shape[0], 1)
    made = []
    pol._roots = lambda k, legal: made.append(_StubRoots(k, legal)) or made[-1]
    stub = SimpleNamespace(record=False, last_record=None, search=lambda *a, **k: None)
    pol._mcts_collect = pol._mcts_eval = stub
    return pol, made


def test_policy_numpy_stream_order():
    """after np.random.seed(s) a collect forward over three envs with ragged masks leaves numpy's generator where
    three dirichlet draws (sizes: the legal counts) followed by three choice draws leave it; the eval forward draws
    nothing"""
    A = 4
    masks = [np.array(m) for m in ([1, 1, 1, 1], [0, 1, 1, 0], [1, 0, 1, 1])]
    pol, made = _stub_policy(A, masks)
    data = torch.zeros(3, 4)
    np.random.seed(1234)
    out = pol.forward(data, masks, temperature=1.0, to_play=[-1] * 3)
    after = np.random.rand()
    assert made[-1].prepared == "noise"
    np.random.seed(1234)
    for m in masks:
        np.random.dirichlet([0.3] * int(m.sum()))
    for m in masks:
        d = np.array([3.0 + j for j in range(int(m.sum()))])
        np.random.choice(len(d), p=(d / d.sum()).tolist())
    assert after == np.random.rand()
    keys = ['action', 'visit_count_distributions', 'visit_count_distribution_entropy', 'searched_value',
            'roots_completed_value', 'improved_policy_probs', 'predicted_value', 'predicted_policy_logits']
    assert list(out[0].keys()) == keys
    # the action: the first maximum of the masked improved policy, an id of the whole action space
    assert [int(out[i]['action']) for i in range(3)] == [3, 2, 3]
    assert np.array_equal(out[1]['roots_completed_value'], [0.0, 1.0, 1.0, 0.0])
    np.random.seed(99)
    want = np.random.rand()
    np.random.seed(99)
    ev = pol.eval_mode.forward(data, masks, to_play=[-1] * 3)
    assert np.random.rand() == want and made[-1].prepared == "no_noise"
    assert list(ev[0].keys()) == [k for k in keys if k not in ('roots_completed_value', 'improved_policy_probs')]
