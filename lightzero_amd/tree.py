"""DeviceTree: one lzm_handle (a batch of search trees resident in HBM) plus its result buffers.

Host-side owner of the structures the reference keeps in ``CRoots`` + ``CSearchResults``
(/root/reference/lzero/mcts/ctree/ctree_muzero/lib/cnode.h:48-79). All tensors are on the GPU;
every method enqueues work on the current torch stream and never synchronises.
"""
import ctypes
import itertools
import threading
import time

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

# ----------------------------------------------------------------------------- seeds
_seed_lock = threading.Lock()
_seed_source = None


def reference_time_seed():
    """The reference seeds every batch_traverse with gettimeofday().tv_usec (common_lib/utils.cpp:25)."""
    return int(time.time_ns() // 1000 % 1000000)


def set_seed_source(fn):
    """Install a callable returning the next traverse seed (None restores the time seed)."""
    global _seed_source
    with _seed_lock:
        _seed_source = fn


def next_seed():
    with _seed_lock:
        fn = _seed_source
    return int(fn() if fn is not None else reference_time_seed()) & 0xFFFFFFFF


class SequentialSeeds:
    """Deterministic seed source: usec_k = (1000003*seed + k) mod 1e6."""

    def __init__(self, seed):
        self.seed, self.k = int(seed), 0

    def __call__(self):
        v = (1000003 * self.seed + self.k) % 1000000
        self.k += 1
        return v


# ----------------------------------------------------------------------------- handle
_uids = itertools.count(1)


def _rec_ptrs(rec, names=("x", "action", "search_len", "decoded", "policy_logits")):
    """the one-launch searches' record outputs: device pointers of a _Recorder-like object's buffers, NULL
    without one (or without that buffer)"""
    return [None if rec is None else ptr(getattr(rec, n, None)) for n in names]


class DeviceTree:
    def __init__(self, num_roots, action_space, max_sims=64, ez=False, fast_rng=False, device=None, gumbel=False):
        """gumbel: a Gumbel MuZero tree (LZM_TREE_GUMBEL; ctree_gumbel_muzero), driven by the gumbel_* methods"""
        _lib.require_gpu()
        if gumbel and ez:
            raise ValueError("DeviceTree: gumbel and ez are mutually exclusive")
        self.uid = next(_uids)  # never reused (a handle address can be, after lzm_destroy)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.B, self.A = int(num_roots), int(action_space)
        self.ez, self.fast_rng, self.gumbel = bool(ez), bool(fast_rng), bool(gumbel)
        flags = ((_lib.LZM_TREE_EZ if ez else 0) | (_lib.LZM_RNG_FAST if fast_rng else 0)
                 | (_lib.LZM_TREE_GUMBEL if gumbel else 0))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            call("lzm_create", self.B, self.A, int(max_sims), flags, ctypes.byref(h))
        self.h = h
        _lib.register_owner(self)  # closed at exit before the runtime's own teardown
        self.generation = 0
        self._pb_c = (19652, 1.25)  # lzm_create builds the table for the reference defaults
        i32 = dict(dtype=torch.int32, device=self.device)
        B = self.B
        self.x = torch.zeros(B, **i32)
        self.y = torch.zeros(B, **i32)
        self.action = torch.zeros(B, **i32)
        self.action64 = torch.zeros(B, dtype=torch.int64, device=self.device)
        self.vtp = torch.zeros(B, **i32)
        self.search_len = torch.zeros(B, **i32)
        self.is_reset = torch.zeros(B, **i32)
        self.seed_buf = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._unchecked = False  # a search ran whose error words no getter has checked yet

    def searched(self):
        """mark that a search (or traverse) ran: the next result getter checks the error words once"""
        self._unchecked = True

    def check_once(self):
        """check_errors(clear=True) once per search, by whichever result getter runs first: raises
        LzmError when the search's tie-break stream broke (the words are cleared as they are read, so a
        pooled tree never carries them into the next owner's searches)"""
        if self._unchecked:
            self._unchecked = False
            self.check_errors(clear=True)

    def reset_errors(self, stream=None):
        """zero the sticky error words without raising (a recycled handle starts clean); synchronises"""
        out = (ctypes.c_int32 * _lib.LZM_ERR_WORDS)()
        _lib.load().lzm_check_errors(self.h, out, 1, stream_ptr(stream))
        self._unchecked = False

    @property
    def sims_capacity(self):
        return _lib.load().lzm_sims_capacity(self.h)

    def reserve(self, max_sims):
        if max_sims > self.sims_capacity:
            with torch.cuda.device(self.device):
                call("lzm_reserve", self.h, int(max_sims))
            self.generation += 1  # device buffers moved: captured graphs are stale

    def set_pb_c(self, pb_c_base, pb_c_init):
        key = (int(pb_c_base), float(np.float32(pb_c_init)))
        if key != self._pb_c:
            with torch.cuda.device(self.device):
                call("lzm_set_pb_c", self.h, key[0], key[1])
            self._pb_c = key

    def copy_roots_from(self, other, stream=None):
        call("lzm_copy_tree", self.h, other.h, stream_ptr(stream))

    def close(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                _lib.load().lzm_destroy(h)
            except Exception:  # interpreter shutdown
                pass
        self.h = None

    def __del__(self):
        self.close()

    # -- calls ---------------------------------------------------------------------------
    def prepare(self, legal, count, noises, noise_weight, rewards, logits, to_play, stream=None):
        call("lzm_roots_prepare", self.h, ptr(legal), ptr(count), ptr(noises), float(noise_weight), ptr(rewards),
             ptr(logits), ptr(to_play), stream_ptr(stream))

    def set_norm_words(self, words=None):
        """int32 device [2 * ceil(B / 2)] ensure_softmax verdict words that the step's head kernel
        writes (lzm_conv_heads); decode_backprop then skips its own check. None restores it."""
        self._norm_words = words
        call("lzm_set_norm_words", self.h, ptr(words))

    def set_reuse(self, true_action=None, reuse_value=None):
        """ReZero search-with-reuse inputs for the following traverse / backprop calls (device int32 /
        float32 [B]; None clears). The tensors are kept alive here: the handle keeps their pointers."""
        if true_action is None:
            self._reuse = None
            call("lzm_set_reuse", self.h, None, None)
            return
        ta = true_action.to(device=self.device, dtype=torch.int32).reshape(self.B).contiguous()
        rv = reuse_value.to(device=self.device, dtype=torch.float32).reshape(self.B).contiguous()
        self._reuse = (ta, rv)
        call("lzm_set_reuse", self.h, ptr(ta), ptr(rv))

    def traverse(self, minmax, seed, vtp_in, pb_c_base=19652, pb_c_init=1.25, discount=0.997, stream=None):
        """seed: 1-element device tensor (int32/uint32 bits)."""
        self._unchecked = True
        call("lzm_traverse", self.h, int(pb_c_base), float(pb_c_init), float(discount), ptr(minmax), ptr(seed),
             ptr(vtp_in), ptr(self.x), ptr(self.y), ptr(self.action), ptr(self.action64), ptr(self.vtp),
             ptr(self.search_len), stream_ptr(stream))

    def gather(self, pool, row_elems, out, stream=None):
        call("lzm_gather_latent", self.h, ptr(pool), int(row_elems), ptr(self.x), ptr(out), stream_ptr(stream))

    def backprop(self, cur, discount, minmax, rewards, values, logits, to_play, is_reset=None, stream=None):
        call("lzm_backprop", self.h, int(cur), float(discount), ptr(minmax), ptr(rewards), ptr(values), ptr(logits),
             ptr(to_play), ptr(is_reset), stream_ptr(stream))

    def _value_support(self, Vv, V):
        """the value rows' length for the decode when it differs from the reward rows' (lzm_set_value_support;
        host state, set only when it changes)"""
        want = 0 if Vv == V else int(Vv)
        if want != getattr(self, "_vsupport", 0):
            call("lzm_set_value_support", self.h, want)
            self._vsupport = want

    def decode_backprop(self, cur, discount, minmax, reward_logits, value_logits, categorical, policy_logits, to_play,
                        lstm_horizon=0, out_is_reset=None, next_latent=None, pool_slot=None, row_elems=0,
                        out_decoded=None, stream=None):
        V = reward_logits.shape[-1] if categorical else 1
        self._value_support(value_logits.shape[-1] if categorical else 1, V)
        call("lzm_decode_backprop", self.h, int(cur), float(discount), ptr(minmax), ptr(reward_logits),
             ptr(value_logits), int(V), int(bool(categorical)), ptr(policy_logits), ptr(to_play), int(lstm_horizon),
             ptr(out_is_reset), ptr(next_latent), ptr(pool_slot), int(row_elems), ptr(out_decoded), stream_ptr(stream))

    def decode_backprop_traverse(self, cur, discount, minmax, reward_logits, value_logits, categorical, policy_logits,
                                 to_play, seed, vtp_in, pb_c_base=19652, pb_c_init=1.25, lstm_horizon=0,
                                 out_is_reset=None, next_latent=None, pool_slot=None, row_elems=0, out_decoded=None,
                                 stream=None):
        """decode_backprop of simulation `cur` and the traverse of the next one in one launch (parity
        mode); the traverse outputs overwrite x / y / action / vtp / search_len."""
        V = reward_logits.shape[-1] if categorical else 1
        self._value_support(value_logits.shape[-1] if categorical else 1, V)
        call("lzm_decode_backprop_traverse", self.h, int(cur), float(discount), ptr(minmax), ptr(reward_logits),
             ptr(value_logits), int(V), int(bool(categorical)), ptr(policy_logits), ptr(to_play), int(lstm_horizon),
             ptr(out_is_reset), ptr(next_latent), ptr(pool_slot), int(row_elems), ptr(out_decoded), int(pb_c_base),
             float(pb_c_init), ptr(seed), ptr(vtp_in), ptr(self.x), ptr(self.y), ptr(self.action), ptr(self.action64),
             ptr(self.vtp), ptr(self.search_len), stream_ptr(stream))

    # -- Gumbel MuZero trees (lzm_gumbel_*; LzmError on any other tree, nothing launched) --------------
    def set_considered(self, num_simulations, max_num_considered_actions):
        """the device considered-visits row for (S, m), built now (a synchronous copy: outside graph capture);
        a change retires captured graphs (generation)"""
        key = (int(num_simulations), int(max_num_considered_actions))
        if key != getattr(self, "_considered", None):
            with torch.cuda.device(self.device):
                call("lzm_gumbel_set_considered", self.h, *key)
            if getattr(self, "_considered", None) is not None:
                self.generation += 1
            self._considered = key

    def set_root_values(self, values, stream=None):
        """the roots' raw_value (the value pool of Roots.prepare, gmz_tree.pyx:36-40): float32 device [B],
        after prepare"""
        call("lzm_gumbel_set_root_values", self.h, ptr(values), stream_ptr(stream))

    def gumbel_traverse(self, num_simulations, max_num_considered_actions, discount, vtp_in, stream=None):
        call("lzm_gumbel_traverse", self.h, int(num_simulations), int(max_num_considered_actions), float(discount),
             ptr(vtp_in), ptr(self.x), ptr(self.y), ptr(self.action), ptr(self.action64), ptr(self.vtp),
             ptr(self.search_len), stream_ptr(stream))
        self._considered = (int(num_simulations), int(max_num_considered_actions))

    def gumbel_backprop(self, cur, discount, minmax, rewards, values, logits, to_play, stream=None):
        call("lzm_gumbel_backprop", self.h, int(cur), float(discount), ptr(minmax), ptr(rewards), ptr(values),
             ptr(logits), ptr(to_play), stream_ptr(stream))

    def gumbel_decode_backprop(self, cur, discount, minmax, reward_logits, value_logits, categorical, policy_logits,
                               to_play, next_latent=None, pool_slot=None, row_elems=0, out_decoded=None, stream=None):
        V = reward_logits.shape[-1] if categorical else 1
        self._value_support(value_logits.shape[-1] if categorical else 1, V)
        call("lzm_gumbel_decode_backprop", self.h, int(cur), float(discount), ptr(minmax), ptr(reward_logits),
             ptr(value_logits), int(V), int(bool(categorical)), ptr(policy_logits), ptr(to_play), ptr(next_latent),
             ptr(pool_slot), int(row_elems), ptr(out_decoded), stream_ptr(stream))

    def gumbel_decode_backprop_traverse(self, cur, discount, minmax, reward_logits, value_logits, categorical,
                                        policy_logits, to_play, num_simulations, max_num_considered_actions, vtp_in,
                                        next_latent=None, pool_slot=None, row_elems=0, out_decoded=None, stream=None):
        """gumbel_decode_backprop of simulation `cur` and the traverse of the next one in one launch; the traverse
        outputs overwrite x / y / action / vtp / search_len."""
        V = reward_logits.shape[-1] if categorical else 1
        self._value_support(value_logits.shape[-1] if categorical else 1, V)
        call("lzm_gumbel_decode_backprop_traverse", self.h, int(cur), float(discount), ptr(minmax),
             ptr(reward_logits), ptr(value_logits), int(V), int(bool(categorical)), ptr(policy_logits), ptr(to_play),
             ptr(next_latent), ptr(pool_slot), int(row_elems), ptr(out_decoded), int(num_simulations),
             int(max_num_considered_actions), ptr(vtp_in), ptr(self.x), ptr(self.y), ptr(self.action),
             ptr(self.action64), ptr(self.vtp), ptr(self.search_len), stream_ptr(stream))

    def children_values(self, discount, stream=None):
        """Roots.get_children_values: float32 [B, A], the completed Q in action order, -inf where illegal"""
        out = torch.empty((self.B, self.A), dtype=torch.float32, device=self.device)
        call("lzm_gumbel_get_children_values", self.h, float(discount), ptr(out), stream_ptr(stream))
        return out

    def policies(self, discount, stream=None):
        """Roots.get_policies: float32 [B, A], the improved policy, exactly 0 where illegal"""
        out = torch.empty((self.B, self.A), dtype=torch.float32, device=self.device)
        call("lzm_gumbel_get_policies", self.h, float(discount), ptr(out), stream_ptr(stream))
        return out

    def collect_outputs(self, discount, out=None, count=None, stream=None):
        """The roots' outputs a Gumbel collect step reads, in one launch (lzm_gumbel_collect_outputs): dict of
        distributions int32 [B, A] (legal order, -1 past the legal count), values [B], completed_q [B, A] (action
        order, 0 where illegal), improved_policy [B, A] and action int32 [B] (the first maximum of the policy row);
        `out`: such a dict to write into; count: the int64 device step counter to advance by 1."""
        if out is None:
            f32, i32 = dict(dtype=torch.float32, device=self.device), dict(dtype=torch.int32, device=self.device)
            out = dict(distributions=torch.empty((self.B, self.A), **i32), values=torch.empty(self.B, **f32),
                       completed_q=torch.empty((self.B, self.A), **f32),
                       improved_policy=torch.empty((self.B, self.A), **f32), action=torch.empty(self.B, **i32))
        call("lzm_gumbel_collect_outputs", self.h, float(discount), ptr(out["distributions"]), ptr(out["values"]),
             ptr(out["completed_q"]), ptr(out["improved_policy"]), ptr(out["action"]), ptr(count), stream_ptr(stream))
        return out

    def search_mlp_gumbel(self, dims, weights, S, m, minmax, vtp_in, pool, discount=0.997, rec=None, stream=None):
        """One launch for the whole Gumbel MuZero search of a MuZeroModelMLP (lzm_search_mlp_gumbel; dims /
        weights: the packed network in the kernel layout, as search_mlp's); m: max_num_considered_actions;
        rec: optional _Recorder-like object (its vtp rows are the caller's: to_play passes through)."""
        self._unchecked = True
        with torch.cuda.device(self.device):  # (a changed (S, m) rebuilds the considered-visits row)
            call("lzm_search_mlp_gumbel", self.h, dims["hidden"], dims["head_hidden"], dims["support"],
                 int(dims["res"]), ptr(weights), int(S), int(m), float(discount), ptr(minmax), ptr(vtp_in), ptr(pool),
                 *_rec_ptrs(rec), stream_ptr(stream))
        self._considered = (int(S), int(m))

    def search_mlp_gumbel_plan(self, dims, S):
        """What search_mlp_gumbel(dims, ..., S) launches on this handle as it stands (lzm_search_mlp_gumbel_plan;
        host only): dict(roots_per_wg, kernel 'streaming' / None when the kernel refuses the shape, its LDS need
        or a handle that is no Gumbel tree, mode 0, tree_in_lds)."""
        out = (ctypes.c_int32 * 4)()
        call("lzm_search_mlp_gumbel_plan", self.h, int(S), dims["hidden"], dims["head_hidden"], dims["support"],
             int(dims["res"]), out)
        return dict(roots_per_wg=out[0], kernel={0: "streaming"}.get(out[1]), mode=out[2], tree_in_lds=bool(out[3]))

    def search_conv_gumbel(self, net, S, m, minmax, vtp_in, pool, discount=0.997, categorical=True, rec=None,
                           max_roots=0, stream=None):
        """One launch per root slice for the whole Gumbel MuZero search of a conv MuZeroModel
        (lzm_search_conv_gumbel; net: a native split-precision conv_infer.FoldedConvNet, as search_conv's);
        m: max_num_considered_actions; max_roots: a cap on the slice (0: the library's 1,024); rec: optional
        _Recorder-like object (its vtp rows are the caller's: to_play passes through)."""
        hp = net.heads
        self._unchecked = True
        with torch.cuda.device(self.device):  # (a changed (S, m) rebuilds the considered-visits row)
            call("lzm_search_conv_gumbel", self.h, int(S), int(m), float(discount), ptr(minmax), ptr(vtp_in),
                 ptr(pool), ptr(net.native), ptr(net.actmap), int(net.n_dres), int(net.n_pres), int(net.r_ch),
                 int(net.h_ch), ptr(hp["w1t"]), ptr(hp["b1"]), ptr(hp["w2q"]), ptr(hp["b2"]), int(hp["Kr"]),
                 int(hp["Khd"]), int(hp["off_policy"]), int(hp["Vr"]), int(hp["Vv"]), int(bool(categorical)),
                 *_rec_ptrs(rec), int(max_roots), stream_ptr(stream))
        self._considered = (int(S), int(m))

    def search_conv_gumbel_plan(self, net, S, categorical=True, max_roots=0):
        """What search_conv_gumbel(net, S, ..., max_roots=max_roots) launches on this handle as it stands
        (lzm_search_conv_gumbel_plan: the launch's own decision; host only, nothing is launched):
        search_conv_sliced_plan's dict — supported, code, reason, workgroups (of the largest slice), lds_bytes
        (the raw_value slice and the Gumbel tables included), pinned, out_rounds, slices, slice_roots,
        last_slice_roots."""
        hp = net.heads
        out = (ctypes.c_int32 * 11)()
        call("lzm_search_conv_gumbel_plan", self.h, int(S), int(net.n_dres), int(net.n_pres), int(net.r_ch),
             int(net.h_ch), int(hp["Kr"]), int(hp["Khd"]), int(hp["off_policy"]), int(hp["Vr"]), int(hp["Vv"]),
             int(bool(categorical)), int(max_roots), out)
        reason = None if out[0] == 0 else _lib.load().lzm_last_error().decode()
        return dict(supported=out[0] == 0, code=out[0], reason=reason, workgroups=out[1], lstm_tiles=out[2],
                    lds_bytes=out[3], pinned=out[4], pbt_rows=out[5], out_rounds=out[6], out_one_round=False,
                    reward_one_round=bool(out[7]), slices=out[8], slice_roots=out[9], last_slice_roots=out[10])

    def search_mlp(self, dims, weights, S, minmax, seeds, vtp_in, pool, pb_c_base=19652, pb_c_init=1.25,
                   discount=0.997, rec=None, stream=None):
        """One launch for the whole search (lzm_search_mlp); rec: optional _Recorder-like object."""
        self._unchecked = True
        call("lzm_search_mlp", self.h, dims["hidden"], dims["head_hidden"], dims["support"], int(dims["res"]),
             ptr(weights), int(S), int(pb_c_base), float(pb_c_init), float(discount), ptr(minmax), ptr(seeds),
             ptr(vtp_in), ptr(pool), *_rec_ptrs(rec), stream_ptr(stream))

    def search_mlp_plan(self, dims, S):
        """What search_mlp(dims, ..., S) launches on this handle as it stands (lzm_search_mlp_plan; host
        only): dict(roots_per_wg, kernel 'resident' / 'streaming' / None when the kernels refuse the
        shape, mode: the resident kernel's selection mode, tree_in_lds)."""
        out = (ctypes.c_int32 * 4)()
        call("lzm_search_mlp_plan", self.h, int(S), dims["hidden"], dims["head_hidden"], dims["support"],
             int(dims["res"]), out)
        return dict(roots_per_wg=out[0], kernel={1: "resident", 0: "streaming"}.get(out[1]), mode=out[2],
                    tree_in_lds=bool(out[3]))

    def search_mlp_ez(self, dims, weights, S, minmax, seeds, vtp_in, pool, hpool, cpool, horizon, pb_c_base=19652,
                      pb_c_init=1.25, discount=0.997, rec=None, stream=None):
        """One launch for the whole search of an EfficientZeroModelMLP (lzm_search_mlp_ez; dims / weights:
        fused.pack_efficientzero_mlp's, in the kernel layout); hpool / cpool: the LSTM state pools
        [S + 1, B, lstm_hidden] with slot 0 = the roots' state; rec: optional _Recorder-like object (with
        is_reset)."""
        self._unchecked = True
        rx, ra, rl, rd, rg = _rec_ptrs(rec)
        call("lzm_search_mlp_ez", self.h, dims["hidden"], dims["lstm_hidden"], dims["head_hidden"], dims["support"],
             int(dims["res"]), ptr(weights), int(S), int(horizon), int(pb_c_base), float(pb_c_init), float(discount),
             ptr(minmax), ptr(seeds), ptr(vtp_in), ptr(pool), ptr(hpool), ptr(cpool), rx, ra, rl,
             *_rec_ptrs(rec, ("is_reset",)), rd, rg, stream_ptr(stream))

    def search_mlp_ez_plan(self, dims, S):
        """What search_mlp_ez(dims, ..., S) launches on this handle as it stands (lzm_search_mlp_ez_plan; host
        only): dict(roots_per_wg, kernel 'streaming' / None when the kernel refuses the shape, its LDS need or
        a MuZero tree, mode 0, tree_in_lds)."""
        out = (ctypes.c_int32 * 4)()
        call("lzm_search_mlp_ez_plan", self.h, int(S), dims["hidden"], dims["lstm_hidden"], dims["head_hidden"],
             dims["support"], int(dims["res"]), out)
        return dict(roots_per_wg=out[0], kernel={0: "streaming"}.get(out[1]), mode=out[2], tree_in_lds=bool(out[3]))

    def _conv_plan(self, name, n_out, net, S, H, horizon, categorical, *cap):
        """the two conv plan queries' call (cap: the sliced query's max_roots) and their dict"""
        hp = net.heads
        out = (ctypes.c_int32 * n_out)()
        call(name, self.h, int(S), int(self.ez), int(H), int(horizon), int(net.n_dres), int(net.n_pres),
             int(net.r_ch), int(net.h_ch), int(hp["Kr"]), int(hp["Khd"]), int(hp["off_policy"]), int(hp["Vr"]),
             int(hp["Vv"]), int(bool(categorical)), *cap, out)
        reason = None if out[0] == 0 else _lib.load().lzm_last_error().decode()
        return out, dict(supported=out[0] == 0, code=out[0], reason=reason, workgroups=out[1], lstm_tiles=out[2],
                         lds_bytes=out[3], pinned=out[4], pbt_rows=out[5], out_rounds=out[6],
                         out_one_round=bool(self.ez and out[6] == 0), reward_one_round=bool(out[7]))

    def search_conv_plan(self, net, S, H=0, horizon=1, categorical=True):
        """What search_conv (MuZero trees) / search_conv_ez (EfficientZero trees; H: the LSTM width, horizon:
        lstm_horizon_len) launches for the native FoldedConvNet `net` and S simulations on this handle as the
        process stands (lzm_search_conv_plan: the launches' own decision; host only, nothing is launched):
        dict(supported, code: the launch's return code (0 runs, _lib.LZM_ERR_RESIDENCY the EfficientZero grid
        cannot be co-resident), reason: the library's message when refused, workgroups, lstm_tiles, lds_bytes,
        pinned: head half-heads kept in LDS, pbt_rows: pb_c table rows in LDS (0: the walk divides),
        out_rounds: rounds of 768 output columns (MuZero: Vr + Vv + A; EfficientZero: Vv + A, 0 when
        out_one_round), out_one_round / reward_one_round: EfficientZero's one-column-per-thread forms of the
        value | policy and the reward output (up to 256 columns))."""
        return self._conv_plan("lzm_search_conv_plan", 8, net, S, H, horizon, categorical)[1]

    def search_conv_sliced_plan(self, net, S, H=0, horizon=1, categorical=True, max_roots=0):
        """search_conv_plan for search_conv_sliced / search_conv_ez_sliced with the same max_roots
        (lzm_search_conv_sliced_plan; host only, nothing is launched): search_conv_plan's fields for the largest
        slice, plus slices, slice_roots (roots per slice) and last_slice_roots (all 0 when refused). A batch that
        fits one slice gets search_conv_plan's own answer with slices = 1."""
        out, plan = self._conv_plan("lzm_search_conv_sliced_plan", 11, net, S, H, horizon, categorical, int(max_roots))
        return dict(plan, slices=out[8], slice_roots=out[9], last_slice_roots=out[10])

    def _search_conv(self, name, net, S, minmax, seeds, vtp_in, pool, pb_c_base, pb_c_init, discount, categorical, rec,
                     stream, lstm=None, max_roots=None):
        """the four one-launch conv searches' call. lstm: (hpool, cpool, horizon) for the EfficientZero entry
        points, which take the LSTM state and weights and the is_reset record and no Kr; max_roots: the sliced
        entry points' cap"""
        hp = net.heads
        state, gates, kr, reset = [], [], [int(hp["Kr"])], []
        if lstm is not None:
            hpool, cpool, horizon = lstm
            state = [ptr(hpool), ptr(cpool), int(hpool.shape[2]), int(horizon)]
            gates = [ptr(net.lstm_frag), ptr(net.t["lstm_b"]), ptr(net.t["vp_s"]), ptr(net.t["vp_t"])]
            kr, reset = [], _rec_ptrs(rec, ("is_reset",))
        cap = [] if max_roots is None else [int(max_roots)]
        self._unchecked = True
        call(name, self.h, int(S), int(pb_c_base), float(pb_c_init), float(discount), ptr(minmax), ptr(seeds),
             ptr(vtp_in), ptr(pool), *state, ptr(net.native), ptr(net.actmap), int(net.n_dres), int(net.n_pres),
             int(net.r_ch), int(net.h_ch), *gates, ptr(hp["w1t"]), ptr(hp["b1"]), ptr(hp["w2q"]), ptr(hp["b2"]), *kr,
             int(hp["Khd"]), int(hp["off_policy"]), int(hp["Vr"]), int(hp["Vv"]), int(bool(categorical)),
             *_rec_ptrs(rec), *reset, *cap, stream_ptr(stream))

    def search_conv_sliced(self, net, S, minmax, seeds, vtp_in, pool, pb_c_base=19652, pb_c_init=1.25,
                           discount=0.997, categorical=True, rec=None, max_roots=0, stream=None):
        """search_conv over root slices (lzm_search_conv_sliced): any number of roots, one launch per slice of
        up to min(1024, max_roots or 1024) roots, enqueued here one after another; the same results."""
        self._search_conv("lzm_search_conv_sliced", net, S, minmax, seeds, vtp_in, pool, pb_c_base, pb_c_init,
                          discount, categorical, rec, stream, max_roots=max_roots)

    def search_conv_ez_sliced(self, net, S, minmax, seeds, vtp_in, pool, hpool, cpool, horizon, pb_c_base=19652,
                              pb_c_init=1.25, discount=0.997, categorical=True, rec=None, max_roots=0, stream=None):
        """search_conv_ez over root slices (lzm_search_conv_ez_sliced): batches past 256 roots or past the
        co-resident grid, one launch per slice (whole blocks of 64 roots, each grid co-resident on its own),
        enqueued here one after another; the same results. ResidencyError when not even 64 roots fit."""
        self._search_conv("lzm_search_conv_ez_sliced", net, S, minmax, seeds, vtp_in, pool, pb_c_base, pb_c_init,
                          discount, categorical, rec, stream, lstm=(hpool, cpool, horizon), max_roots=max_roots)

    def search_conv(self, net, S, minmax, seeds, vtp_in, pool, pb_c_base=19652, pb_c_init=1.25, discount=0.997,
                    categorical=True, rec=None, stream=None):
        """One launch for the whole search of a conv MuZeroModel (lzm_search_conv; net: a native
        split-precision conv_infer.FoldedConvNet); rec: optional _Recorder-like object."""
        self._search_conv("lzm_search_conv", net, S, minmax, seeds, vtp_in, pool, pb_c_base, pb_c_init, discount,
                          categorical, rec, stream)

    def search_conv_ez(self, net, S, minmax, seeds, vtp_in, pool, hpool, cpool, horizon, pb_c_base=19652,
                       pb_c_init=1.25, discount=0.997, categorical=True, rec=None, stream=None):
        """One launch for the whole search of a conv EfficientZeroModel (lzm_search_conv_ez; net: a native
        split-precision conv_infer.FoldedConvNet with the fused LSTM step packed); hpool / cpool: the LSTM
        state pools [S + 1, B, H] with slot 0 = the roots' state; rec: optional _Recorder-like object
        (with is_reset)."""
        self._search_conv("lzm_search_conv_ez", net, S, minmax, seeds, vtp_in, pool, pb_c_base, pb_c_init, discount,
                          categorical, rec, stream, lstm=(hpool, cpool, horizon))

    def set_step(self, count=None, base=0, increment=True, dist=None, values=None, fresh_minmax=False,
                 value_delta_max=0.0):
        """Collect-step mode of the next search_mlp calls (lzm_search_set_step; host state only):
        device seeds from the int64 step counter `count` (incremented by the search if
        `increment`), root outputs into `dist` / `values`, fresh min-max bounds. set_step() clears
        it."""
        call("lzm_search_set_step", self.h, ptr(count), int(base), int(bool(increment)), ptr(dist), ptr(values),
             int(bool(fresh_minmax)), float(np.float32(value_delta_max)))

    def error_word(self, i):
        """device address (ctypes) of sticky error word i, for kernels launched outside the handle"""
        return ctypes.c_void_p(_lib.load().lzm_error_word(self.h, int(i)))

    def check_errors(self, clear=True, stream=None):
        """Post-search integrity check (synchronises the stream): raises LzmError when a look-back
        spin timed out or a draw fell outside the coefficient table on any search path of this
        handle, i.e. when the parity-mode tie-break stream may differ from the reference's, and
        SplitRangeError when a split-fp16 network value was non-finite or out of range (word 4).
        Returns the counters otherwise (all zero)."""
        out = (ctypes.c_int32 * _lib.LZM_ERR_WORDS)()
        if clear:
            self._unchecked = False
        call("lzm_check_errors", self.h, out, int(bool(clear)), stream_ptr(stream))
        return list(out)

    def peek_errors(self, stream=None):
        """the sticky error words without raising or clearing them (synchronises the stream)"""
        out = (ctypes.c_int32 * _lib.LZM_ERR_WORDS)()
        _lib.load().lzm_check_errors(self.h, out, 0, stream_ptr(stream))
        return list(out)

    def search_diagnostics(self):
        out = torch.zeros(4, dtype=torch.int32, device=self.device)
        call("lzm_search_diagnostics", self.h, ptr(out), stream_ptr())
        return out.cpu().tolist()

    def distributions(self, stream=None):
        out = torch.empty((self.B, self.A), dtype=torch.int32, device=self.device)
        call("lzm_get_distributions", self.h, ptr(out), stream_ptr(stream))
        return out

    def values(self, stream=None):
        out = torch.empty(self.B, dtype=torch.float32, device=self.device)
        call("lzm_get_values", self.h, ptr(out), stream_ptr(stream))
        return out

    def root_outputs(self, stream=None):
        """(distributions(), values()) from one launch"""
        dist = torch.empty((self.B, self.A), dtype=torch.int32, device=self.device)
        vals = torch.empty(self.B, dtype=torch.float32, device=self.device)
        call("lzm_get_root_outputs", self.h, ptr(dist), ptr(vals), stream_ptr(stream))
        return dist, vals

    def trajectories(self, tmax=64, stream=None):
        out = torch.empty((self.B, tmax), dtype=torch.int32, device=self.device)
        call("lzm_get_trajectories", self.h, ptr(out), int(tmax), stream_ptr(stream))
        return out


def new_minmax(n, value_delta_max, device, stream=None, out=None):
    mm = torch.empty((n, 4), dtype=torch.float32, device=device) if out is None else out
    call("lzm_minmax_init", ptr(mm), int(n), float(np.float32(value_delta_max)), stream_ptr(stream))
    return mm


def seed_tensor(seed, device):
    return torch.tensor([np.uint32(seed).view(np.int32)], dtype=torch.int32, device=device)


# ----------------------------------------------------------------------------- handle pool
class TreePool:
    """Re-uses handles across searches so device pointers stay stable (graph replay)."""

    def __init__(self):
        self._free = {}
        self._lock = threading.Lock()

    def acquire(self, B, A, max_sims, ez, fast_rng, device, gumbel=False):
        key = (B, A, ez, fast_rng, str(device), bool(gumbel))
        t = None
        with self._lock:
            lst = self._free.get(key) or []
            while lst and t is None:
                c = lst.pop()
                # a tree whose owner was reclaimed by the cyclic GC can be returned here by
                # Roots.__del__ after its own finalizer closed the handle: skip it
                if c.h is not None and c.h.value:
                    t = c
        if t is None:
            t = DeviceTree(B, A, max_sims, ez=ez, fast_rng=fast_rng, device=device, gumbel=gumbel)
        else:
            t.reserve(max_sims)
            # the previous owner's sticky error words must not surface in this owner's searches
            # (ADVICE r03); acquiring happens between searches, never inside a graph capture
            if not torch.cuda.is_current_stream_capturing():
                t.reset_errors()
            t._value_support(0, 0)  # (the previous owner's value support length: host state on the handle)
        return t

    def release(self, t):
        if t is None or t.h is None:
            return
        key = (t.B, t.A, t.ez, t.fast_rng, str(t.device), t.gumbel)
        with self._lock:
            self._free.setdefault(key, []).append(t)


POOL = TreePool()
