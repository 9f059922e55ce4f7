"""Drop-in ``MuZeroMCTSCtree`` / ``EfficientZeroMCTSCtree`` / ``GumbelMuZeroMCTSCtree`` with the search loop on the GPU.

Same class surface as /root/reference/lzero/mcts/tree_search/mcts_ctree.py:172-420 (MuZero) and
:623-827 (EfficientZero): class attribute ``config``, ``default_config()``, ``__init__(cfg)``,
classmethod ``roots(n, legal_actions)`` and ``search(...)``. The difference is where the
per-simulation loop (mcts_ctree.py:255-321) runs: here every step is a device kernel or a
device-resident model call on one stream —

    traverse (select, HIP)  ->  gather leaf latents (HIP)  ->  model.recurrent_inference
    ->  decode value/reward supports + expand + backup (one HIP kernel, also files the new
        latents into the [S+1, B, ...] pool in HBM)

with no host round trip inside a search. The tree and the tie-break RNG follow the reference
bit for bit in the default parity mode (glibc rand() stream seeded per traverse, exactly one
draw per tree level), see lzm_kernels.hip.
"""
import copy
import os
import weakref
from collections import OrderedDict
from contextlib import contextmanager
from types import SimpleNamespace
from typing import Any, List, Union

import numpy as np
import torch

from . import _lib
from .ctree import ez_tree, gmz_tree, mz_tree
from .conv_infer import FoldedCache
from .fused import NotPackable, PackedCache, pack_efficientzero_mlp
from .scaling_transform import InverseScalarTransform
from .tree import DeviceTree, new_minmax, next_seed
from .utils import EasyDict


def _seeds(n, device):
    s = np.array([next_seed() for _ in range(n)], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(s).to(device)


def _to_play_tensor(to_play_batch, B, device):
    if isinstance(to_play_batch, torch.Tensor):
        return to_play_batch.to(device=device, dtype=torch.int32).reshape(B)
    if isinstance(to_play_batch, (int, np.integer)):
        return torch.full((B,), int(to_play_batch), dtype=torch.int32, device=device)
    return torch.as_tensor(np.asarray(to_play_batch, dtype=np.int32).reshape(B), device=device)


def _usable_i32(x, n, device):
    """a contiguous int32 device tensor of n elements on `device` (readable by a kernel as is)"""
    return (isinstance(x, torch.Tensor) and x.dtype == torch.int32 and x.is_contiguous() and x.numel() == n
            and x.device == torch.device(device))


def _latent_tensor(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float32)
    if isinstance(x, (list, tuple)):
        x = np.asarray(x)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)


class _Recorder:
    """Optional per-simulation record of what the tree requested and consumed (tests, tracing)."""

    def __init__(self, S, B, A, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.x = torch.zeros((S, B), **i32)
        self.action = torch.zeros((S, B), **i32)
        self.search_len = torch.zeros((S, B), **i32)
        self.vtp = torch.zeros((S, B), **i32)
        self.decoded = torch.zeros((S, B, 2), dtype=torch.float32, device=device)
        self.policy_logits = torch.zeros((S, B, A), dtype=torch.float32, device=device)
        self.seeds = None

    def step(self, k, t, policy_logits):
        self.x[k].copy_(t.x)
        self.action[k].copy_(t.action)
        self.search_len[k].copy_(t.search_len)
        self.vtp[k].copy_(t.vtp)
        self.policy_logits[k].copy_(policy_logits)

    def numpy(self):
        return {k: getattr(self, k).cpu().numpy() for k in
                ("x", "action", "search_len", "vtp", "decoded", "policy_logits")} | {"seeds": self.seeds}


class _SearchBuffers:
    """Per (B, S, latent shape) device buffers reused across searches."""

    def __init__(self):
        self.key = None

    def get(self, B, S, shape, device, extra=()):
        key = (B, S, tuple(shape), str(device), tuple(extra))
        if key != self.key:
            self.pool = torch.empty((S + 1, B) + tuple(shape), dtype=torch.float32, device=device)
            self.net_in = torch.empty((B,) + tuple(shape), dtype=torch.float32, device=device)
            self.extra = [torch.empty((S + 1, B, e), dtype=torch.float32, device=device) for e in extra]
            self.extra_in = [torch.empty((B, e), dtype=torch.float32, device=device) for e in extra]
            self.mm = torch.empty((B, 4), dtype=torch.float32, device=device)
            self.vtp_in = torch.empty(B, dtype=torch.int32, device=device)
            self.seeds = torch.empty(S, dtype=torch.int32, device=device)
            self.key = key
        return self


def _step_net(mcts, model):
    """the BN-folded recurrent step for the conv MuZeroModel / EfficientZeroModel family
    (conv_infer.FoldedConvNet, cfg.fold_network, default on), else the model itself"""
    if mcts._cfg.get('fold_network', True):
        net = mcts._folded.get(model)
        if net is not None:
            return net
    return model


class _GraphEntry:
    """One captured search: the graph together with everything its kernels point at — the
    buffers the inputs are copied into, the (folded) network whose weights it reads — so none of
    them can be freed or rebuilt while the graph may replay."""

    def __init__(self, graph, buf, net, model, tree):
        self.graph, self.buf, self.net = graph, buf, net
        self.model_ref, self.tree_ref = weakref.ref(model), weakref.ref(tree)

    def valid_for(self, model, tree):
        return self.model_ref() is model and self.tree_ref() is tree and tree.h is not None

    def replay(self):
        if self.net is not None and hasattr(self.net, "refresh"):
            self.net.refresh()  # re-fold in place if the parameters changed since capture
        self.graph.replay()


class _GraphCache:
    """LRU of captured searches keyed by (tree uid, tree generation, model, B, S, latent shape);
    entries whose tree or model died are dropped on lookup, the oldest beyond `cap` evicted."""

    def __init__(self, cap=4):
        self.cap = int(cap)
        self._d = OrderedDict()

    def __len__(self):
        return len(self._d)

    def get(self, key, model, tree):
        e = self._d.get(key)
        if e is None:
            return None
        if not e.valid_for(model, tree):
            del self._d[key]
            return None
        self._d.move_to_end(key)
        return e

    def put(self, key, entry):
        self._d[key] = entry
        self._d.move_to_end(key)
        for k in [k for k, e in self._d.items() if e.tree_ref() is None or e.model_ref() is None]:
            del self._d[k]
        while len(self._d) > self.cap:
            self._d.popitem(last=False)


def _graph_key(t, model, B, S, shape, extra=()):
    return (t.uid, t.generation, id(model), B, S, tuple(shape), tuple(extra))


def _fuse_traverse(cfg, t):
    """fold each simulation's traverse into the previous simulation's decode launch (parity mode;
    cfg.fuse_traverse, default off: measured even with the two launches at the conv configs,
    DESIGN.md 6.3; LZM_FUSE=0 forces it off)"""
    return cfg.get('fuse_traverse', False) and not t.fast_rng and os.environ.get("LZM_FUSE", "1") != "0"


class _HeadVerdicts:
    """The native conv step's head kernel writes ensure_softmax's verdict words for the tree's
    decode (one launch fewer per simulation); set for the duration of a loop."""

    def __init__(self, t, net, buf, on):
        self.t, self.net, self.on = t, net, on
        if on:
            n = 2 * ((t.B + 1) // 2)
            w = getattr(buf, "norm_words", None)
            if w is None or w.numel() != n or w.device != t.device:
                buf.norm_words = torch.ones(n, dtype=torch.int32, device=t.device)
            self.words = buf.norm_words

    def __enter__(self):
        if self.on:
            self.net.norm_out = self.words
            self.t.set_norm_words(self.words)
        return self

    def __exit__(self, *exc):
        if self.on:
            self.net.norm_out = None
            self.t.set_norm_words(None)
        return False


def _native_trunk(net, buf):
    """the step net runs the lzm_conv_trunk kernel straight on the latent pool"""
    return getattr(net, "native", None) is not None and tuple(buf.pool.shape[2:]) == (64, 8, 8)


class _MCTSCtree(object):
    """What MuZeroMCTSCtree and EfficientZeroMCTSCtree share: the class surface, the search prologue, the
    staging of seeds and to_play, the collect step's glue, the per-simulation loop and its graph capture.
    The subclasses add their public signatures, the network step of one simulation and their one-launch
    searches."""

    config = dict(
        root_dirichlet_alpha=0.3,
        root_noise_weight=0.25,
        pb_c_base=19652,
        pb_c_init=1.25,
        value_delta_max=0.01,
        env_type='not_board_games',
        # the one-launch conv searches over root slices (lzm_search_conv_sliced / lzm_search_conv_ez_sliced):
        # batches past 1,024 roots (EfficientZero: past 256 roots or the co-resident grid) stay on the
        # hand-written kernels, one launch per slice; sliced_search_max_roots caps a slice (0: the library's rule)
        sliced_search=False,
        sliced_search_max_roots=0,
    )

    _tree = None  # the ctree module of the roots this search takes (mz_tree / ez_tree)
    reward_name = None  # the step output the decode reads as the reward logits
    # MuZero keeps cfg.fuse_traverse on under search_with_reuse, EfficientZero turns it off there
    fuse_under_reuse = True
    # 'glibc': the reference's tie-break stream, bit-exact (default); 'philox': independent
    # counter-based stream per root (LZM_RNG_FAST), no batch-serial dependency.
    rng_mode = 'glibc'
    record = False  # set on an instance: keep a _Recorder of the next searches in last_record

    @classmethod
    def default_config(cls: type) -> EasyDict:
        cfg = EasyDict(copy.deepcopy(cls.config))
        cfg.cfg_type = cls.__name__ + 'Dict'
        return cfg

    def __init__(self, cfg: EasyDict = None) -> None:
        default_config = self.default_config()
        default_config.update(cfg)
        self._cfg = default_config
        self.inverse_scalar_transform_handle = InverseScalarTransform(
            self._cfg.model.support_scale, self._cfg.device, self._cfg.model.categorical_distribution
        )
        self._buf = _SearchBuffers()
        self._graphs = _GraphCache(int(self._cfg.get('graph_cache_size', 4)))
        self._folded = FoldedCache()
        self.residency_fallbacks = self.timeout_fallbacks = 0  # (one-launch searches re-run on the generic path)

    @classmethod
    def roots(cls: int, active_collect_env_num: int, legal_actions: List[Any]) -> "Roots":
        return cls._tree.Roots(active_collect_env_num, legal_actions, fast_rng=(cls.rng_mode == 'philox'))

    def _categorical(self):
        return bool(self._cfg.model.get('categorical_distribution', True))

    def _pb_c(self):
        return int(self._cfg.pb_c_base), float(self._cfg.pb_c_init)

    def _discount(self):
        return float(np.float32(self._cfg.discount_factor))

    # ---- the pieces of search() / search_with_reuse() ---------------------------------------------------------
    def _begin(self, what, roots, model, latent_state_roots, state_roots=()):
        """The prologue: the prepared tree with S simulations reserved, the root latents and the root rows of
        the extra state pools (EfficientZero's LSTM (c, h)) on the device, and their sizes."""
        model.eval()
        t = roots.tree
        if t is None:
            raise RuntimeError(f"{what}: roots must be prepared (Roots.prepare / prepare_no_noise) first")
        if what == "search_with_reuse" and t.fast_rng:
            raise ValueError("search_with_reuse: parity (glibc) mode only")
        B, S = roots.num, int(self._cfg.num_simulations)
        t.reserve(S)
        t.set_pb_c(*self._pb_c())
        lat0 = _latent_tensor(latent_state_roots, t.device)
        shape = tuple(lat0.shape[1:])
        state = [_latent_tensor(s, t.device).reshape(B, -1) for s in state_roots]
        return SimpleNamespace(t=t, B=B, S=S, dev=t.device, lat0=lat0, shape=shape,
                               row=int(np.prod(shape)) if len(shape) else 1, state=state,
                               extra=tuple(s.shape[1] for s in state), in_kernel=False)

    def _buffers(self, c, model, graph=False):
        """The search's buffers — the driver's own or, for a search replayed as a graph (cfg.use_hip_graph),
        the ones its captured graph owns (they are what its kernels point at) — with the roots' slots filled."""
        c.graph = bool(graph)
        c.gkey = _graph_key(c.t, model, c.B, c.S, c.shape, c.extra) if graph else None
        c.entry = self._graphs.get(c.gkey, model, c.t) if graph else None
        c.buf = c.entry.buf if c.entry is not None else (_SearchBuffers() if graph else self._buf).get(
            c.B, c.S, c.shape, c.dev, extra=c.extra)
        if c.lat0.data_ptr() != c.buf.pool[0].data_ptr():  # (the collect step writes it in place)
            c.buf.pool[0].copy_(c.lat0.reshape((c.B,) + c.shape))
        for pool, rows in zip(c.buf.extra, c.state):
            pool[0].copy_(rows)

    def _stage(self, c, to_play_batch, seeds, step, in_place=False):
        """(to_play, seeds) as device int32 tensors for the search: copied into the buffers, or with in_place
        the caller's own tensors where a kernel can read them as they are. The seeds come from the host seed
        source, from `seeds`, or from the collect step's counter (lzm_seed_sequence); None when the one-launch
        kernel derives them itself (c.in_kernel)."""
        buf = c.buf
        vt = to_play_batch if in_place and _usable_i32(to_play_batch, c.B, c.dev) else None
        if vt is None:
            buf.vtp_in.copy_(_to_play_tensor(to_play_batch, c.B, c.dev))
            vt = buf.vtp_in
        if c.in_kernel:
            return vt, None
        if step is not None:
            self._step_seeds(c, step)
            return vt, buf.seeds
        sd = seeds if in_place and _usable_i32(seeds, c.S, c.dev) else None
        if sd is None:
            buf.seeds.copy_(_seeds(c.S, c.dev) if seeds is None else seeds.reshape(c.S))
            sd = buf.seeds
        return vt, sd

    def _recorder(self, c):
        """a fresh _Recorder holding the staged seeds when self.record is set (is_reset on EfficientZero trees)"""
        if not self.record:
            return None
        rec = _Recorder(c.S, c.B, c.t.A, c.dev)
        if c.t.ez:
            rec.is_reset = torch.zeros((c.S, c.B), dtype=torch.int32, device=c.dev)
        rec.seeds = c.buf.seeds.cpu().numpy().view(np.uint32)
        return rec

    # the collect step's glue (search()'s `step`) as launches around a search: the seeds
    # (base + count * S + k) mod 10^6 before it, the root outputs and the counter increment after it
    def _step_seeds(self, c, step):
        _lib.call("lzm_seed_sequence", _lib.ptr(step["count"]), int(step["base"]), c.S, _lib.ptr(c.buf.seeds),
                  _lib.stream_ptr())

    def _step_outputs(self, c, step):
        _lib.call("lzm_get_root_outputs", c.t.h, _lib.ptr(step["dist"]), _lib.ptr(step["values"]), _lib.stream_ptr())
        if step.get("increment", True):
            step["count"].add_(1)

    @contextmanager
    def _glue(self, c, step):
        """Around a one-launch search: with c.in_kernel the kernel runs the collect step's glue itself
        (lzm_search_set_step: seeds from the step counter, fresh min-max bounds, root outputs, the counter
        increment), else fresh min-max bounds. A body that falls back to the generic path clears the mode
        and c.in_kernel itself."""
        if c.in_kernel:
            c.t.set_step(step["count"], int(step["base"]), step.get("increment", True), step["dist"], step["values"],
                         True, self._cfg.value_delta_max)
        else:
            new_minmax(c.B, self._cfg.value_delta_max, c.dev, out=c.buf.mm)
        try:
            yield
        finally:
            if c.in_kernel:
                c.t.set_step()

    def _generic(self, c, model, rec):
        """the per-simulation path: the loop itself or, with the graph _buffers looked up, its capture's replay"""
        if not c.graph:
            return self._loop(c.t, model, c, rec)
        if c.entry is None:
            c.entry = self._capture(c, model)
            self._graphs.put(c.gkey, c.entry)
        c.entry.replay()

    def _finish(self, c, roots, step, rec):
        if step is not None and not c.in_kernel:
            self._step_outputs(c, step)
        c.t.searched()
        roots._last_minmax = c.buf.mm
        self.last_record = rec

    def _search_with_reuse(self, roots, model, latent_state_roots, state_roots, to_play_batch, true_action_list,
                           reuse_value_list, seeds):
        if true_action_list is None or reuse_value_list is None:
            raise TypeError("search_with_reuse needs true_action_list and reuse_value_list")
        with torch.no_grad():
            c = self._begin("search_with_reuse", roots, model, latent_state_roots, state_roots)
            self._buffers(c, model)
            self._stage(c, to_play_batch, seeds, None)
            ta = torch.as_tensor(np.asarray(true_action_list, np.int32).reshape(c.B) if not torch.is_tensor(
                true_action_list) else true_action_list, device=c.dev)
            rv = torch.as_tensor(np.asarray(reuse_value_list, np.float32).reshape(c.B) if not torch.is_tensor(
                reuse_value_list) else reuse_value_list, device=c.dev)
            rec = self._recorder(c)
            infer = torch.zeros(c.S, dtype=torch.int64, device=c.dev)
            c.t.set_reuse(ta, rv)
            try:
                self._loop(c.t, model, c, rec, infer=infer)
            finally:
                c.t.set_reuse(None)
            roots._last_minmax = c.buf.mm
            self.last_record = rec
            counts = infer.cpu().numpy()
        return int(counts[-1]) if c.S else 0, float(counts.sum()) / max(c.S, 1)

    def _loop(self, t, model, c, rec=None, infer=None, net=None):
        """The S simulations (mcts_ctree.py:255-321, 756-827) on tree t over c.buf, all enqueued on the current
        stream. infer: optional device int64 [S], per simulation the number of roots that ran inference
        (search-with-reuse: roots whose walk stopped on an expanded node report x = -1).
        net: the step network to run (default: _step_net(model))."""
        cfg, buf, S = self._cfg, c.buf, c.S
        disc, cat, pb_c = self._discount(), self._categorical(), self._pb_c()
        new_minmax(t.B, cfg.value_delta_max, t.device, out=buf.mm)
        net = _step_net(self, model) if net is None else net
        native = _native_trunk(net, buf)
        fuse = _fuse_traverse(cfg, t) and (infer is None or self.fuse_under_reuse)
        with _HeadVerdicts(t, net, buf, native and cat and getattr(net, "heads", None) is not None):
            for k in range(S):
                if k == 0 or not fuse:
                    t.traverse(buf.mm, buf.seeds[k:k + 1], buf.vtp_in, *pb_c, disc)
                if infer is not None:
                    infer[k] = (t.x >= 0).sum()
                out = self._step(t, net, c, k, native)
                logits = out.policy_logits.float().contiguous()
                if rec is not None:
                    rec.step(k, t, logits)
                reward = getattr(out, self.reward_name).float().contiguous()
                value = out.value.float().contiguous()
                kw = dict(next_latent=None if native else out.latent_state.float().contiguous(),
                          pool_slot=None if native else buf.pool[k + 1], row_elems=0 if native else c.row,
                          out_decoded=None if rec is None else rec.decoded[k])
                if t.ez:
                    kw.update(lstm_horizon=int(cfg.lstm_horizon_len), out_is_reset=t.is_reset)
                if fuse and k + 1 < S:  # this simulation's backup and the next one's traverse in one launch
                    t.decode_backprop_traverse(k + 1, disc, buf.mm, reward, value, cat, logits, t.vtp,
                                               buf.seeds[k + 1:k + 2], buf.vtp_in, *pb_c, **kw)
                else:
                    t.decode_backprop(k + 1, disc, buf.mm, reward, value, cat, logits, t.vtp, **kw)
                self._after_step(t, out, c, k, native, rec)

    def _after_step(self, t, out, c, k, native, rec):
        pass  # (EfficientZero: the is_reset record and the reset mask on the LSTM state)

    def _capture(self, c, model):
        """Captures the whole S-simulation loop as one HIP graph over c.buf (the static buffers filled just
        before) and the network _step_net picks now; the entry keeps both alive."""
        t = c.t
        net = _step_net(self, model)
        # warm up every kernel and library handle on a scratch tree (must not touch `t`)
        scratch = DeviceTree(t.B, t.A, max(c.S, t.sims_capacity), ez=t.ez, fast_rng=t.fast_rng, device=t.device,
                             gumbel=t.gumbel)
        scratch.copy_roots_from(t)
        scratch.set_pb_c(*self._pb_c())
        self._loop(scratch, model, c, net=net)
        torch.cuda.synchronize(t.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._loop(t, model, c, net=net)
        scratch.close()
        return _GraphEntry(g, c.buf, net if net is not model else None, model, t)

    def _sliced(self):
        return bool(self._cfg.get('sliced_search', False))

    def _conv_plan(self, t, net, S, **kw):
        """the library's plan of this search's conv launch: the sliced launches' with cfg.sliced_search (the slice
        fields in last_plan), the single launch's otherwise"""
        if self._sliced():
            return t.search_conv_sliced_plan(net, S, max_roots=int(self._cfg.get('sliced_search_max_roots', 0) or 0),
                                             **kw)
        return t.search_conv_plan(net, S, **kw)

    def _conv_call(self, t, name, *args, **kw):
        """DeviceTree.<name> or, with cfg.sliced_search, DeviceTree.<name>_sliced with the configured cap"""
        if self._sliced():
            return getattr(t, name + "_sliced")(*args, max_roots=int(self._cfg.get('sliced_search_max_roots', 0) or 0),
                                                **kw)
        return getattr(t, name)(*args, **kw)

    def _conv_path(self, name):
        n = (self.last_plan or {}).get("slices", 1)
        return name if n <= 1 else f"{name} ({n} slices)"

    def _native_conv_net(self, model, t, shape, on=None):
        """What every _fused_conv starts from: the native split-precision step network of this class's family,
        with packed heads, when `on` (default: cfg.fused_search, itself default on) and LZM_FUSED_CONV allow a
        one-launch search of a 64 x 8 x 8 latent on tree t; None otherwise. Clears last_plan (the plan of this
        search, when the library is asked)."""
        self.last_plan = None
        ez = self._tree.Roots.EZ
        on = self._cfg.get('fused_search', True) if on is None else on
        if not on or t.ez != ez or os.environ.get("LZM_FUSED_CONV", "1") == "0":
            return None
        net = _step_net(self, model)
        hp = getattr(net, "heads", None)
        if tuple(shape) != (64, 8, 8) or getattr(net, "native", None) is None or hp is None \
                or getattr(net, "precision", None) != "split" or bool(getattr(net, "ez", not ez)) != ez \
                or hp["A"] != t.A:
            return None
        return net


class MuZeroMCTSCtree(_MCTSCtree):
    """MCTS for MuZero on the GPU (reference: mcts_ctree.py:172-321)."""

    _tree = mz_tree
    reward_name = 'reward'

    def __init__(self, cfg: EasyDict = None) -> None:
        super().__init__(cfg)
        self._packed = PackedCache()

    @classmethod
    def roots_from_mask(cls, action_mask: torch.Tensor) -> "mz_tree.Roots":
        """roots() with the legal lists taken from a device action mask (no host round trip)"""
        return mz_tree.Roots.from_action_mask(action_mask, fast_rng=(cls.rng_mode == 'philox'))

    def _fused(self, model, t, S=None):
        """(packed weights, dims) when the whole search can run as one lzm_search_mlp launch:
        a MuZeroModelMLP-shaped network with categorical heads, eval-mode BatchNorm and ReLU, of a
        shape the kernels take on this tree for S simulations (default: the tree's reserved capacity),
        by the library's own launch plan (lzm_search_mlp_supported, lzm_search_mlp_plan)."""
        if not self._cfg.get('fused_search', True) or not self._categorical() or t.ez:
            return None
        try:
            packed, dims = self._packed.get(model, t.device)
        except NotPackable:
            return None
        if dims["actions"] != t.A or dims["support"] != 2 * int(self._cfg.model.support_scale) + 1:
            return None
        if t.search_mlp_plan(dims, t.sims_capacity if S is None else S)["kernel"] is None:
            return None  # (the streaming kernel's LDS need at this width and tree size)
        return packed, dims

    def _fused_conv(self, model, t, shape, S=None):
        """The native split-precision FoldedConvNet when the whole search of S simulations (default: the tree's
        reserved capacity) can run as one lzm_search_conv launch: a conv MuZeroModel with a 64 x 8 x 8 latent
        whose trunk and heads are packed, of a shape and tree size the launch itself accepts — asked of the
        library (DeviceTree.search_conv_plan: head K multiples of 128, supports <= 1024, up to 1024 roots, the
        tree in the workgroup's LDS); None otherwise (the generic per-simulation path). cfg.fused_search
        (default on) and LZM_FUSED_CONV=0 turn it off. With cfg.sliced_search the sliced launches' plan is asked
        (DeviceTree.search_conv_sliced_plan: any number of roots, in slices of up to 1,024)."""
        net = self._native_conv_net(model, t, shape)
        if net is None:
            return None
        self.last_plan = self._conv_plan(t, net, t.sims_capacity if S is None else S, categorical=self._categorical())
        return net if self.last_plan["supported"] else None

    def _step(self, t, net, c, k, native):
        buf = c.buf
        if native:  # leaf latents read from the pool and the next latents filed by the trunk kernel
            return net.step_from_pool(buf.pool, t.x, t.action, buf.pool[k + 1], range_err=t.error_word(4))
        t.gather(buf.pool, c.row, buf.net_in)
        return net.recurrent_inference(buf.net_in, t.action64)

    def search(self, roots: Any, model: torch.nn.Module, latent_state_roots: List[Any],
               to_play_batch: Union[int, List[Any]], seeds: torch.Tensor = None, step: dict = None) -> None:
        """seeds (not in the reference): optional device int32 [num_simulations] traverse seeds
        (the srand(tv_usec) values, uint32 bits) instead of the host seed source — keeps the call
        free of host copies (HIP-graph capture, lightzero_amd.collect).
        step (not in the reference; lightzero_amd.collect): dict(count=int64 device counter,
        base=int, dist=int32 [B, A], values=float32 [B], increment=True) — the collect step's glue
        in the search itself: seeds (base + count * S + k) mod 10^6 (`seeds` ignored), count
        incremented (unless increment=False), the
        root outputs (get_distributions / get_values as device tensors) written to dist / values,
        fresh min-max bounds. The one-launch search does all of it in its kernel
        (lzm_search_set_step); other paths run the same steps as separate launches."""
        with torch.no_grad():
            c = self._begin("search", roots, model, latent_state_roots)
            t, S = c.t, c.S
            fz = self._fused(model, t, S)
            cz = self._fused_conv(model, t, c.shape, S) if fz is None else None
            one_launch = fz is not None or cz is not None
            self._buffers(c, model, graph=not one_launch and not self.record and self._cfg.get('use_hip_graph', False))
            # the one-launch searches read the caller's device seeds / to_play in place (no staging copies:
            # EfficientZero's always stages them) and run the collect step's glue in their kernels
            in_place = one_launch and not self.record
            c.in_kernel = step is not None and in_place
            vt, sd = self._stage(c, to_play_batch, seeds, step, in_place)
            rec = self._recorder(c)
            buf = c.buf
            if not one_launch:
                self._generic(c, model, rec)
            else:
                with self._glue(c, step):
                    if cz is not None:  # the conv network's whole search in one launch (lzm_search_conv)
                        self._conv_call(t, "search_conv", cz, S, buf.mm, sd, vt, buf.pool, *self._pb_c(),
                                        self._discount(), self._categorical(), rec=rec)
                    else:
                        packed, dims = fz
                        t.search_mlp(dims, packed, S, buf.mm, sd, vt, buf.pool, *self._pb_c(), self._discount(),
                                     rec=rec)
            self._finish(c, roots, step, rec)
            self.last_path = self._conv_path("fused-conv") if cz is not None else (
                "fused-mlp" if fz is not None else "generic")

    def search_with_reuse(self, roots: Any, model: torch.nn.Module, latent_state_roots: List[Any],
                          to_play_batch: Union[int, List[Any]], true_action_list=None, reuse_value_list=None,
                          seeds: torch.Tensor = None):
        """ReZero search with value reuse (mcts_ctree.py:323-420; arXiv 2404.16364): at the root the
        true action's child is scored with the reuse value (carm_score) and choosing it ends the
        walk; roots stopping on an already expanded node skip the network and back up their reuse
        value, roots stopping at the unexpanded true-action child are expanded but back up the
        reuse value too. Runs the generic device loop with the reuse inputs on the tree handle
        (lzm_set_reuse); the network is evaluated for every root (rows of skipped roots unused).
        Returns (length, average_infer) as the reference: roots that ran inference in the last
        simulation, and inferences per simulation."""
        return self._search_with_reuse(roots, model, latent_state_roots, (), to_play_batch, true_action_list,
                                       reuse_value_list, seeds)


class EfficientZeroMCTSCtree(_MCTSCtree):
    """MCTS for EfficientZero on the GPU (reference: mcts_ctree.py:623-827)."""

    _tree = ez_tree
    reward_name = 'value_prefix'
    fuse_under_reuse = False

    def __init__(self, cfg: EasyDict = None) -> None:
        super().__init__(cfg)
        self._packed = PackedCache(pack=pack_efficientzero_mlp)

    def _fused(self, model, t, Hl=None, S=None):
        """(packed weights, dims) when the whole search can run as one lzm_search_mlp_ez launch, by
        MuZeroMCTSCtree._fused's rules: cfg.fused_search, categorical heads, an EfficientZero tree, an
        EfficientZeroModelMLP-shaped network (eval-mode BatchNorm, ReLU, a one-layer reward LSTM) whose action
        and support sizes are the tree's and the config's and whose LSTM width is the root state's (Hl; None:
        not checked), of a shape the kernel takes on this tree for S simulations (default: the tree's reserved
        capacity) by the library's own launch plan (lzm_search_mlp_ez_supported, lzm_search_mlp_ez_plan)."""
        if not self._cfg.get('fused_search', True) or not self._categorical() or not t.ez:
            return None
        try:
            packed, dims = self._packed.get(model, t.device)
        except NotPackable:
            return None
        if dims["actions"] != t.A or dims["support"] != 2 * int(self._cfg.model.support_scale) + 1:
            return None
        if Hl is not None and dims["lstm_hidden"] != Hl:
            return None
        if t.search_mlp_ez_plan(dims, t.sims_capacity if S is None else S)["kernel"] is None:
            return None
        return packed, dims

    def _horizon(self):
        horizon = int(self._cfg.lstm_horizon_len)
        if horizon <= 0:
            raise ValueError("lstm_horizon_len must be > 0 (mcts_ctree.py:809, 899)")
        return horizon

    def _fused_conv(self, model, t, shape, Hl, S=None):
        """The native split-precision FoldedConvNet (with the fused LSTM step packed) when the whole search of
        S simulations (default: the tree's reserved capacity) is one the lzm_search_conv_ez launch takes: a
        conv EfficientZeroModel with a 64 x 8 x 8 latent whose trunk, heads and LSTM are packed, of a shape and
        tree size the launch accepts — asked of the library (DeviceTree.search_conv_plan: head K multiples of
        128, supports <= 1024, LSTM width a multiple of 128, the tree in LDS); None otherwise (the generic
        per-simulation path). A plan refused for co-residency only (max(B, 2 T) workgroups, T = ceil(B / 64) *
        H / 16 LSTM tiles, against the CUs and the kernel's occupancy) still returns the network: an eager
        search() launches, is refused with ResidencyError before anything runs, and counts the fallback; a
        captured one takes the generic path without launching.
        cfg.fused_search (default on) and LZM_FUSED_CONV=0 turn it off. With cfg.sliced_search the sliced
        launches' plan is asked (DeviceTree.search_conv_sliced_plan): a batch past 256 roots or past the
        co-resident grid runs as slices of whole 64-root blocks, and the co-residency refusal is left only
        when not even one block fits."""
        net = self._native_conv_net(model, t, shape)
        if net is None or getattr(net, "lstm_frag", None) is None or net.heads["Kr"] != Hl:
            return None
        plan = self._conv_plan(t, net, t.sims_capacity if S is None else S, H=Hl,
                               horizon=int(self._cfg.lstm_horizon_len), categorical=self._categorical())
        self.last_plan = plan
        return net if plan["supported"] or plan["code"] == _lib.LZM_ERR_RESIDENCY else None

    def _step(self, t, net, c, k, native):
        buf = c.buf
        if native:
            # the LSTM state is gathered from / filed (reset-masked) into the state pools on the device
            return net.step_from_pool_lstm(buf.pool, t.x, t.action, buf.pool[k + 1], buf.extra[0], buf.extra[1], k,
                                           t.search_len, int(self._cfg.lstm_horizon_len), err=t.error_word(3),
                                           range_err=t.error_word(4))
        t.gather(buf.extra[0], c.extra[0], buf.extra_in[0])
        t.gather(buf.extra[1], c.extra[1], buf.extra_in[1])
        hidden = (buf.extra_in[0].unsqueeze(0), buf.extra_in[1].unsqueeze(0))
        t.gather(buf.pool, c.row, buf.net_in)
        return net.recurrent_inference(buf.net_in, hidden, t.action64)

    def _after_step(self, t, out, c, k, native, rec):
        if rec is not None:
            rec.is_reset[k].copy_(t.is_reset)
        if native:
            return  # lzm_ez_lstm_cell already filed the masked state
        # reset the LSTM state of roots whose search_len % horizon == 0 (mcts_ctree.py:810-816)
        keep = (1 - t.is_reset).to(torch.float32).unsqueeze(1)
        for pool, s in zip(c.buf.extra, out.reward_hidden_state):
            torch.mul(s.reshape(t.B, -1).float(), keep, out=pool[k + 1])

    def search(self, roots: Any, model: torch.nn.Module, latent_state_roots: List[Any],
               reward_hidden_state_roots: List[Any], to_play_batch: Union[int, List[Any]],
               seeds: torch.Tensor = None, step: dict = None) -> None:
        """seeds: optional device int32 [num_simulations] traverse seeds; step: the collect step's glue
        (lightzero_amd.collect: device seeds from a step counter, root outputs into device tensors, the
        counter advanced) — both as in MuZeroMCTSCtree.search."""
        with torch.no_grad():
            self._horizon()
            c = self._begin("search", roots, model, latent_state_roots, reward_hidden_state_roots[:2])
            fz = self._fused(model, c.t, c.extra[0], c.S) if len(c.shape) == 1 else None
            if fz is not None:
                # the MLP network's whole search, reward LSTM included, in one launch (lzm_search_mlp_ez): every
                # root's LSTM is its own workgroup's work, nothing is co-resident (no hand-off guard, no snapshot)
                self.last_plan = None
                self._buffers(c, model)
                c.in_kernel = step is not None and not self.record
                self._stage(c, to_play_batch, seeds, step)
                rec = self._recorder(c)
                buf = c.buf
                with self._glue(c, step):
                    c.t.search_mlp_ez(fz[1], fz[0], c.S, buf.mm, None if c.in_kernel else buf.seeds, buf.vtp_in,
                                      buf.pool, buf.extra[0], buf.extra[1], self._horizon(), *self._pb_c(),
                                      self._discount(), rec=rec)
                self.last_path = "fused-mlp"
                self._finish(c, roots, step, rec)
                return
            cz = self._fused_conv(model, c.t, c.shape, c.extra[0], c.S)
            # A grid the plan refuses for co-residency is not launched where a fallback after the refusal is
            # not possible: when this search captures the generic path itself (use_hip_graph), and inside a
            # caller's stream capture (collect.py's graph), which then captures the generic path instead of
            # raising. (The plan is a host query; eagerly the launch is tried, refused and counted.)
            refused = cz is not None and not self.last_plan["supported"]
            graph = self._cfg.get('use_hip_graph', False) and not self.record and (cz is None or refused)
            if graph or (refused and torch.cuda.is_current_stream_capturing()):
                cz = None
            self._buffers(c, model, graph)
            c.in_kernel = step is not None and cz is not None and not self.record
            self._stage(c, to_play_batch, seeds, step)  # (always into the buffers, unlike MuZero's)
            rec = self._recorder(c)
            if cz is None:
                self.last_path = "generic"
                self._generic(c, model, rec)
            else:
                rec = self._search_conv_ez(c, model, cz, step, rec)
            self._finish(c, roots, step, rec)

    def _search_conv_ez(self, c, model, cz, step, rec):
        """The conv network's whole search, reward LSTM included, in one launch (lzm_search_conv_ez). The launch
        needs its whole grid co-resident: when the occupancy bound refuses it, nothing ran and the generic
        per-simulation path runs instead — eagerly only: inside a stream capture a plan-refused grid never gets
        here (search() dropped cz), and a refusal the plan did not foresee is raised (no fallback inside a
        capture). Eager launches are also checked for hand-off timeouts (another stream's kernel can
        hold CUs the static occupancy bound counted on): the tree (and the step counter) are kept, and a search
        whose waits timed out is discarded and re-run on the generic path. Returns the record that counts."""
        cfg, t, buf = self._cfg, c.t, c.buf
        capturing = torch.cuda.is_current_stream_capturing()
        guard = bool(cfg.get('guard_handoffs', True)) and not capturing
        with self._glue(c, step):
            if guard:
                snap = self._snapshot(t)
                count0 = step["count"].clone() if c.in_kernel else None
            try:
                self._conv_call(t, "search_conv_ez", cz, c.S, buf.mm, None if c.in_kernel else buf.seeds, buf.vtp_in,
                                buf.pool, buf.extra[0], buf.extra[1], int(cfg.lstm_horizon_len), *self._pb_c(),
                                self._discount(), self._categorical(), rec=rec)
                self.last_path = self._conv_path("fused")
                if not (guard and t.peek_errors()[0]):
                    return rec
                t.copy_roots_from(snap)
                t.reset_errors()
                if c.in_kernel:
                    step["count"].copy_(count0)
                self.timeout_fallbacks += 1
                self.last_path = "generic (hand-off timeout)"
            except _lib.ResidencyError:
                if capturing:
                    raise
                self.residency_fallbacks += 1
                self.last_path = "generic (co-residency refused)"
            if c.in_kernel:  # the glue as launches around the generic path
                t.set_step()
                c.in_kernel = False
                self._step_seeds(c, step)
            rec = self._recorder(c)
            self._loop(t, model, c, rec)
        return rec

    def _snapshot(self, t):
        """a copy of tree t (lzm_copy_tree) in a handle kept for the purpose"""
        key = (t.B, t.A, t.ez, t.fast_rng, str(t.device))
        s = getattr(self, "_snap", None)
        if s is None or s[0] != key:
            s = (key, DeviceTree(t.B, t.A, t.sims_capacity, ez=t.ez, fast_rng=t.fast_rng, device=t.device))
            self._snap = s
        s[1].reserve(t.sims_capacity)
        s[1].copy_roots_from(t)
        return s[1]

    def search_with_reuse(self, roots: Any, model: torch.nn.Module, latent_state_roots: List[Any],
                          reward_hidden_state_roots: List[Any], to_play_batch: Union[int, List[Any]],
                          true_action_list=None, reuse_value_list=None, seeds: torch.Tensor = None):
        """ReZero search with value reuse for EfficientZero (mcts_ctree.py:829-955; arXiv 2404.16364), in
        its DEFINED form: the reference builds is_reset_list over the envs that ran inference and
        cbatch_backpropagate_with_reuse then reads it by env index (ctree_efficientzero/lib/cnode.cpp:638),
        an out-of-range, misaligned read as soon as an env skips inference; here every env's leaf gets
        is_reset = search_len % lstm_horizon_len == 0 (what the reference computes when no env skips).
        Otherwise as MuZeroMCTSCtree.search_with_reuse: the true action's root child is scored with the
        reuse value, a walk stopping on it ends there (no inference when it is expanded, its reuse
        value backed up), the device loop runs every env's network row (skipped rows unused). Returns
        (length, average_infer) as the reference."""
        self._horizon()
        return self._search_with_reuse(roots, model, latent_state_roots, reward_hidden_state_roots[:2], to_play_batch,
                                       true_action_list, reuse_value_list, seeds)


class GumbelMuZeroMCTSCtree(_MCTSCtree):
    """MCTS for Gumbel MuZero on the GPU (reference: mcts_ctree.py:956-1123). The generic per-simulation loop over
    the Gumbel tree (lzm_gumbel.h): Gumbel traverse, leaf gather, recurrent_inference (the user's module or the
    native conv trunk, as _loop chooses), then one launch for this simulation's decode + expand + backup and the
    next simulation's traverse. Eager, or one HIP graph with cfg.use_hip_graph. The walk draws no random number:
    there are no seeds and no rng_mode, and search_with_reuse does not exist, as in the reference.
    With cfg.fused_search (off by default here) a MuZeroModelMLP's whole search runs as one launch
    (lzm_search_mlp_gumbel) where _fused allows it; with cfg.fused_conv_search (a key of its own, off by default)
    a conv MuZeroModel's runs as one launch per root slice (lzm_search_conv_gumbel) where _fused_conv allows it;
    last_path says which path ran."""

    config = dict(
        num_simulations=50,
        root_dirichlet_alpha=0.3,
        root_noise_weight=0.25,
        value_delta_max=0.01,
    )  # (the reference's keys only; cfg.fused_search and cfg.fused_conv_search are read with default False: the
    #    one-launch searches are opt-in)
    _tree = gmz_tree
    reward_name = 'reward'
    rng_mode = None
    FUSED_WIDE_HIDDEN = 512  # latents wider than this take the one launch only at one root per workgroup (_fused)

    def __init__(self, cfg: EasyDict = None) -> None:
        super().__init__(cfg)
        self._packed = PackedCache()

    @classmethod
    def roots(cls: int, active_collect_env_num: int, legal_actions: List[Any]) -> "gmz_tree.Roots":
        return gmz_tree.Roots(active_collect_env_num, legal_actions)

    def _pb_c(self):
        return 19652, 1.25  # (the handle's pUCT table, never read by the Gumbel walk)

    def _considered(self):
        return int(self._cfg.num_simulations), int(self._cfg.max_num_considered_actions)

    def _recorder(self, c):
        if not self.record:
            return None
        return _Recorder(c.S, c.B, c.t.A, c.dev)

    _step = MuZeroMCTSCtree._step

    def _fused(self, model, t, S):
        """(packed weights, dims) when cfg.fused_search is set and the whole search can run as one
        lzm_search_mlp_gumbel launch: a MuZeroModelMLP-shaped network with categorical heads, eval-mode BatchNorm
        and ReLU, whose actions and support match the tree and the config, of a shape the kernel takes on this
        tree for S simulations by the library's own launch plan (lzm_search_mlp_gumbel_plan: lzm_search_mlp's
        shapes, at most 64 actions, the LDS the tree slice with its raw_value needs) and the measured routing rule
        below; None otherwise."""
        if not self._cfg.get('fused_search', False) or not self._categorical():
            return None
        try:
            packed, dims = self._packed.get(model, t.device)
        except NotPackable:
            return None
        if dims["actions"] != t.A or dims["support"] != 2 * int(self._cfg.model.support_scale) + 1:
            return None
        plan = t.search_mlp_gumbel_plan(dims, S)
        if plan["kernel"] is None:
            return None
        # measured: a latent wider than 512 loses to the graph path once a workgroup holds several
        # roots (1,024 wide, 1,024 roots: 14.67 against 13.97 ms), and wins with one root per workgroup
        if dims["hidden"] > self.FUSED_WIDE_HIDDEN and plan["roots_per_wg"] > 1:
            return None
        return packed, dims

    def _max_roots(self):
        return int(self._cfg.get('sliced_search_max_roots', 0) or 0)

    def _fused_conv(self, model, t, shape, S):
        """The native split-precision FoldedConvNet (_native_conv_net's packing) when cfg.fused_conv_search is set
        and the whole search of S simulations can run as lzm_search_conv_gumbel launches: a conv MuZeroModel with a
        64 x 8 x 8 latent whose trunk and heads are packed, of a shape and tree size the launch itself accepts —
        asked of the library (DeviceTree.search_conv_gumbel_plan: lzm_search_conv's shapes, the tree slice with its
        raw_value and the Gumbel tables in the workgroup's LDS, any number of roots in slices of up to 1,024 or
        cfg.sliced_search_max_roots); None otherwise (the generic per-simulation path). The plan is left in
        last_plan. The key is not cfg.fused_search: DeviceSearchStep(algo="gumbel") sets that one for the MLP
        search, and a conv model keeps the generic path unless asked."""
        net = self._native_conv_net(model, t, shape, on=bool(self._cfg.get('fused_conv_search', False)))
        if net is None:
            return None
        self.last_plan = t.search_conv_gumbel_plan(net, S, categorical=self._categorical(),
                                                   max_roots=self._max_roots())
        return net if self.last_plan["supported"] else None

    def _loop(self, t, model, c, rec=None, infer=None, net=None):
        """The S simulations (mcts_ctree.py:1054-1122) on tree t over c.buf, all enqueued on the current stream:
        simulation k's backup and simulation k + 1's traverse share a launch."""
        cfg, buf, S = self._cfg, c.buf, c.S
        disc, cat, (ns, m) = self._discount(), self._categorical(), self._considered()
        new_minmax(t.B, cfg.value_delta_max, t.device, out=buf.mm)
        net = _step_net(self, model) if net is None else net
        native = _native_trunk(net, buf)
        with _HeadVerdicts(t, net, buf, native and cat and getattr(net, "heads", None) is not None):
            for k in range(S):
                if k == 0:
                    t.gumbel_traverse(ns, m, disc, buf.vtp_in)
                out = self._step(t, net, c, k, native)
                logits = out.policy_logits.float().contiguous()
                if rec is not None:
                    rec.step(k, t, logits)
                reward = out.reward.float().contiguous()
                value = out.value.float().contiguous()
                kw = dict(next_latent=None if native else out.latent_state.float().contiguous(),
                          pool_slot=None if native else buf.pool[k + 1], row_elems=0 if native else c.row,
                          out_decoded=None if rec is None else rec.decoded[k])
                if k + 1 < S:
                    t.gumbel_decode_backprop_traverse(k + 1, disc, buf.mm, reward, value, cat, logits, t.vtp, ns, m,
                                                      buf.vtp_in, **kw)
                else:
                    t.gumbel_decode_backprop(k + 1, disc, buf.mm, reward, value, cat, logits, t.vtp, **kw)

    def search(self, roots: Any, model: torch.nn.Module, latent_state_roots: List[Any],
               to_play_batch: Union[int, List[Any]]) -> None:
        with torch.no_grad():
            c = self._begin("search", roots, model, latent_state_roots)
            if not getattr(c.t, "gumbel", False):
                raise TypeError("GumbelMuZeroMCTSCtree.search: roots must come from GumbelMuZeroMCTSCtree.roots")
            c.t.set_considered(*self._considered())  # (before any capture: a synchronous table copy)
            fz = self._fused(model, c.t, c.S)
            cz = self._fused_conv(model, c.t, c.shape, c.S) if fz is None else None
            one_launch = fz is not None or cz is not None
            self._buffers(c, model, graph=not one_launch and not self.record and self._cfg.get('use_hip_graph', False))
            c.buf.vtp_in.copy_(_to_play_tensor(to_play_batch, c.B, c.dev))
            rec = self._recorder(c)
            if not one_launch:
                self._generic(c, model, rec)
            else:  # the whole search in one launch; the requests' to_play is the roots' (it passes through)
                new_minmax(c.B, self._cfg.value_delta_max, c.dev, out=c.buf.mm)
                if cz is not None:  # the conv network (lzm_search_conv_gumbel; one launch per root slice)
                    c.t.search_conv_gumbel(cz, c.S, self._considered()[1], c.buf.mm, c.buf.vtp_in, c.buf.pool,
                                           self._discount(), self._categorical(), rec=rec,
                                           max_roots=self._max_roots())
                else:
                    packed, dims = fz
                    c.t.search_mlp_gumbel(dims, packed, c.S, self._considered()[1], c.buf.mm, c.buf.vtp_in,
                                          c.buf.pool, self._discount(), rec=rec)
                if rec is not None:
                    rec.vtp.copy_(c.buf.vtp_in.expand(c.S, c.B))
            self._finish(c, roots, None, rec)
            # (independent slices are one search: their count is last_plan["slices"], not part of the path's name)
            self.last_path = "fused-conv" if cz is not None else ("fused-mlp" if fz is not None else "generic")
