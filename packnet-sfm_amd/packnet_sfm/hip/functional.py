"""torch.autograd bindings of the gfx950 kernels (forward AND hand-written backward kernels).

These Functions are what the drop-in modules (networks/layers/packnet/layers01.py,
losses/multiview_photometric_loss.py) are made of.  Autograd only sequences the launches; every derivative
is computed by a HIP kernel of libpnsfm_hip.so.
"""
import contextlib
import os
import weakref

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from . import _seq
from ._lib import HipError as _HipError

# bumped by optimizers that update parameters through raw pointers (bypassing tensor._version)
_WEIGHT_EPOCH = [0]


def bump_weight_epoch():
    _WEIGHT_EPOCH[0] += 1


def get_conv_math():
    from . import _lib
    return 'bx3' if _lib.get().pnsfm_get_conv_math() else 'f32'


def set_conv_math(mode):
    """Arithmetic of the conv forward / backward-data kernels: 'bx3' (default; fp32 rebuilt from exact bf16 splits on the
    bf16 matrix pipe, 6 products, fp32 accumulate) or 'f32' (v_mfma_f32_32x32x2_f32).  See include/pnsfm.h
    (pnsfm_set_conv_math).  The packed-weight layout depends on the mode: every cached packed weight is invalidated.
    Returns the previous mode."""
    from . import _lib
    m = {'bx3': 1, 'f32': 0, 1: 1, 0: 0}[mode]
    prev = _lib.get().pnsfm_set_conv_math(m)
    bump_weight_epoch()
    _PACK_TABLES.clear()      # the batched packer's device table records which weights the mode covers (and their layout)
    return 'bx3' if prev else 'f32'


# Fused / multi-tensor optimizers (torch.optim.Adam(fused=True), the one bench.py uses) update parameters WITHOUT bumping
# tensor._version, so the version alone cannot tell a packed weight copy is stale.  Every optimizer step of any
# torch.optim optimizer therefore advances the epoch (global post-step hook), which re-packs each conv weight on its next
# use: one read + two writes of the weight per step (~1.5 GB for PackNet01), inside the timed region of the bench.
# (Re-packing all weights right away on a side stream, underneath the next forward pass, measured slower: 82.7 vs 84.7
# img/s -- ~110 tiny launches contending with the first layers -- so packing stays lazy, in front of each conv.)
try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post_hook
    _reg_post_hook(lambda optimizer, args, kwargs: bump_weight_epoch())
except ImportError:      # older torch: callers must invalidate themselves (FlatAdam does)
    pass


class PackedConvWeight:
    """Per-layer cache of the MFMA-friendly weight layouts ([k*k][K][M], see csrc/conv2d.hip).

    Re-packed only when the parameter changed (tensor version / storage / optimizer epoch / dtype), so eval loops and the
    backward pass of the same step reuse the buffers.  Cost when stale: one read + two writes of the weight.
    The cache keeps an alias of the tensor it packed (`_src_*`): the key names that tensor's storage by its address, and an address
    is only unique while the storage is alive.  `module.half().float()` swaps a parameter's `.data` without touching its version
    counter; without the alias the freed fp32 storage could be handed back to the new fp32 tensor, giving an identical key over
    different (fp16-rounded) values.  In training the alias shares the parameter's storage: no extra memory.
    """

    def __init__(self, volatile=False):
        self.wp_fwd = None
        self.wp_bwd = None
        self.key_fwd = None
        self.key_bwd = None
        self._src_f = None            # alias of the tensor behind key_fwd / key_bwd / key_h16 (see the class comment)
        self._src_b = None
        self._src_h16 = None
        self.volatile = volatile      # weight is a freshly computed tensor every call (e.g. a composed kernel): always repack
        self._serial = 0
        self._weight_ref = None       # the parameter this cache last packed (repack_all re-packs it in the batched launch)
        self.wp_h16 = None            # fp16 forward (evaluation / inference): packed fp16 image + fp32 copy of the bias
        self.bias_h16 = None
        self.key_h16 = None
        self.shape_h16 = None
        self.fold_h16 = None          # fp16 forward of the ResNet networks: the folded BatchNorm behind the convolution
        self.key_fold_h16 = None
        self._src_fold_h16 = None

    def get(self, weight, need_bwd, tapT=False):
        """tapT: the packed images of weight.transpose(2, 3), read from `weight` in place (the same bytes as packing a materialised
        transpose: the key does not tell them apart).  Such a cache is never registered for the optimizer's batched re-pack, whose
        tables hold one image pair per parameter."""
        if self.volatile:
            self._serial += 1
            key = ('volatile', self._serial)
        else:
            # (torch.Size and torch.device compare and hash natively: no tuple() / str() per call -- ~300 calls per step)
            key = (weight._version, weight.data_ptr(), _WEIGHT_EPOCH[0], weight.shape, weight.device, weight.dtype)
        do_f = self.key_fwd != key
        do_b = need_bwd and self.key_bwd != key
        if do_f or do_b:
            w = weight.detach()
            if do_f and self.wp_fwd is not None and (self.wp_fwd.device != w.device):
                self.wp_fwd = None
            if do_b and self.wp_bwd is not None and (self.wp_bwd.device != w.device):
                self.wp_bwd = None
            f, b = ops.conv2d_pack(w.contiguous(), self.wp_fwd if do_f else None, self.wp_bwd if do_b else None,
                                   want_fwd=do_f, want_bwd=do_b, tapT=tapT)
            held = None if self.volatile else w
            if do_f:
                self.wp_fwd, self.key_fwd, self._src_f = f, key, held
            if do_b:
                self.wp_bwd, self.key_bwd, self._src_b = b, key, held
            if not self.volatile and not tapT and weight.is_leaf and weight.requires_grad:
                _register_packed(self, weight)
        return self.wp_fwd, (self.wp_bwd if need_bwd else None)

    @staticmethod
    def key_of(weight):
        return (weight._version, weight.data_ptr(), _WEIGHT_EPOCH[0], weight.shape, weight.device, weight.dtype)

    def get_h16(self, weight, bias, key=None, hold=None):
        """(packed fp16 weight, fp32 bias or None) of the fp16 forward.  `weight` is fp16 (a layer's parameter) or fp32 (a composed
        weight: then `key` names the parameters it was built from and `hold` is those parameters, kept alive with the key).  Never
        registered for the optimizer's batched repack."""
        if key is None:
            key = (self.key_of(weight), None if bias is None else self.key_of(bias))
            hold = (weight, bias)
        if self.key_h16 != key:
            self._src_h16 = tuple(None if t is None else t.detach() for t in hold)
            self.wp_h16 = ops.conv2d_pack_h16(weight.detach().contiguous(), self.wp_h16)
            self.bias_h16 = None if bias is None else bias.detach().float().contiguous()
            self.shape_h16 = tuple(weight.shape)
            self.key_h16 = key
        return self.wp_h16, self.bias_h16

    def get_fold_h16(self, bn):
        """fp32 [2, C] scale | shift of an eval-mode fp16 BatchNorm2d behind this layer's convolution (ops.bn_fold_h16), re-folded only
        when one of its four tensors changed: the key is key_of each, and aliases of them are held for the reason the class comment
        gives."""
        four = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = tuple(self.key_of(t) for t in four) + (bn.eps,)
        if self.key_fold_h16 != key:
            self._src_fold_h16 = tuple(t.detach() for t in four)
            self.fold_h16 = ops.bn_fold_h16(*(t.detach().contiguous() for t in four), bn.eps)
            self.key_fold_h16 = key
        return self.fold_h16


# ---- batched re-pack: every conv weight of the model in ONE launch, right after the optimizer step ----------------------------
# The lazy re-pack in front of each conv is ~100 launches of ~10 us per step (profiles/r03_*: 0.55 ms of the 0.83 ms the packers
# take are per-launch floor, not bytes).  Caches register the LEAF parameter they pack; repack_all() -- called by FlatAdam.step
# -- rebuilds the device table when the set of (parameter, buffers) changed, runs pnsfm_conv2d_pack_table and stamps the caches
# with the new key, so the next forward finds them fresh.  PNSFM_PACK_BATCH=0 keeps the lazy path only.
_PACK_REG = {}          # id(cache) -> (weakref(cache), weakref(parameter))
_PACK_TABLES = {}       # device -> [signature, table tensor, n items, blocks, indices of the covered (cache, parameter) pairs]


def _register_packed(cache, weight):
    ent = _PACK_REG.get(id(cache))
    if ent is not None and ent[0]() is cache and ent[1]() is weight:
        return
    cid = id(cache)
    _PACK_REG[cid] = (weakref.ref(cache, lambda r, cid=cid: _PACK_REG.pop(cid, None)), weakref.ref(weight))
    cache._weight_ref = _PACK_REG[cid][1]


def _pack_pairs(only=None, exclude=None):
    """{device: [(cache, parameter)]} of the registered conv weights whose forward AND backward-data buffers exist; `only` /
    `exclude`: sets of id(parameter)."""
    by_dev = {}
    for cref, wref in list(_PACK_REG.values()):
        c, w = cref(), wref()
        if c is None or w is None or c.wp_fwd is None or c.wp_bwd is None or c.wp_fwd.device != w.device:
            continue
        if (only is not None and id(w) not in only) or (exclude is not None and id(w) in exclude):
            continue
        by_dev.setdefault(w.device, []).append((c, w))
    return by_dev


def _run_pack_table(slot, dev, pairs):
    """One pnsfm_conv2d_pack_table launch over `pairs` on the CURRENT stream; the device table is cached under `slot` and rebuilt
    when the set of (parameter, buffers) or the arithmetic mode changed.  Returns the pairs the table covers."""
    # the table's coverage and layout follow from the arithmetic mode too (a table built under 'bx3' replayed after
    # set_conv_math('f32') wrote split-bf16 bytes into f32-layout buffers and stamped them fresh)
    sig = (get_conv_math(),) + tuple((w.data_ptr(), tuple(w.shape), c.wp_fwd.data_ptr(), c.wp_bwd.data_ptr()) for c, w in pairs)
    tab = _PACK_TABLES.get(slot)
    if tab is None or tab[0] != sig:
        table, n, blocks, covered = ops.conv2d_pack_table_build([(w.detach(), c.wp_fwd, c.wp_bwd) for c, w in pairs], dev)
        tab = _PACK_TABLES[slot] = [sig, table, n, blocks, covered]      # (indices into `pairs`: no strong references kept)
    if not tab[2]:
        return []
    with torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext():
        ops.conv2d_pack_table_run(tab[1], tab[2], tab[3])
    return [pairs[i] for i in tab[4]]


def _pack_batch_on():
    if os.environ.get('PNSFM_PACK_BATCH', '1') == '0' or not _PACK_REG:
        return False
    return not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())


def repack_all(exclude=None):
    """Re-pack every registered conv weight whose forward AND backward-data buffers exist, one launch per device, and stamp the
    caches fresh.  `exclude`: ids of parameters already re-packed (the optimizer's fused tail).  Returns the number of weights packed.  No-op
    under PNSFM_PACK_BATCH=0 and while a stream is being captured."""
    if not _pack_batch_on():
        return 0
    done = 0
    for dev, pairs in _pack_pairs(exclude=exclude).items():
        covered = _run_pack_table((dev, 'all' if not exclude else ('rest', len(exclude))), dev, pairs)
        stamp_packed(covered)
        done += len(covered)
    return done


def stamp_packed(pairs):
    for c, w in pairs:
        k = c.key_fwd = c.key_bwd = PackedConvWeight.key_of(w)
        if c._src_f is None or c._src_f.data_ptr() != k[1] or c._src_b is not c._src_f:
            c._src_f = c._src_b = w.detach()


class _WgradStream:
    """Weight gradients on a side HIP stream.  ON by default since round 5 (PNSFM_WGRAD_STREAM=0 switches it off): most launches of
    the backward pass are resident in ONE round of workgroups (tools/bx3_ablate.py: prologue -> matrix work -> store burst, all
    workgroups in step), so a second stream's kernel fills the ramp-up and the store tail of the first: +1.8 .. +2.2 % images/s in
    three same-box A/Bs on the atomics-free kernels (profiles/r04_ab_wgrad_side_stream.txt, profiles/r05_ab_streams.txt).  History:
    +4 % with the f32-MFMA kernels of round 1, a LOSS in round 2 (116.6 vs 123.8 img/s: the zero-fills and atomics of the then
    split-K / pixel-split kernels doubled the memset and event traffic), off from round 2 to round 4 -- in round 4 only because the
    bench's per-launch roofline is event-timed as-run; bench.py now prices the kernels in a separate pass with the side streams off.

    Within a layer's backward the data gradient is on the critical path (the next layer waits for it) while the weight
    gradient is only needed by the optimizer / the gradient all-reduce.  With a second stream the GPU can co-schedule
    the two kernels -- the low-resolution layers cannot fill 256 CUs on their own -- and the tail of one hides under
    the other.  Ordering: the side stream waits for the compute stream before each weight gradient (dy is ready), the
    inputs are `record_stream`-ed so the caching allocator does not recycle them early, and the compute stream joins the
    side stream once, from an autograd-engine callback at the end of the backward pass (before any optimizer / reducer
    kernel can touch the gradients).

    Only gradients of LEAF parameters that are used ONCE in the step go to the side stream: their sole consumer is the
    engine's AccumulateGrad (a pointer hand-over, no kernel).  A non-leaf weight (the composed kernel of the collapsed
    packing block) or a parameter used by several nodes (that block's Conv2d / Conv3d weights) has its gradient read or
    accumulated by compute-stream kernels during the same backward pass: for those the weight gradient still runs on the
    side stream next to the node's own data gradient, but the compute stream waits for it before the node returns.  (The collapsed
    packing block's parameters have an owner of their own where it applies -- _PackGrads -- and then stay in flight like the others.)
    """
    _env = os.environ.get('PNSFM_WGRAD_STREAM', '1')
    enabled = _env not in ('0', '')
    # PNSFM_WGRAD_STREAM=<n> with n > 1: only layers whose gradient map has at most n pixels (batch x H x W) go to the side stream --
    # the low-resolution layers, whose launches are resident in one round and latency-bound (tools/bx3_ablate.py), overlap well;
    # the full-resolution ones are MFMA-bound and only contend
    max_pixels = int(_env) if _env.isdigit() and int(_env) > 1 else None

    @classmethod
    def use_for(cls, dy):
        if not (cls.enabled and dy.is_cuda):
            return False
        return cls.max_pixels is None or dy.shape[0] * dy.shape[-2] * dy.shape[-1] <= cls.max_pixels
    _streams = {}
    _pending = set()
    _uses = {}          # id(parameter) -> [forward uses whose backward has not run yet, shared-in-this-step flag]
    _cb_task = None     # autograd graph-task id whose end-of-backward callback is queued (None: no backward in flight)

    @classmethod
    def note_use(cls, recording, *params):
        """Called in forward for every parameter a node will produce a gradient for.  `recording`: autograd was recording
        when the op was CALLED (torch.is_grad_enabled() outside the Function -- inside forward grad mode is always off and
        needs_input_grad ignores no_grad), so validation under torch.no_grad() is not counted.  Entries of graphs that are
        never back-propagated make the next step fall back to the in-node wait and are dropped at the end of that step's
        backward pass."""
        if not recording:
            return
        for p in params:
            if p is not None and p.requires_grad:
                u = cls._uses.setdefault(id(p), [0, False])
                u[0] += 1
                if u[0] > 1:
                    u[1] = True

    @classmethod
    def side_ok(cls, *params):
        """Called once in backward: may this node's parameter gradients be left in flight on the side stream until the
        end-of-backward join (True), or must the node wait for them itself (False)?"""
        ok = True
        task = torch._C._current_graph_task_id()
        if cls._cb_task != task:        # first parameter gradient of this backward pass: arrange the end-of-pass clean-up
            if cls._cb_task is not None:
                # the previous backward pass never reached its callback (it raised): join what it left in flight now
                cls._join_pending()
            cls._cb_task = task
            from torch.autograd import Variable
            Variable._execution_engine.queue_callback(cls._end_of_backward)
        for p in params:
            if p is None:
                continue
            u = cls._uses.get(id(p))
            if not p.is_leaf or u is None or u[1]:
                ok = False
            # AccumulateGrad only hands the pointer over when .grad is None and nothing hooks the gradient; otherwise it
            # runs `p.grad += dw` (or the hook) on the COMPUTE stream, which knows nothing about the side stream: gradient
            # accumulation over several backward() calls, zero_grad(set_to_none=False), Tensor.register_hook
            if p.is_leaf and (p.grad is not None or p._backward_hooks):
                ok = False
            if u is not None:
                u[0] -= 1
                if u[0] <= 0:
                    del cls._uses[id(p)]
        return ok

    @classmethod
    def get(cls, device):
        st = cls._streams.get(device)
        if st is None:
            st = cls._streams[device] = torch.cuda.Stream(device=device)
        return st

    @classmethod
    def run(cls, fn, *tensors, detached=True, pure=True):
        """fn() -> outputs, executed on the side stream of tensors[0].device.  detached: nothing on the compute stream
        will touch the outputs before the end-of-backward join; otherwise returns (outputs, wait) and the caller must
        call wait() on the compute stream after it has enqueued its own independent work.
        pure (round 5): fn calls nothing but ops.* launches -- the fork is one C call (ops.stream_wait_stream) and the launches are
        redirected with ops.stream_override instead of torch's Stream.wait_stream + stream context (~50 -> ~10 us of host time per
        weight gradient, ~75 of them per step).  Outputs are then allocated in the COMPUTE stream's pool: they are gradients that live
        until the optimizer has run, long after the end-of-backward join, so the allocator cannot hand their memory out early."""
        dev = tensors[0].device
        side = cls.get(dev)
        if pure and _FAST_FORK:
            main_raw, side_raw = ops.current_raw_stream(dev), side.cuda_stream
            ops.stream_wait_stream(side_raw, main_raw)
            with ops.stream_override(side_raw, dev.index):
                out = fn()
            for t in tensors:
                t.record_stream(side)       # inputs live in the compute stream's pool but are read here
            if not detached:
                return out, (lambda: ops.stream_wait_stream(main_raw, side_raw))
            cls._pending.add(dev)
            return out
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            out = fn()
            ev = None if detached else side.record_event()
        for t in tensors:
            t.record_stream(side)           # inputs live in the compute stream's pool but are read here
        for o in out:
            if o is not None:
                o.record_stream(main)       # outputs live in the side stream's pool but are consumed on the compute stream
        if not detached:
            return out, (lambda: main.wait_event(ev))
        cls._pending.add(dev)            # joined by _end_of_backward (queued by side_ok, which every caller ran first)
        return out

    @classmethod
    def run_beside(cls, dy, want_w, detached, wgrad, dgrad, tensors, pure=True):
        """(dx, dw, db) of one conv node, the weight gradient beside the data gradient: wgrad() -> (dw, db) goes to the side stream
        first when `dy` qualifies (see run: `tensors` are what it reads, `detached` / `pure` as there), then dgrad() -> dx (or None: no
        data gradient wanted) on the compute stream, then the weight gradient in line if it was not forked, then the wait of a
        gradient that must not stay in flight."""
        dx = dw = db = wait = None
        if want_w and cls.use_for(dy):
            r = cls.run(wgrad, *tensors, detached=detached, pure=pure)
            (dw, db), wait = (r, None) if detached else r
            want_w = False
        if dgrad is not None:
            dx = dgrad()
        if want_w:
            dw, db = wgrad()
        if wait is not None:
            wait()
        return dx, dw, db

    @classmethod
    def seq_fork(cls, dy, want_w, detached):
        """(main raw stream, side raw stream or 0, side torch Stream or None) for a block-sequencer backward body, which forks, launches
        and joins by itself (csrc/seq/pnsfm_seq.cpp: conv_backward_tail, the order of run_beside with the one-call fork of run).  A
        detached weight gradient is left in flight: the device is marked for the end-of-backward join here."""
        if not dy.is_cuda:
            return 0, 0, None
        main_raw = ops.launch_stream_raw(dy.device)
        if want_w and cls.use_for(dy):
            side = cls.get(dy.device)
            if detached:
                cls._pending.add(dy.device)
            return main_raw, side.cuda_stream, side
        return main_raw, 0, None

    @classmethod
    def _end_of_backward(cls):
        """Autograd-engine callback at the end of a backward pass: the compute streams wait for the weight gradients
        still in flight, and the per-pass use counts are dropped."""
        cls._cb_task = None
        cls._join_pending()
        cls._uses.clear()
        _PackGrads.end_of_backward()

    @classmethod
    def _join_pending(cls):
        for dev in list(cls._pending):
            torch.cuda.current_stream(dev).wait_stream(cls.get(dev))
        cls._pending.clear()


_FAST_FORK = os.environ.get('PNSFM_FAST_FORK', '1') != '0'


def set_wgrad_stream(on):
    _WgradStream.enabled = bool(on)


# Gradient slots: id(parameter) -> (weak reference to the parameter, tensor its gradient should be WRITTEN into: a view of the
# flat gradient arena of rccl/flat_adam.py, which is also the all-reduce bucket).  Only used when the node's gradient is the
# parameter's only one this step (leaf, used once, .grad undefined, no hooks -- exactly `side_ok`): then AccumulateGrad just
# adopts the view.  The entry dies with the parameter (weakref callback) and is only honoured while the weak reference still
# points at the very tensor object asking -- CPython reuses ids, so a later model must never find a dead optimizer's arena.
_GRAD_SLOTS = {}


def _drop_slot(key, ref):
    ent = _GRAD_SLOTS.get(key)
    if ent is not None and ent[0] is ref:
        del _GRAD_SLOTS[key]


def register_grad_slots(pairs):
    """pairs: iterable of (parameter, view).  Returns a handle whose .remove() unregisters them (also done automatically when a
    parameter is garbage-collected, and when a newer optimizer registers the same parameter: the newer registration wins)."""
    mine = []
    for p, v in pairs:
        key = id(p)
        ref = weakref.ref(p, lambda r, key=key: _drop_slot(key, r))
        _GRAD_SLOTS[key] = (ref, v)
        mine.append((key, ref))

    class _Handle:
        def remove(self):
            for key, ref in mine:
                _drop_slot(key, ref)
            del mine[:]
    return _Handle()


def _slot_of(p):
    """The registered gradient slot of parameter `p`, or None (stale entries of a collected parameter never match)."""
    if p is None:
        return None
    ent = _GRAD_SLOTS.get(id(p))
    if ent is None or ent[0]() is not p:
        return None
    return ent[1]


def _slots_for(weight, bias, usable):
    if not usable or not _GRAD_SLOTS:
        return None, None
    sw = _slot_of(weight)
    sb = _slot_of(bias)
    if sw is None or (bias is not None and sb is None):
        return None, None
    if tuple(sw.shape) != tuple(weight.shape) or (bias is not None and sb.numel() != bias.numel()):
        return None, None           # the parameter was re-shaped behind the optimizer's back: plain gradient path
    return sw, sb


class _PackGrads:
    """One owner for the gradients of the four parameters (W2, b2, W3, b3) of a collapsed packing block (PNSFM_PACK_WPATH, below).

    Each of them is read by three nodes of the block -- the kernel composition, the row strips and the column strips -- so autograd
    used to add three gradients per parameter with elementwise kernels (one of them through a transposed view), FlatAdam gathered
    the sums into its arena with a copy, and the compute stream waited inside every node for a weight gradient on the side stream.
    With an owner the FIRST contribution of a backward pass is written into the parameter's gradient slot (_slot_of; a fresh tensor
    when no optimizer registered one), LATER ones are added there by the kernels' own epilogues (dst = dst + finished sum: the bits
    of the elementwise add) and only the LAST node hands the tensor to autograd; the others return None.  The order of the
    contributions is the order the engine runs the nodes in -- column strips, row strips, composition -- so (g1 + g2) + g3 is unchanged.

    Two groups, each returned by its own last node: 'c2' = (W2, b2), 'c3' = (W3, b3).  Streams: a contribution on the side stream is
    ordered behind everything on the compute stream by the fork (_WgradStream.run); one on the compute stream that follows one on
    the side stream waits for it explicitly (before()).  The owner is made per forward call (layers01.py) and decides ONCE per
    backward pass, at its first node, whether it is in charge: every parameter a leaf without .grad and without hooks (what
    side_ok asks), and no other owner of the same parameters alive in the graph.  Otherwise every node returns its own gradient,
    in the parameter's own layout, and autograd adds them as before."""
    _live = {}          # id(parameter) -> owners made for it since the last end of a backward pass
    _active = []        # owners in charge in the running backward pass (checked complete at its end)
    passes = 0          # backward passes an owner was in charge of (tests)

    def __init__(self, W2, b2, W3, b3):
        self.params = (W2, b2, W3, b3)
        self.expect = {'c2': 0, 'c3': 0}
        self.left = None
        self.task = None
        self.on = False
        self.dst = {'c2': None, 'c3': None}
        self.side_dirty = False
        for q in self.params:
            if q is not None:
                _PackGrads._live[id(q)] = _PackGrads._live.get(id(q), 0) + 1

    def expect_node(self, *groups):
        for g in groups:
            self.expect[g] += 1

    def begin(self):
        """Called by every node's backward: is the owner in charge in this backward pass?"""
        task = torch._C._current_graph_task_id()
        if self.task != task:
            self.task = task
            self.left = dict(self.expect)
            self.dst = {'c2': None, 'c3': None}
            self.side_dirty = False
            self.on = all(q is None or (q.is_leaf and q.grad is None and not q._backward_hooks and _PackGrads._live.get(id(q), 0) == 1)
                          for q in self.params)
            if self.on:
                _PackGrads._active.append(self)
                _PackGrads.passes += 1
        return self.on

    def dest(self, group):
        """(weight destination, bias destination or None, first contribution?) of `group`."""
        d = self.dst[group]
        if d is not None:
            return d[0], d[1], False
        w, b = self.params[:2] if group == 'c2' else self.params[2:]
        sw, sb = _slot_of(w), _slot_of(b)
        if sw is not None and tuple(sw.shape) != tuple(w.shape):
            sw = None
        if sb is not None and sb.numel() != b.numel():
            sb = None
        dw = sw if sw is not None else torch.empty_like(w, memory_format=torch.contiguous_format)
        db = None if b is None else (sb if sb is not None else torch.empty_like(b))
        self.dst[group] = (dw, db)
        return dw, db, True

    def before(self, ref, on_side):
        """Stream order of the contribution about to be enqueued for a tensor on ref's device: on the compute stream behind
        contributions still running on the side stream."""
        if on_side:
            self.side_dirty = True
        elif self.side_dirty and ref.is_cuda:
            ops.stream_wait_stream(ops.launch_stream_raw(ref.device), _WgradStream.get(ref.device).cuda_stream)
            self.side_dirty = False

    def done(self, group):
        """A node has enqueued its contribution to `group`: (dw, db) for autograd when it was the last one, else (None, None)."""
        self.left[group] -= 1
        if self.left[group] > 0:
            return None, None
        dw, db = self.dst[group]
        self.dst[group] = None
        # fresh view objects: AccumulateGrad adopts a gradient only if nobody else holds the tensor object
        return dw.view(dw.shape), (None if db is None else db.view(db.shape))

    @classmethod
    def end_of_backward(cls):
        act, cls._active = cls._active, []
        cls._live.clear()
        for o in act:
            if o.left is not None and any(v > 0 for v in o.left.values()):
                o.task = None
                raise RuntimeError("collapsed packing block: a backward pass ended before every node had contributed its parameter "
                                   "gradients (PNSFM_PACK_WPATH=0 runs the path without a gradient owner)")


def pack_grad_owner(W2, b2, W3, b3, h, w):
    """The gradient owner of a collapsed packing block's forward call on a packed map of h x w pixels, or None: the former path.
    Needs autograd recording, four trainable leaf parameters, the packers' in-place tap transpose for the Conv2d (split-bf16 layers)
    and the row-window Conv3d kernels for both strip directions."""
    if not (_PACK_WPATH and torch.is_grad_enabled() and ops.conv3d_ring_ok()):
        return None
    for q in (W2, W3, b3):
        if not (q.is_leaf and q.requires_grad and q.dtype == torch.float32):
            return None
    if b2 is not None and not (b2.is_leaf and b2.requires_grad):
        return None
    if get_conv_math() != 'bx3' or not ops.conv2d_pack_tapT_supported(W2.shape[1], W2.shape[0], W2.shape[2]):
        return None
    if not (ops.conv3d_rows_window_ok(w) and ops.conv3d_rows_window_ok(h)):
        return None
    return _PackGrads(W2, b2, W3, b3)


def side_streams(device):
    """The side streams gradients may still be in flight on (weight-gradient stream, independent-branch stream) -- for a consumer
    that wants ITS stream to wait for them instead of joining them into the compute stream (rccl/reducer.py)."""
    if device.type != 'cuda':
        return []
    return [st for st in (_WgradStream._streams.get(device), _BRANCH_STREAMS.get(device)) if st is not None]


def join_wgrad_stream(device):
    """Make the current stream of `device` wait for every weight gradient launched so far (no-op when unused) and for the
    independent-branch stream (branch_stream) -- the gradient all-reduce calls this before it gathers a bucket in the middle
    of the backward pass, and a bucket may hold parameters of both networks."""
    if device.type != 'cuda':
        return
    cur = torch.cuda.current_stream(device)
    for st in (_WgradStream._streams.get(device), _BRANCH_STREAMS.get(device)):
        if st is not None and st != cur:
            cur.wait_stream(st)


# Independent-branch stream: the pose network shares nothing with the depth network until the loss, and its kernels are tiny
# (a few workgroups each, latency-bound), so models/SfmModel.py enqueues it on a second HIP stream where it fills the launch gaps
# and tail rounds of the depth network's kernels.  Autograd replays every node on the stream its forward ran on and orders the
# two streams with events, so the pose network's backward pass overlaps the depth decoder's backward pass the same way.
# ON by default since round 5 (PNSFM_BRANCH_STREAM=0 / set_branch_stream(False) switch it off): +0.85 % images/s
# (profiles/r04_ab_branch_stream.txt), bit-identical results (tests/test_gpu_round4.py::test_branch_stream_is_bit_identical).
# Kernels that share the GPU stretch each other, so bench.py measures the per-kernel roofline in a pass with both side streams off.
_BRANCH_STREAMS = {}
_BRANCH_ON = os.environ.get('PNSFM_BRANCH_STREAM', '1') == '1'


def set_branch_stream(on):
    global _BRANCH_ON
    _BRANCH_ON = bool(on)


def branch_stream(t):
    """The second compute stream of t's device, or None (CPU tensors, switched off)."""
    if not (_BRANCH_ON and torch.is_tensor(t) and t.is_cuda):
        return None
    st = _BRANCH_STREAMS.get(t.device)
    if st is None:
        st = _BRANCH_STREAMS[t.device] = torch.cuda.Stream(device=t.device)
    return st


# ---- fp16 forward (evaluation / inference; include/pnsfm.h "fp16 forward") ---------------------------------------------------------
# fp16 activations dispatch to the _h16 kernels here, before any fp32 code path runs (the block sequencer never sees fp16).  Forward
# only: with grad disabled the ops are called directly; with grad enabled the result carries a node whose backward raises.
_H16_ONLY_FWD = "fp16 is supported for the forward pass only (evaluation / inference); train in float32"


class _H16ForwardOnlyFn(Function):
    @staticmethod
    def forward(ctx, fn, *args):
        return fn(*args)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(_H16_ONLY_FWD)


def _h16_run(fn, *args):
    if torch.is_grad_enabled() and any(torch.is_tensor(a) and a.requires_grad for a in args):
        return _H16ForwardOnlyFn.apply(fn, *args)
    return fn(*args)


def _h16_params(*params):
    """Mixed precision is an error, as F.conv2d makes it one in the reference: fp16 activations need fp16 parameters."""
    for p in params:
        if p is not None and p.dtype != torch.float16:
            raise RuntimeError("fp16 input into a %s layer: convert the network with .half() / .to(dtype=torch.float16)" % p.dtype)


def _h16_input(x, *params):
    """x is fp32 but a parameter is fp16: the reverse mix, named clearly instead of failing inside a kernel wrapper."""
    for p in params:
        if p is not None and p.dtype == torch.float16:
            raise RuntimeError("%s input into a float16 network: cast the input with .half()" % x.dtype)


def _conv2d_h16(xs, weight, bias, cache):
    _h16_params(weight, bias)
    Cout, Cin, ks, _ = weight.shape
    if sum(t.shape[1] for t in xs) != Cin:
        raise RuntimeError("conv2d: inputs have %d channels, weight expects %d" % (sum(t.shape[1] for t in xs), Cin))
    wp, b32 = cache.get_h16(weight, bias)
    return _h16_run(lambda *a: ops.conv2d_forward_h16(tuple(t.contiguous() for t in a[:len(xs)]), wp, b32, Cout, ks), *xs, weight, bias)


def _groupnorm_act_h16(x, gamma, beta, G, eps, act, res=None):
    _h16_params(gamma, beta)
    if res is not None and res.dtype != torch.float16:
        raise RuntimeError("groupnorm_act: fp16 input with a %s residual" % res.dtype)
    return _h16_run(lambda x, r, g, b: ops.groupnorm_act_forward_h16(x.contiguous(), None if r is None else r.contiguous(), g.detach(),
                                                                     b.detach(), G, eps, act), x, res, gamma, beta)


def conv2d_h16_composed(P, W_eff, bias_eff, cache, key):
    """fp16 forward of the collapsed packing convolution: W_eff / bias_eff are fp32 (composed from the upcast fp16 parameters); the
    packed fp16 image and the fp32 bias are cached on `key` (the parameters' keys: eval weights do not change).  W_eff may be None
    when the cache already holds `key`."""
    if W_eff is not None:
        cache.get_h16(W_eff, bias_eff, key=key)
    if cache.key_h16 != key:
        raise RuntimeError("conv2d_h16_composed: no packed weight for these parameters")
    Cout, _, ks, _ = cache.shape_h16
    return ops.conv2d_forward_h16((P.contiguous(),), cache.wp_h16, cache.bias_h16, Cout, ks)


def conv2d_h16_fused(xs, weight, cache, *, stride=1, pad='zeros', up=1, bias=None, bn=None, res=None, act=ops.ACT_NONE, disp=(0., 1.),
                     pre_affine=None):
    """The fp16 forward's convolution of the ResNet networks, everything around it included, in one launch (csrc/conv2d_h16g.h):
    act(bn(conv(pad(cat(upsample(xs))) * a + b, weight) + bias) + res).  xs: a tensor or up to three (their channel concatenation), each
    up-sampled by `up` (one factor, or one per source) first; pad: 'zeros' | 'reflect' of k // 2; bn: an nn.BatchNorm2d in eval mode
    (folded into a per-channel scale and shift, cached in `cache`); res: fp16 of the output's shape; pre_affine: (a, b)."""
    xs = tuple(xs) if isinstance(xs, (tuple, list)) else (xs,)
    ups = tuple(up) if isinstance(up, (tuple, list)) else (up,) * len(xs)
    if pad not in ('zeros', 'reflect'):
        raise ValueError("conv2d_h16_fused: pad must be 'zeros' or 'reflect', got %r" % (pad,))
    bn_params = () if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    for t in xs + (res,):
        if t is not None and t.dtype != torch.float16:
            _h16_input(t, weight, bias, *bn_params)
            raise RuntimeError("conv2d_h16_fused: float16 activations only, got %s" % t.dtype)
    if bn is not None:
        if bn.training or not bn.track_running_stats or bn.running_mean is None or not bn.affine:
            raise NotImplementedError("fp16 BatchNorm runs with running statistics only (evaluation / inference): call .eval(); "
                                      "training needs float32")
        if bias is not None:
            raise ValueError("conv2d_h16_fused: a bias and a BatchNorm behind one convolution are not supported")
    _h16_params(weight, bias, *bn_params)
    Cout, Cin, ks, _ = weight.shape
    if sum(t.shape[1] for t in xs) != Cin:
        raise RuntimeError("conv2d: inputs have %d channels, weight expects %d" % (sum(t.shape[1] for t in xs), Cin))
    wp, b32 = cache.get_h16(weight, bias)
    scale = shift = None
    if bn is not None:
        fold = cache.get_fold_h16(bn)
        scale, shift = fold[0], fold[1]
    elif b32 is not None:
        shift = b32
    n = len(xs)

    def run(*a):
        return ops.conv2d_forward_h16g(tuple(t.contiguous() for t in a[:n]), wp, Cout, ks, stride=stride, reflect=(pad == 'reflect'),
                                       ups=ups, scale=scale, shift=shift, res=None if a[n] is None else a[n].contiguous(), act=act,
                                       disp=disp, pre_affine=pre_affine)
    return _h16_run(run, *xs, res, weight, bias, *bn_params[:2])


# ---- the stride-1 conv nodes (Conv2dFn, ConvGnActFn): what their backward bodies share once dy exists ---------------------------------
def _seq_takes(dy, xs, want_w, cat_wgrad, g_tap):
    """May the block sequencer run this conv backward as its one call?  Its weight gradient is the multi-source kernel or nothing (no
    concatenating fallback), its tap is the addend of the split-bf16 backward-data kernels, and it forks to the side stream with the
    one C call only: under PNSFM_FAST_FORK=0 a weight gradient bound for the side stream takes the Python body, whose
    _WgradStream.run forks the torch way."""
    if want_w and not _FAST_FORK and _WgradStream.use_for(dy):
        return False
    return (not want_w or len(xs) == 1 or (cat_wgrad and get_conv_math() == 'bx3')) and (g_tap is None or get_conv_math() == 'bx3')


def _conv_bwd_plan(ctx, dy, xs, g_tap, x0):
    """What a stride-1 conv backward decides before it enqueues anything: ((sequencer, main raw stream, side raw stream, side Stream) or
    None for the Python body, need_dx, want_w, detached, weight slot, bias slot).  x0: position of the first source among the
    node's inputs (weight and bias are inputs 0 and 1 of both nodes)."""
    need_dx = any(ctx.needs_input_grad[x0:])
    want_w = bool(ctx.needs_input_grad[0] or (ctx.meta[3] and ctx.needs_input_grad[1]))
    detached = _WgradStream.side_ok(*ctx.params)
    sw, sb = _slots_for(ctx.params[0], ctx.params[1], detached and ctx.needs_input_grad[0])
    sq = _seq.get()
    seq = None
    if sq is not None and _seq_takes(dy, xs, want_w, ctx.cat_wgrad, g_tap):
        seq = (sq,) + _WgradStream.seq_fork(dy, want_w, detached)
    return seq, need_dx, want_w, detached, sw, sb


def _conv_bwd_python(ctx, dy, xs, wp_bwd, g_tap, need_dx, want_w, detached, sw, sb):
    """The Python body of a stride-1 conv backward from dy on: (gradient of the whole concatenation or None, dw, db)."""
    Cin, _, ks, has_bias = ctx.meta[:4]
    # (the multi-source envelope was decided at forward time under the arithmetic mode in force THEN; a set_conv_math('f32') between
    # forward and backward takes the multi-source kernel away -- ADVICE r04 -- so the mode is re-checked here)
    direct = len(xs) == 1 or (ctx.cat_wgrad and get_conv_math() == 'bx3')

    def wgrad():
        if len(xs) == 1:
            return ops.conv2d_backward_weight(xs[0], dy, ks, want_bias=has_bias, dw_out=sw, db_out=sb)
        if direct:
            return ops.conv2d_backward_weight_cat(xs, dy, ks, want_bias=has_bias, dw_out=sw, db_out=sb)
        # outside the multi-source weight-gradient kernel's envelope (decided once, in _cat_wgrad_ok): concatenate for this kernel
        return ops.conv2d_backward_weight(torch.cat(xs, 1), dy, ks, want_bias=has_bias, dw_out=sw, db_out=sb)

    # (pure: the closure launches kernels only -- the concatenating fallback calls torch.cat and takes the stream-context path)
    return _WgradStream.run_beside(dy, want_w, detached, wgrad, (lambda: _dgrad_tap(dy, wp_bwd, Cin, ks, g_tap)) if need_dx else None,
                                   (dy, *xs), pure=direct)


def _split_dx(dx, xs, needs):
    """The gradient of the whole concatenation as one channel slice (a view) per source that wants its gradient."""
    if dx is None:
        return (None,) * len(xs)
    if len(xs) == 1:
        return (dx,)
    dxs, c0 = [], 0
    for t, need in zip(xs, needs):
        dxs.append(dx[:, c0:c0 + t.shape[1]] if need else None)
        c0 += t.shape[1]
    return tuple(dxs)


class Conv2dFn(Function):
    """y = conv2d(zero_pad_{k//2}(cat(xs, 1)), weight) + bias, stride 1 (fp32 implicit GEMM on the matrix pipe; arithmetic: set_conv_math).
    xs: 1..3 tensors.  With several, the concatenation is folded into the K loop of the split-bf16 kernels (the decoder's skip
    connections, reference PackNet01.py:138-174): the concatenated tensor -- 254 MB for iconv1 at 192x640 batch 4 -- is neither written
    nor read.  Backward-data produces the gradient of the whole concatenation in one tensor; the inputs receive channel slices of it
    (views)."""

    @staticmethod
    def forward(ctx, weight, bias, cache, recording, cat_wgrad, tap, *xs):
        xs = tuple(t.contiguous() for t in xs)
        ctx.cat_wgrad = cat_wgrad
        need_dx = any(ctx.needs_input_grad[6:])
        wp_fwd, wp_bwd = cache.get(weight, need_dx)
        Cout, Cin, ks, _ = weight.shape
        if sum(t.shape[1] for t in xs) != Cin:
            if len(xs) == 1:
                raise RuntimeError("conv2d: input has %d channels, weight expects %d" % (xs[0].shape[1], Cin))
            raise RuntimeError("conv2d_cat: inputs have %d channels, weight expects %d" % (sum(t.shape[1] for t in xs), Cin))
        sq = _seq.get()
        if sq is not None:
            y = sq.conv2d_forward(list(xs), wp_fwd, bias, Cin, Cout, ks, ops.launch_stream_raw(xs[0].device))
        elif len(xs) == 1:
            y = ops.conv2d_forward(xs[0], wp_fwd, bias.detach() if bias is not None else None, Cout, ks)
        else:
            y = ops.conv2d_forward_cat(xs, wp_fwd, bias.detach() if bias is not None else None, Cout, ks)
        ctx.save_for_backward(wp_bwd if wp_bwd is not None else y.new_empty(0), *xs)
        ctx.meta = (Cin, Cout, ks, bias is not None)
        ctx.params = (weight, bias)
        _WgradStream.note_use(recording, weight, bias)
        # tap (single input only, see conv2d_tap): the input comes back as a second output; what its other consumers send back arrives
        # in backward as g_tap (None when nobody read the tap: no zero tensor is materialised) and is added inside the backward-data launch
        if tap:
            ctx.set_materialize_grads(False)
            return y, xs[0].view_as(xs[0])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, g_tap=None):
        if dy is None:         # only the tap was used: its gradient passes straight through
            return (None,) * 6 + (g_tap,)
        wp_bwd, *xs = ctx.saved_tensors
        Cin, Cout, ks, has_bias = ctx.meta
        dy = dy.contiguous()
        seq, need_dx, want_w, detached, sw, sb = _conv_bwd_plan(ctx, dy, xs, g_tap, 6)
        if seq is not None:
            sq, main_raw, side_raw, side = seq
            dx, dw, db = sq.conv2d_backward(dy, xs, wp_bwd, Cin, Cout, ks, has_bias, need_dx, want_w, sw, sb, g_tap, main_raw, side_raw,
                                            detached, side)
        else:
            dx, dw, db = _conv_bwd_python(ctx, dy, xs, wp_bwd, g_tap, need_dx, want_w, detached, sw, sb)
        return (dw, db, None, None, None, None) + _split_dx(dx, xs, ctx.needs_input_grad[6:])


def conv2d(x, weight, bias, cache):
    if x.dtype == torch.float16:
        return _conv2d_h16((x,), weight, bias, cache)
    _h16_input(x, weight)
    return Conv2dFn.apply(weight, bias, cache, torch.is_grad_enabled(), False, False, x)


class Conv2dRowsFn(Function):
    """The stride-1 convolution of the collapsed packing block's batched border strips, computed for the frame rows only.
    x: [2B, Cin, 2r, w], r = k // 2 -- the leading half the strips whose frame rows are their FIRST r rows (top / left), the trailing half
    those whose frame rows are their LAST r (bottom / right).  y: [2B, Cout, r, w] = the rows conv2d(x) would hold there (leading half:
    rows 0..r-1, trailing half: rows r..2r-1), element for element the same sums: the row-window kernels of include/pnsfm.h.  Backward:
    dx [2B, Cin, 2r, w] from the r rows of dy (no zero rows are staged), the weight gradient over dy's r rows, on the side stream like
    every other convolution's."""

    @staticmethod
    def forward(ctx, x, weight, bias, cache, r, recording=True, tapT=False, owner=None):
        x = x.contiguous()
        need_dx = ctx.needs_input_grad[0]
        wp_fwd, wp_bwd = cache.get(weight, need_dx, tapT=tapT)
        ctx.tapT, ctx.owner = tapT, (owner if recording else None)
        if ctx.owner is not None:
            ctx.owner.expect_node('c2')
        Cout, Cin, ks, _ = weight.shape
        if ks // 2 != r or x.shape[1] != Cin:
            raise RuntimeError("conv2d_rows: weight %s does not fit r = %d, input %s" % (tuple(weight.shape), r, tuple(x.shape)))
        y = ops.conv2d_forward_rows(x, wp_fwd, bias.detach() if bias is not None else None, Cout, ks, r)
        ctx.save_for_backward(x, wp_bwd if wp_bwd is not None else x.new_empty(0))
        ctx.meta = (Cin, Cout, ks, bias is not None, r)
        ctx.params = (weight, bias)
        _WgradStream.note_use(recording, weight, bias)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, wp_bwd = ctx.saved_tensors
        Cin, Cout, ks, has_bias, r = ctx.meta
        dy = dy.contiguous()
        want_w = bool(ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]))
        detached = _WgradStream.side_ok(*ctx.params)
        epi = ops.WGRAD_EPI_TAPT if ctx.tapT else 0      # (the gradient leaves in the weight's own layout either way)
        dgrad = (lambda: ops.conv2d_backward_data_rows(dy, wp_bwd, Cin, ks, r)) if ctx.needs_input_grad[0] else None
        own = ctx.owner
        if own is not None and own.begin():
            # the block's gradient owner: written / added into the parameter's one gradient tensor, left in flight on the side stream
            dwd, dbd, first = own.dest('c2')
            if not first:
                epi |= ops.WGRAD_EPI_ADD
            own.before(dy, _WgradStream.use_for(dy))
            dx, _, _ = _WgradStream.run_beside(
                dy, True, True, lambda: ops.conv2d_backward_weight_rows(x, dy, ks, r, want_bias=has_bias, dw_out=dwd, db_out=dbd, epi=epi),
                dgrad, (x, dy))
            dw, db = own.done('c2')
            return dx, dw, db, None, None, None, None, None
        sw, sb = _slots_for(ctx.params[0], ctx.params[1], detached and ctx.needs_input_grad[1])
        dx, dw, db = _WgradStream.run_beside(
            dy, want_w, detached, lambda: ops.conv2d_backward_weight_rows(x, dy, ks, r, want_bias=has_bias, dw_out=sw, db_out=sb, epi=epi),
            dgrad, (x, dy))
        return dx, dw, db, None, None, None, None, None


def conv2d_rows(x, weight, bias, cache, r, tapT=False, owner=None):
    """Frame rows of conv2d over the batched border strips (Conv2dRowsFn): x [2B, Cin, 2r, w] -> [2B, Cout, r, w].
    tapT: convolve with weight.transpose(2, 3), read in place (packer flag; the weight gradient comes back in weight's own layout).
    owner: the block's gradient owner (_PackGrads) or None."""
    if x.dtype == torch.float16:
        raise NotImplementedError("conv2d_rows: the fp16 forward keeps the full-strip form (conv2d + strip rows dropped at the paste)")
    _h16_input(x, weight)
    return Conv2dRowsFn.apply(x, weight, bias, cache, r, torch.is_grad_enabled(), tapT, owner)


# Round 5: gradient taps.  A tensor read by a convolution AND by something else (the encoder feature that is also a decoder skip input;
# the ResidualConv input read by conv1 and by the 1x1 shortcut; the decoder feature read by the next unpack block and by the InvDepth
# head) receives two gradients, which autograd adds with an elementwise kernel: 3 passes over the tensor and a launch, 18 times per
# PackNet01 step (1.2 GB).  conv2d_tap / conv2d_gn_act_tap return (y, x_tap): x_tap is x again, but as an OUTPUT of the convolution's
# node -- the other consumers read x_tap, their gradient comes back to the node as g_tap, and the convolution's backward-data launch
# adds it in its epilogue (ops.conv2d_backward_data(addend=...)): one read of the addend, no extra launch.  For a tensor with two
# consumers the bits are the untapped graph's (fl(acc + addend) either way); with three (ResidualConv input that is also a skip) the
# association differs from autograd's arrival order -- fixed, deterministic, inside every golden's tolerance.
# PNSFM_GRAD_TAPS=0 / set_grad_taps(False): plain graph.
_GRAD_TAPS = os.environ.get('PNSFM_GRAD_TAPS', '1') != '0'


def set_grad_taps(on):
    global _GRAD_TAPS
    _GRAD_TAPS = bool(on)


def grad_taps():
    return _GRAD_TAPS


def _dgrad_tap(dy, wp_bwd, Cin, ks, g_tap):
    """backward-data (+ the tap's gradient).  The tap was granted at forward time under the arithmetic mode in force then; should the
    mode have left 'bx3' since, the sum is formed the ordinary way instead of raising."""
    if g_tap is not None and get_conv_math() != 'bx3':
        return ops.conv2d_backward_data(dy, wp_bwd, Cin, ks) + g_tap
    return ops.conv2d_backward_data(dy, wp_bwd, Cin, ks, addend=g_tap)


def _tap_ok(weight):
    # the addend lives in the split-bf16 kernels' epilogue: backward-data's K is the layer's Cout
    return get_conv_math() == 'bx3' and weight.shape[0] >= 16


def conv2d_tap(x, weight, bias, cache):
    """(conv2d(x), x_tap)."""
    if x.dtype == torch.float16:
        return _conv2d_h16((x,), weight, bias, cache), x
    if not (_GRAD_TAPS and torch.is_grad_enabled() and x.requires_grad and _tap_ok(weight)):
        return conv2d(x, weight, bias, cache), x
    return Conv2dFn.apply(weight, bias, cache, True, False, True, x)


def _cat_fold_ok(xs):
    """May the concatenation of `xs` be folded into the K loop?  The envelope of the multi-source FORWARD kernel: 2 or 3 tensors, every
    one but the last ending on a 16-channel boundary, at least 16 channels in all, the split-bf16 arithmetic; the environment
    switch read here materialises every concatenation instead."""
    C0 = xs[0].shape[1]
    return os.environ.get('PNSFM_CAT_FOLD', '1') != '0' and len(xs) in (2, 3) and C0 % 16 == 0 and \
        (len(xs) == 2 or (C0 + xs[1].shape[1]) % 16 == 0) and get_conv_math() == 'bx3' and sum(t.shape[1] for t in xs) >= 16


def _cat_wgrad_ok(xs, weight):
    """May the multi-source weight-gradient kernels (wgrad3 / wgrad4, pnsfm_conv2d_backward_weight_cat) take these sources?  Their
    channel tiles are 32 wide (64 with two ci tiles per wave): every source but the last must end on such a boundary.  Decided ONCE
    per call here (the backward used to find out by catching every HipError, real launch failures included)."""
    return ops.conv2d_cat_wgrad_supported([t.shape[1] for t in xs], weight.shape[0], xs[0].shape[2], xs[0].shape[3], weight.shape[2],
                                          B=xs[0].shape[0])


def conv2d_cat(xs, weight, bias, cache):
    """xs: tuple of 2 or 3 NCHW tensors.  Falls back to torch.cat + conv2d when the shape is outside the multi-source FORWARD
    kernel's envelope (_cat_fold_ok); a shape the forward takes but the multi-source weight-gradient kernels do not concatenates for
    that one kernel only."""
    if xs[0].dtype == torch.float16:
        return _conv2d_h16(tuple(xs), weight, bias, cache)
    if not _cat_fold_ok(xs):
        return conv2d(torch.cat(xs, 1), weight, bias, cache)
    return Conv2dFn.apply(weight, bias, cache, torch.is_grad_enabled(), _cat_wgrad_ok(xs, weight), False, *xs)


class ConvGnActFn(Function):
    """act(GroupNorm_G(conv2d(zero_pad(cat(xs, 1)), weight) + bias)) as ONE autograd node (round 5): the reference's Conv2D block
    (layers01.py:28-37).  xs: 1..3 tensors (the decoder's concatenations stay folded into the K loop).  One node instead of two halves
    the autograd / Python overhead of the block (profiles/r05_host_profile.txt: ~35 us per Function.apply, the host needs 16-18 ms
    to enqueue a 24 ms step).
    Round 6: both bodies are ONE call into the block sequencer (csrc/seq/pnsfm_seq.cpp) when it is loaded.  (The conv epilogue that
    also left the GroupNorm statistics behind -- round 5, measured neutral twice, profiles/r05_ab_conv_gn_stats.txt -- is gone.)
    From the GroupNorm backward on, the backward is Conv2dFn's."""

    @staticmethod
    def forward(ctx, weight, bias, gamma, beta, cache, recording, cat_wgrad, G, eps, act, tap, *xs):
        xs = tuple(t.contiguous() for t in xs)
        ctx.cat_wgrad = cat_wgrad
        need_dx = any(ctx.needs_input_grad[11:])
        wp_fwd, wp_bwd = cache.get(weight, need_dx)
        Cout, Cin, ks, _ = weight.shape
        if sum(t.shape[1] for t in xs) != Cin:
            raise RuntimeError("conv_gn_act: inputs have %d channels, weight expects %d" % (sum(t.shape[1] for t in xs), Cin))
        bias_d = bias.detach() if bias is not None else None
        sq = _seq.get()
        if sq is not None:
            # ONE call: conv -> GroupNorm statistics -> normalise + activation (csrc/seq/pnsfm_seq.cpp)
            out, y, ms = sq.conv_gn_act_forward(list(xs), wp_fwd, bias_d, gamma, beta, Cin, Cout, ks, G, float(eps), act,
                                                ops.launch_stream_raw(xs[0].device))
        else:
            y = ops.conv2d_forward(xs[0], wp_fwd, bias_d, Cout, ks) if len(xs) == 1 else ops.conv2d_forward_cat(xs, wp_fwd, bias_d, Cout, ks)
            out, mean, rstd = ops.groupnorm_act_forward(y, None, gamma.detach(), beta.detach(), G, eps, act)
            ms = mean._base        # [mean | rstd]: one allocation (ops.groupnorm_act_forward)
        ctx.save_for_backward(wp_bwd if wp_bwd is not None else y.new_empty(0), y, gamma, beta, ms, *xs)
        ctx.meta = (Cin, Cout, ks, bias is not None, G, act)
        ctx.params = (weight, bias)
        _WgradStream.note_use(recording, weight, bias)
        # tap (single input only, see conv2d_tap): x comes back as a second output, its other consumers' gradient is added in backward-data
        if tap:
            ctx.set_materialize_grads(False)
            return out, xs[0].view_as(xs[0])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, g_tap=None):
        if dout is None:       # only the tap was used: its gradient passes straight through
            return (None,) * 11 + (g_tap,)
        wp_bwd, y, gamma, beta, ms, *xs = ctx.saved_tensors
        Cin, Cout, ks, has_bias, G, act = ctx.meta
        seq, need_dx, want_w, detached, sw, sb = _conv_bwd_plan(ctx, dout, xs, g_tap, 11)
        if seq is not None:
            # ONE call: GroupNorm backward -> fork -> weight gradient (side stream) -> backward-data (+ tap) [-> join]
            sq, main_raw, side_raw, side = seq
            dx, dw, db, dgamma, dbeta = sq.conv_gn_act_backward(dout, y, gamma, beta, ms, xs, wp_bwd, Cin, Cout, ks, G, act, has_bias, need_dx,
                                                                want_w, sw, sb, g_tap, main_raw, side_raw, detached, side)
        else:
            dy, dgamma, dbeta = ops.groupnorm_act_backward(dout.contiguous(), y, None, gamma.detach(), beta.detach(), ms[0], ms[1], G, act)
            dx, dw, db = _conv_bwd_python(ctx, dy, xs, wp_bwd, g_tap, need_dx, want_w, detached, sw, sb)
        return (dw, db, dgamma, dbeta, None, None, None, None, None, None, None) + _split_dx(dx, xs, ctx.needs_input_grad[11:])


_CONV_GN_FUSE = os.environ.get('PNSFM_CONV_GN_FUSE', '1') != '0'

def set_conv_gn_fuse(on):
    global _CONV_GN_FUSE
    _CONV_GN_FUSE = bool(on)


def conv2d_gn_act(x, weight, bias, gamma, beta, cache, G=16, eps=1e-5, act=ops.ACT_ELU):
    """The Conv2D block: x a tensor or a tuple of 2-3 tensors standing for their channel concatenation."""
    xs = tuple(x) if isinstance(x, (tuple, list)) else (x,)
    if xs[0].dtype == torch.float16:
        return _groupnorm_act_h16(_conv2d_h16(xs, weight, bias, cache), gamma, beta, G, eps, act)
    _h16_input(xs[0], weight)
    if len(xs) > 1 and not _cat_fold_ok(xs):
        xs = (torch.cat(xs, 1),)
    if not _CONV_GN_FUSE:
        y = conv2d(xs[0], weight, bias, cache) if len(xs) == 1 else conv2d_cat(xs, weight, bias, cache)
        return groupnorm_act(y, gamma, beta, G, eps, act)
    cat_wgrad = _cat_wgrad_ok(xs, weight) if len(xs) > 1 else False
    return ConvGnActFn.apply(weight, bias, gamma, beta, cache, torch.is_grad_enabled(), cat_wgrad, G, eps, act, False, *xs)


def conv2d_gn_act_tap(x, weight, bias, gamma, beta, cache, G=16, eps=1e-5, act=ops.ACT_ELU):
    """The Conv2D block with a gradient tap on its (single-tensor) input: (out, x_tap) -- see conv2d_tap."""
    if torch.is_tensor(x) and x.dtype == torch.float16:
        return conv2d_gn_act(x, weight, bias, gamma, beta, cache, G, eps, act), x
    if not (_GRAD_TAPS and _CONV_GN_FUSE and torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad and _tap_ok(weight)):
        return conv2d_gn_act(x, weight, bias, gamma, beta, cache, G, eps, act), x
    return ConvGnActFn.apply(weight, bias, gamma, beta, cache, True, False, G, eps, act, True, x)


class Conv2dStride2Fn(Function):
    """Stride-2 conv with zero padding k//2 (PoseNet).  Forward and weight-gradient run the strided MFMA kernels; the
    data-gradient is the stride-1 backward-data kernel on dy zero-upsampled onto the input grid."""

    @staticmethod
    def forward(ctx, x, weight, bias, cache, recording=True, wgrad_s1=False):
        x = x.contiguous()
        need_dx = ctx.needs_input_grad[0]
        wp_fwd, wp_bwd = cache.get(weight, need_dx)
        Cout, Cin, ks, _ = weight.shape
        y = ops.conv2d_forward_strided(x, wp_fwd, bias.detach() if bias is not None else None, Cout, ks, 2)
        ctx.save_for_backward(x, wp_bwd if wp_bwd is not None else x.new_empty(0))
        ctx.meta = (Cin, Cout, ks, bias is not None)
        # wgrad_s1: the weight gradient as the STRIDE-1 weight gradient of x with dy zero-upsampled onto the input grid (the tensor the
        # data gradient builds anyway) -- the same sums, the zeros adding nothing.  For wide layers on short maps (ResNet's layer{2,3,4}.0:
        # 256 -> 512 channels onto 6x20), whose patch the strided weight-gradient kernel cannot hold in LDS.
        ctx.wgrad_s1 = bool(wgrad_s1)
        ctx.params = (weight, bias)
        _WgradStream.note_use(recording, weight, bias)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, wp_bwd = ctx.saved_tensors
        Cin, Cout, ks, has_bias = ctx.meta
        dy = dy.contiguous()
        want_w = ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2])
        detached = _WgradStream.side_ok(*ctx.params)

        def upsampled():
            B, _, H, W = x.shape
            up = dy.new_zeros((B, Cout, H, W))
            up[:, :, ::2, ::2] = dy                      # dy[y][x] sits at (2y, 2x) of the input grid
            return up

        if ctx.wgrad_s1:
            up = upsampled()                             # once, for both gradients
            dx, dw, db = _WgradStream.run_beside(up, want_w, detached, lambda: ops.conv2d_backward_weight(x, up, ks, want_bias=has_bias),
                                                 (lambda: ops.conv2d_backward_data(up, wp_bwd, Cin, ks)) if ctx.needs_input_grad[0] else None,
                                                 (x, up))
            return dx, dw, db, None, None, None

        dx, dw, db = _WgradStream.run_beside(dy, want_w, detached, lambda: ops.conv2d_backward_weight_strided(x, dy, ks, 2, want_bias=has_bias),
                                             (lambda: ops.conv2d_backward_data(upsampled(), wp_bwd, Cin, ks)) if ctx.needs_input_grad[0] else None,
                                             (x, dy))
        return dx, dw, db, None, None, None


def conv2d_stride2(x, weight, bias, cache, wgrad_s1=False):
    return Conv2dStride2Fn.apply(x, weight, bias, cache, torch.is_grad_enabled(), wgrad_s1)


class GroupNormActFn(Function):
    """y = act(GroupNorm_G(x [+ res]))."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, G, eps, act):
        sq = _seq.get()
        if sq is not None:
            y, ms, x, res = sq.gn_act_forward(x, res, gamma, beta, G, float(eps), act, ops.launch_stream_raw(x.device))
        else:
            x = x.contiguous()
            res = res.contiguous() if res is not None else None
            y, mean, rstd = ops.groupnorm_act_forward(x, res, gamma.detach(), beta.detach(), G, eps, act)
            ms = mean._base
        ctx.save_for_backward(x, res if res is not None else x.new_empty(0), gamma, beta, ms)
        ctx.meta = (G, act, res is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, res, gamma, beta, ms = ctx.saved_tensors
        G, act, has_res = ctx.meta
        sq = _seq.get()
        if sq is not None:
            dx, dgamma, dbeta = sq.gn_act_backward(dy, x, res if has_res else None, gamma, beta, ms, G, act, ops.launch_stream_raw(x.device))
        else:
            dx, dgamma, dbeta = ops.groupnorm_act_backward(dy.contiguous(), x, res if has_res else None, gamma.detach(), beta.detach(),
                                                           ms[0], ms[1], G, act)
        return dx, (dx if has_res else None), dgamma, dbeta, None, None, None


def groupnorm_act(x, gamma, beta, G=16, eps=1e-5, act=ops.ACT_ELU, res=None):
    if x.dtype == torch.float16:
        return _groupnorm_act_h16(x, gamma, beta, G, eps, act, res)
    return GroupNormActFn.apply(x, res, gamma, beta, G, eps, act)


class SpaceToDepthFn(Function):
    @staticmethod
    def forward(ctx, x):
        return ops.space_to_depth(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return ops.depth_to_space(dy.contiguous())


class DepthToSpaceFn(Function):
    @staticmethod
    def forward(ctx, x):
        return ops.depth_to_space(x.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return ops.space_to_depth(dy)       # dy is often a channel slice (cat backward): handled without a copy


def space_to_depth(x):
    if x.dtype == torch.float16:
        return _h16_run(ops.space_to_depth_h16, x)
    return SpaceToDepthFn.apply(x)


def depth_to_space(x):
    if x.dtype == torch.float16:
        return _h16_run(lambda t: ops.depth_to_space_h16(t.contiguous()), x)
    return DepthToSpaceFn.apply(x)


class Conv3d1to8Fn(Function):
    """[B,D,H,W] -> [B,NF*D,H,W]: Conv3d(1,NF,3,pad 1) over (channel,y,x), channel index f*D+d; NF = 8 (PackNet01)
    or 4 (PackNetSlim01 / PackNetSAN01)."""

    @staticmethod
    def forward(ctx, p, w3, b3, recording=True):
        p = p.contiguous()
        out = ops.conv3d_forward(p, w3.detach().contiguous(), b3.detach().contiguous())
        ctx.save_for_backward(p, w3)
        ctx.params = (w3, b3)
        _WgradStream.note_use(recording, w3, b3)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        p, w3 = ctx.saved_tensors
        dout = dout.contiguous()
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        detached = _WgradStream.side_ok(*ctx.params)
        dp, dw3, db3 = _WgradStream.run_beside(dout, want_w, detached, lambda: ops.conv3d_backward_weight(p, dout),
                                               (lambda: ops.conv3d_backward_data(dout, w3.detach().contiguous())) if ctx.needs_input_grad[0] else None,
                                               (p, dout))
        return dp, dw3, db3, None


def conv3d_1to8(p, w3, b3):
    if p.dtype == torch.float16:
        _h16_params(w3, b3)
        return _h16_run(lambda p, w, b: ops.conv3d_forward_h16(p.contiguous(), w.detach().contiguous(), None if b is None else b.detach()),
                        p, w3, b3)
    _h16_input(p, w3)
    return Conv3d1to8Fn.apply(p, w3, b3, torch.is_grad_enabled())


class Conv3dD2sFn(Function):
    """depth_to_space(Conv3d1to8Fn(p)) of the unpacking block as one node: [B,D,H,W] -> [B,NF*D/4,2H,2W].  The stencil writes the
    shuffled layout (csrc/pack3d.hip: conv3d_fwd_x4_d2s_kernel), so the forward shuffle and the [B,NF*D,H,W] tensor do not exist where
    the fold applies; elsewhere (and with PNSFM_PACK3D_FOLD=0) the entry point runs the two kernels.  Backward is the two nodes':
    space_to_depth of the gradient, then the stencil's gradients.  Bit-identical to the two nodes either way."""

    @staticmethod
    def forward(ctx, p, w3, b3, recording=True):
        p = p.contiguous()
        y = ops.conv3d_forward_d2s(p, w3.detach().contiguous(), b3.detach().contiguous())
        ctx.save_for_backward(p, w3)
        ctx.params = (w3, b3)
        _WgradStream.note_use(recording, w3, b3)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        p, w3 = ctx.saved_tensors
        dout = ops.space_to_depth(dy)       # dy is often a channel slice (cat backward): handled without a copy
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        detached = _WgradStream.side_ok(*ctx.params)
        dp, dw3, db3 = _WgradStream.run_beside(dout, want_w, detached, lambda: ops.conv3d_backward_weight(p, dout),
                                               (lambda: ops.conv3d_backward_data(dout, w3.detach().contiguous())) if ctx.needs_input_grad[0] else None,
                                               (p, dout))
        return dp, dw3, db3, None


def conv3d_1to8_d2s(p, w3, b3):
    """depth_to_space(conv3d_1to8(p, w3, b3))."""
    if p.dtype == torch.float16:
        return depth_to_space(conv3d_1to8(p, w3, b3))
    _h16_input(p, w3)
    return Conv3dD2sFn.apply(p, w3, b3, torch.is_grad_enabled())


class ComposePackWeightFn(Function):
    """W_eff = Conv3d(1->8) composed with the Conv2d that follows it inside PackLayerConv3d (no non-linearity between
    them, reference layers01.py:243-246):

        W_eff[co, ci, U, V] = sum_{f,dz,dy,dx} W3[f,dz,dy,dx] * W2[co, f*D + (ci-dz+1), U-dy, V-dx]       (k -> k+2 taps)

    which is exactly the backward-data stencil of the Conv3d applied to the zero-ring-padded W2, so the gfx950 conv3d
    kernels do the composition and its two gradients (dW2 = forward stencil of dW_eff, dW3 = weight-gradient stencil)."""

    @staticmethod
    def forward(ctx, W2, W3, recording=True):
        w3 = W3.detach().contiguous()
        ctx.ring = _ring_on()
        if ctx.ring:                                                                  # the ring of zeros is implicit (ComposePackParamsFn)
            W2pad = W2.detach().contiguous()                                          # [C, 8D, k, k]
            Weff = ops.conv3d_backward_data_ring(W2pad, w3)                           # [C, D, k+2, k+2]
        else:
            W2pad = torch.nn.functional.pad(W2.detach(), (1, 1, 1, 1)).contiguous()  # [C, 8D, k+2, k+2]
            Weff = ops.conv3d_backward_data(W2pad, w3)
        ctx.save_for_backward(W2pad, w3)
        ctx.params = (W2, W3)
        _WgradStream.note_use(recording, W2, W3)
        return Weff

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        W2pad, w3 = ctx.saved_tensors
        g = g.contiguous()
        _WgradStream.side_ok(*ctx.params)            # bookkeeping only: this node always runs on the compute stream
        dW2 = dW3 = None
        if ctx.needs_input_grad[0]:
            dW2 = ops.conv3d_forward(g, w3, torch.zeros(w3.shape[0], device=g.device, dtype=g.dtype))[:, :, 1:-1, 1:-1].contiguous()
        if ctx.needs_input_grad[1]:
            dW3, _ = ops.conv3d_backward_weight_ring(g, W2pad) if ctx.ring else ops.conv3d_backward_weight(g, W2pad)
        return dW2, dW3, None


def compose_pack_weight(W2, W3):
    return ComposePackWeightFn.apply(W2, W3, torch.is_grad_enabled())


# The weight path of the collapsed packing block without ATen passes (PNSFM_PACK_WPATH=0 / set_pack_wpath(False): the former path, the
# A/B switch and the reference of tests/pack_wpath_cases.py).  The kernel composition and its Conv3d weight gradient read
# the Conv2d weight itself -- the zero ring around its taps is the stencil kernels' window check, not a padded copy (a fill and a copy
# of [C, d*D, k+2, k+2] per block and step, and twice the bytes under both stencils); the column strips read the transposed taps of W2 /
# W3 in place (packer and stencil flags) instead of materialised transposes; and the block's four parameters have one gradient owner
# (_PackGrads) whose contributions meet inside the weight-gradient kernels' epilogues instead of in autograd's adds.  Bit-identical.
_PACK_WPATH = os.environ.get('PNSFM_PACK_WPATH', '1') != '0'


def set_pack_wpath(on):
    """Returns the previous setting."""
    global _PACK_WPATH
    prev, _PACK_WPATH = _PACK_WPATH, bool(on)
    return prev


def _ring_on():
    return _PACK_WPATH and ops.conv3d_ring_ok()


class ComposePackParamsFn(Function):
    """(W_eff, bias_eff) of the composed packing convolution in one node: ComposePackWeightFn's composition plus

        bias_eff[co] = b2[co] + sum_f b3[f] * sum_{ci,taps} W2[co, f*D + ci, taps]

    (a Conv3d bias is a constant plane, which the Conv2d turns into a per-channel constant away from the border).  One node instead
    of two plus a chain of reshape / sum / mul / add: forward = composition stencil (on W2 inside an implicit ring of zeros; under
    PNSFM_PACK_WPATH=0 on a padded copy), one bias kernel; backward = the two stencils and two small kernels that also fold the bias
    path's rank-one term into dW2 (no second gradient to accumulate)."""

    @staticmethod
    def forward(ctx, W2, b2, W3, b3, recording=True, owner=None):
        W2d, w3, b3d = W2.detach().contiguous(), W3.detach().contiguous(), b3.detach().contiguous()
        ctx.ring = _ring_on()
        ctx.owner = owner if (recording and ctx.ring) else None
        if ctx.owner is not None:
            ctx.owner.expect_node('c2', 'c3')
        if ctx.ring:
            W2src = W2d                                                               # [C, d*D, k, k]: the ring is never stored
            Weff = ops.conv3d_backward_data_ring(W2d, w3)                             # [C, D, k+2, k+2]
        else:
            W2src = torch.nn.functional.pad(W2d, (1, 1, 1, 1))                        # [C, d*D, k+2, k+2]
            Weff = ops.conv3d_backward_data(W2src, w3)
        bias_eff, Ssum = ops.pack_bias_eff_forward(W2d, None if b2 is None else b2.detach().contiguous(), b3d)
        ctx.save_for_backward(W2src, w3, b3d, Ssum)
        ctx.params = (W2, W3)
        ctx.k = W2.shape[-1]
        _WgradStream.note_use(recording, W2, W3)
        return Weff, bias_eff

    @staticmethod
    @once_differentiable
    def backward(ctx, gW, gb):
        W2src, w3, b3, Ssum = ctx.saved_tensors
        _WgradStream.side_ok(*ctx.params)            # bookkeeping only: this node always runs on the compute stream
        need_W2, need_b2, need_W3, need_b3 = ctx.needs_input_grad[:4]
        C, k = W2src.shape[0], ctx.k
        if gW is None:
            gW = W2src.new_zeros((C, W2src.shape[1] // w3.shape[0], k + 2, k + 2))
        if gb is None:
            gb = W2src.new_zeros((C,))
        gW, gb = gW.contiguous(), gb.contiguous()
        dW2 = dW3 = db3 = None
        own = ctx.owner
        if own is not None and own.begin():
            # the block's gradient owner (_PackGrads): this node's gradients join the strips' inside its kernels; it runs on the compute
            # stream, behind the strips' contributions on the side stream
            dW2d, db2d, first2 = own.dest('c2')
            dW3d, db3d, first3 = own.dest('c3')
            own.before(gW, False)
            if first2 or first3:
                # (the composition is the block's first node and therefore the last of its backward pass: both strips have contributed)
                raise RuntimeError("collapsed packing block: the composition's backward ran before the border strips'")
            full = ops.conv3d_forward(gW, w3, None)
            ops.pack_bias_eff_backward_add(gb, Ssum, b3, full, k, db3d, dW2d, db2d)
            ops.conv3d_backward_weight_ring(gW, W2src, dw3_out=dW3d, db3_out=None, epi=ops.WGRAD_EPI_ADD)
            dW2, db2 = own.done('c2')
            dW3, db3 = own.done('c3')
            return dW2, db2, dW3, db3, None, None
        if need_W2 or need_b3:
            # the composition's gradient on the padded taps; cropped and completed by the bias path's term in the same kernel
            # (not wanted: a tensor of the right shape that the kernel does not read)
            full = ops.conv3d_forward(gW, w3, None) if need_W2 else W2src.new_empty((C, W2src.shape[1], k + 2, k + 2))
            db3, dW2 = ops.pack_bias_eff_backward(gb, Ssum, b3, full, k, want_db3=need_b3, want_dW2=need_W2)
        if need_W3:
            dW3, _ = ops.conv3d_backward_weight_ring(gW, W2src) if ctx.ring else ops.conv3d_backward_weight(gW, W2src)
        return dW2, (gb if need_b2 else None), dW3, db3, None, None


def compose_pack_params(W2, b2, W3, b3, owner=None):
    return ComposePackParamsFn.apply(W2, b2, W3, b3, torch.is_grad_enabled(), owner)


def _R(op, dst, src=None):
    return (op, dst, src)


# Forward bodies of the collapsed packing block's three strip Functions, shared with the fp16 forward: `run` is ops.region_ops (fp32)
# or ops.region_ops_h16 (fp16 windows) -- one list of windows for both.
def _border_split_fwd(P, S, lr_t, run):
    B, C, h, w = P.shape
    tb = P.new_empty((2 * B, C, S, w))
    # lr_t (round 6): the column strips are stored TRANSPOSED, [2B, C, S, h] -- rows of h pixels instead of rows of S = 3 / 5 --
    # so that every kernel behind them (Conv3d stencil, convolution, weight gradient) sees a map as wide as the row strips'
    lr = P.new_empty((2 * B, C, S, h)) if lr_t else P.new_empty((2 * B, C, h, S))
    lrv = lr.transpose(2, 3) if lr_t else lr
    run([_R(ops.REGION_COPY, tb[:B], P[:, :, :S]), _R(ops.REGION_COPY, tb[B:], P[:, :, h - S:]),
         _R(ops.REGION_COPY, lrv[:B], P[:, :, :, :S]), _R(ops.REGION_COPY, lrv[B:], P[:, :, :, w - S:])])
    return tb, lr


def _strip_select_fwd(z, B, r, dim, run):
    n2 = 2 * r
    if dim == 2:
        out = z.new_empty((z.shape[0], z.shape[1], n2, z.shape[3]))
        run([_R(ops.REGION_COPY, out[:B], z[:B, :, :n2]), _R(ops.REGION_COPY, out[B:], z[B:, :, 1:])])
    else:
        out = z.new_empty((z.shape[0], z.shape[1], z.shape[2], n2))
        run([_R(ops.REGION_COPY, out[:B], z[:B, :, :, :n2]), _R(ops.REGION_COPY, out[B:], z[B:, :, :, 1:])])
    return out


def _border_paste_fwd(y, o_tb, o_lr, r, lr_t, run, rows=False):
    """Pastes in place into y; o_tb / o_lr contiguous.  Returns y.  rows: the strip results hold their frame rows only (conv2d_rows):
    o_tb [2B, C, r, w] and, transposed, o_lr [2B, C, r, h]; untransposed column strips keep their 2r columns."""
    B, h, w = y.shape[0], y.shape[2], y.shape[3]
    if lr_t:                     # [2B, C, 2r | r, h] holds the column strips transposed
        o_lr = o_lr.transpose(2, 3)
    t0 = 0 if rows else r                      # first frame row of the trailing half of o_tb
    c0 = 0 if (rows and lr_t) else r           # ... frame column of o_lr
    run([_R(ops.REGION_COPY, y[:, :, r:h - r, :r], o_lr[:B, :, r:h - r, :r]),
         _R(ops.REGION_COPY, y[:, :, r:h - r, w - r:], o_lr[B:, :, r:h - r, c0:]),
         _R(ops.REGION_COPY, y[:, :, :r], o_tb[:B, :, :r]),
         _R(ops.REGION_COPY, y[:, :, h - r:], o_tb[B:, :, t0:])])
    return y


class PackBorderSplitFn(Function):
    """Collapsed packing block, input side: P -> (P itself for the interior convolution, the top+bottom row strips,
    the left+right column strips; strips batched along dim 0).  Plain slicing would make autograd zero-fill and add a
    full-size dP four times (slice_backward); here the strip gradients are added straight into the interior path's dP.
    Round 4: the four strip gathers are ONE launch (ops.region_ops), and so are the four gradient accumulations."""

    @staticmethod
    def forward(ctx, P, S, lr_t=False):
        ctx.S, ctx.lr_t = S, lr_t
        tb, lr = _border_split_fwd(P, S, lr_t, ops.region_ops)
        return P.view_as(P), tb, lr

    @staticmethod
    @once_differentiable
    def backward(ctx, dP, d_tb, d_lr):
        S = ctx.S
        if dP is None:
            raise RuntimeError('pack_border_split: the interior path must be used')
        dP = dP.contiguous()        # the interior conv's freshly written backward-data buffer: accumulate in place
        B, h, w = dP.shape[0], dP.shape[2], dP.shape[3]
        # (the row strips and the column strips overlap in the corners: two launches keep every destination single-writer per launch)
        # (... and when the map is smaller than two strips -- S <= h < 2S -- the leading and the trailing strip overlap too: the
        # operations of ONE region_ops launch must not share destinations (include/pnsfm.h), so those run as separate launches)
        def add_pair(a, b, overlap):
            if overlap:
                ops.region_ops([a])
                ops.region_ops([b])
            else:
                ops.region_ops([a, b])
        if d_tb is not None:
            d_tb = d_tb.contiguous()
            add_pair(_R(ops.REGION_ADD, dP[:, :, :S], d_tb[:B]), _R(ops.REGION_ADD, dP[:, :, h - S:], d_tb[B:]), h < 2 * S)
        if d_lr is not None:
            d_lr = d_lr.contiguous()
            if ctx.lr_t:
                d_lr = d_lr.transpose(2, 3)
            add_pair(_R(ops.REGION_ADD, dP[:, :, :, :S], d_lr[:B]), _R(ops.REGION_ADD, dP[:, :, :, w - S:], d_lr[B:]), w < 2 * S)
        return dP, None, None


def pack_border_split(P, S, lr_t=False):
    if P.dtype == torch.float16:
        return (P,) + tuple(_h16_run(lambda P: _border_split_fwd(P, S, lr_t, ops.region_ops_h16), P))
    return PackBorderSplitFn.apply(P, S, lr_t)


class StripSelectFn(Function):
    """z: [2B, C, S, w] (dim=2) or [2B, C, h, S] (dim=3), the Conv3d of the batched strips.  Keeps the 2r rows/cols whose
    Conv3d neighbourhood lies inside the strip: the first 2r of the leading half, the last 2r of the trailing half.
    Backward writes every element of dz exactly once (no zero-fill + copy).  One launch each way (ops.region_ops)."""

    @staticmethod
    def forward(ctx, z, B, r, dim):
        ctx.meta = (B, r, dim, tuple(z.shape))
        return _strip_select_fwd(z, B, r, dim, ops.region_ops)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, r, dim, shape = ctx.meta
        g = g.contiguous()
        dz = g.new_empty(shape)
        n2 = 2 * r
        if dim == 2:
            ops.region_ops([_R(ops.REGION_COPY, dz[:B, :, :n2], g[:B]), _R(ops.REGION_ZERO, dz[:B, :, n2:]),
                            _R(ops.REGION_COPY, dz[B:, :, 1:], g[B:]), _R(ops.REGION_ZERO, dz[B:, :, :1])])
        else:
            ops.region_ops([_R(ops.REGION_COPY, dz[:B, :, :, :n2], g[:B]), _R(ops.REGION_ZERO, dz[:B, :, :, n2:]),
                            _R(ops.REGION_COPY, dz[B:, :, :, 1:], g[B:]), _R(ops.REGION_ZERO, dz[B:, :, :, :1])])
        return dz, None, None, None


def strip_select(z, B, r, dim):
    if z.dtype == torch.float16:
        return _h16_run(lambda z: _strip_select_fwd(z, B, r, dim, ops.region_ops_h16), z)
    return StripSelectFn.apply(z, B, r, dim)


class Conv3dStripRowsFn(Function):
    """StripSelectFn(Conv3d1to8Fn(p), B, r, 2) as one node: the stencil computes and stores only the 2r rows the selection keeps, and
    its gradients read the 2r-row gradient at its place in the S-row frame (csrc/pack3d.hip, C3dRows) -- the copy that dropped one
    row of S, and the copy + zero-fill of its backward, do not exist.  Bit-identical to the two nodes."""

    @staticmethod
    def forward(ctx, p, w3, b3, B, recording=True, tapT=False, owner=None):
        out = ops.conv3d_forward_rows(p, w3.detach().contiguous(), b3.detach().contiguous(), B, tapT=tapT)
        ctx.save_for_backward(p, w3)
        ctx.params, ctx.B = (w3, b3), B
        ctx.tapT, ctx.owner = tapT, (owner if recording else None)
        if ctx.owner is not None:
            ctx.owner.expect_node('c3')
        _WgradStream.note_use(recording, w3, b3)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        p, w3 = ctx.saved_tensors
        B, S = ctx.B, p.shape[2]
        dout = dout.contiguous()
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        detached = _WgradStream.side_ok(*ctx.params)
        tapT = ctx.tapT
        epi = ops.WGRAD_EPI_TAPT if tapT else 0      # (the gradient leaves in w3's own layout either way)
        dgrad = (lambda: ops.conv3d_backward_data_rows(dout, w3.detach().contiguous(), S, B, tapT=tapT)) if ctx.needs_input_grad[0] else None
        own = ctx.owner
        if own is not None and own.begin():      # the block's gradient owner: see Conv2dRowsFn.backward
            dwd, dbd, first = own.dest('c3')
            if not first:
                epi |= ops.WGRAD_EPI_ADD
            own.before(p, _WgradStream.use_for(p))
            dp, _, _ = _WgradStream.run_beside(p, True, True, lambda: ops.conv3d_backward_weight_rows(p, dout, B, dw3_out=dwd, db3_out=dbd, epi=epi),
                                               dgrad, (p, dout))
            dw3, db3 = own.done('c3')
            return dp, dw3, db3, None, None, None, None
        # (p: the side-stream rule goes by the pixel count of the S-row frame, as in Conv3d1to8Fn)
        dp, dw3, db3 = _WgradStream.run_beside(p, want_w, detached, lambda: ops.conv3d_backward_weight_rows(p, dout, B, epi=epi), dgrad, (p, dout))
        return dp, dw3, db3, None, None, None, None


def conv3d_1to8_rows(p, w3, b3, B, r, tapT=False, owner=None):
    """strip_select(conv3d_1to8(p, w3, b3), B, r, 2) of the border strips p [2B, D, 2r + 1, w].
    tapT: with w3.transpose(3, 4), read in place (row-window kernels only); owner: the block's gradient owner (_PackGrads) or None."""
    if p.dtype != torch.float16 and p.shape[2] == 2 * r + 1:
        p = p.contiguous()
        if ops.conv3d_rows_folded(p):
            _h16_input(p, w3)
            return Conv3dStripRowsFn.apply(p, w3, b3, B, torch.is_grad_enabled(), tapT, owner)
    if tapT or owner is not None:
        raise RuntimeError("conv3d_1to8_rows: transposed taps and gradient owners run on the row-window kernels only")
    return strip_select(conv3d_1to8(p, w3, b3), B, r, 2)


class PackBorderPasteFn(Function):
    """Collapsed packing block, output side: overwrite the r-pixel frame of the interior result y (in place: y is the
    interior conv's own output buffer) with the strip results o_tb [2B,C,2r,w] / o_lr [2B,C,h,2r] (only their outer r
    rows / columns are valid).  Replaces two torch.cat copies forward and a zero-fill + copy backward; one launch forward, one
    backward (every element of d_tb, d_lr and dy has exactly one writer).
    rows: the strips were convolved for their frame rows only (conv2d_rows) -- o_tb [2B,C,r,w], o_lr transposed [2B,C,r,h]: their
    gradients hold the frame rows and nothing else, so backward zero-fills no inner rows (only the corners of d_lr, which belong to
    the row strips)."""

    @staticmethod
    def forward(ctx, y, o_tb, o_lr, r, lr_t=False, rows=False):
        ctx.r, ctx.lr_t, ctx.rows = r, lr_t, rows
        o_tb, o_lr = o_tb.contiguous(), o_lr.contiguous()
        s_lr = tuple(o_lr.shape)
        _border_paste_fwd(y, o_tb, o_lr, r, lr_t, ops.region_ops, rows)
        ctx.mark_dirty(y)
        ctx.shapes = (tuple(o_tb.shape), s_lr)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        r = ctx.r
        g = g.contiguous()
        B, h, w = g.shape[0], g.shape[2], g.shape[3]
        s_tb, s_lr = ctx.shapes
        d_tb, d_lr_st, dy = g.new_empty(s_tb), g.new_empty(s_lr), torch.empty_like(g)
        d_lr = d_lr_st.transpose(2, 3) if ctx.lr_t else d_lr_st
        dy_ops = [
            # dy: the interior of g, frame zero (the frame's gradient belongs to the strips)
            _R(ops.REGION_COPY, dy[:, :, r:h - r, r:w - r], g[:, :, r:h - r, r:w - r]),
            _R(ops.REGION_ZERO, dy[:, :, :r]), _R(ops.REGION_ZERO, dy[:, :, h - r:]),
            _R(ops.REGION_ZERO, dy[:, :, r:h - r, :r]), _R(ops.REGION_ZERO, dy[:, :, r:h - r, w - r:])]
        if ctx.rows:
            lr_rows = ctx.lr_t        # (untransposed column strips keep 2r columns: their inner r are zero-filled as before)
            lr_ops = [_R(ops.REGION_COPY, d_lr[:B, :, r:h - r, :r], g[:, :, r:h - r, :r]),
                      _R(ops.REGION_COPY, d_lr[B:, :, r:h - r, (0 if lr_rows else r):], g[:, :, r:h - r, w - r:]),
                      _R(ops.REGION_ZERO, d_lr[:, :, :r]), _R(ops.REGION_ZERO, d_lr[:, :, h - r:])]
            if not lr_rows:
                lr_ops += [_R(ops.REGION_ZERO, d_lr[:B, :, r:h - r, r:]), _R(ops.REGION_ZERO, d_lr[B:, :, r:h - r, :r])]
            # d_tb [2B,C,r,w]: the frame rows of g; one launch covers d_tb, dy and d_lr (<= 12 windows, every element one writer)
            ops.region_ops([_R(ops.REGION_COPY, d_tb[:B], g[:, :, :r]), _R(ops.REGION_COPY, d_tb[B:], g[:, :, h - r:])] + dy_ops + lr_ops)
            return dy, d_tb, d_lr_st, None, None, None
        ops.region_ops([
            # d_tb [2B,C,2r,w]: leading half rows 0..r-1 <- top frame, rows r.. zero; trailing half rows r.. <- bottom frame, rows ..r-1 zero
            _R(ops.REGION_COPY, d_tb[:B, :, :r], g[:, :, :r]), _R(ops.REGION_ZERO, d_tb[:B, :, r:]),
            _R(ops.REGION_COPY, d_tb[B:, :, r:], g[:, :, h - r:]), _R(ops.REGION_ZERO, d_tb[B:, :, :r])] + dy_ops)
        ops.region_ops([
            # d_lr [2B,C,h,2r]: only rows r..h-r-1 of the outer r columns carry gradient (the corners went to the row strips)
            _R(ops.REGION_COPY, d_lr[:B, :, r:h - r, :r], g[:, :, r:h - r, :r]), _R(ops.REGION_ZERO, d_lr[:B, :, r:h - r, r:]),
            _R(ops.REGION_COPY, d_lr[B:, :, r:h - r, r:], g[:, :, r:h - r, w - r:]), _R(ops.REGION_ZERO, d_lr[B:, :, r:h - r, :r]),
            _R(ops.REGION_ZERO, d_lr[:, :, :r]), _R(ops.REGION_ZERO, d_lr[:, :, h - r:])])
        return dy, d_tb, d_lr_st, None, None, None


def pack_border_paste(y, o_tb, o_lr, r, lr_t=False, rows=False):
    if y.dtype == torch.float16:
        if torch.is_grad_enabled() and any(t.requires_grad for t in (y, o_tb, o_lr)):
            raise NotImplementedError(_H16_ONLY_FWD)      # (in place into y: the collapsed fp16 block runs it inside its forward-only node)
        return _border_paste_fwd(y, o_tb.contiguous(), o_lr.contiguous(), r, lr_t, ops.region_ops_h16, rows)
    return PackBorderPasteFn.apply(y, o_tb, o_lr, r, lr_t, rows)


class InvDepthActFn(Function):
    @staticmethod
    def forward(ctx, x, min_depth):
        y = ops.invdepth_act_forward(x.contiguous(), min_depth)
        ctx.save_for_backward(y)
        ctx.min_depth = min_depth
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.invdepth_act_backward(dy.contiguous(), y, ctx.min_depth), None


def invdepth_act(x, min_depth):
    return InvDepthActFn.apply(x, min_depth)


class InvDepthConvFn(Function):
    """y = sigmoid(conv3x3(zero_pad1(x), w) + b) / min_depth with ONE output channel (the InvDepth head), fused."""

    @staticmethod
    def forward(ctx, x, weight, bias, min_depth):
        x = x.contiguous()
        w = weight.detach().contiguous()
        y = ops.invdepth_conv_forward(x, w, bias.detach(), min_depth)
        ctx.save_for_backward(x, w, y)
        ctx.min_depth = min_depth
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dz = ops.invdepth_act_backward(dy.contiguous(), y, ctx.min_depth)
        dx, dw, db = ops.invdepth_conv_backward(x, w, dz)
        return dx, dw, db, None


def invdepth_conv(x, weight, bias, min_depth):
    if x.dtype == torch.float16:
        _h16_params(weight, bias)
        return _h16_run(lambda x, w, b: ops.invdepth_conv_forward_h16(x.contiguous(), w.detach().contiguous(), b.detach(), min_depth),
                        x, weight, bias)
    _h16_input(x, weight)
    return InvDepthConvFn.apply(x, weight, bias, min_depth)


class PoseVec2MatFn(Function):
    """[N,6] (tx,ty,tz,rx,ry,rz) -> [N,4,4] rigid transforms, R = Rx*Ry*Rz (euler)."""

    @staticmethod
    def forward(ctx, vec):
        vec = vec.contiguous()
        ctx.save_for_backward(vec)
        return ops.pose_vec2mat_forward(vec)

    @staticmethod
    @once_differentiable
    def backward(ctx, dmat):
        (vec,) = ctx.saved_tensors
        return ops.pose_vec2mat_backward(vec, dmat.contiguous())


def pose_vec2mat44(vec):
    return PoseVec2MatFn.apply(vec)


class UpsampleNearestFn(Function):
    """Nearest-neighbour up-sampling by an integer factor (F.interpolate(mode='nearest') / nn.Upsample of the reference:
    models/model_utils.py:163-180, networks/depth/PackNet01.py:87-89); backward = s x s block sums."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return ops.upsample_nearest_forward(x.contiguous(), s)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return ops.upsample_nearest_backward(dy.contiguous(), ctx.s), None


def upsample_nearest(x, size=None, scale_factor=None):
    """x [B,C,h,w] up-sampled (nearest) to `size` = (H, W) or by `scale_factor`.  Integer factors of fp32 device maps run the gfx950
    kernel (factor 1: the tensor itself); anything else is torch's interpolate (same index rule for integer factors)."""
    h, w = x.shape[-2:]
    if size is not None:
        H, W = int(size[-2]), int(size[-1])
    else:
        H, W = int(h * scale_factor), int(w * scale_factor)
    s = H // h if h else 0
    from . import _lib
    if x.dtype == torch.float16 and s >= 1 and (H, W) == (h * s, w * s) and (W % 4) == 0:
        return x if s == 1 else _h16_run(lambda t: ops.upsample_nearest_forward_h16(t.contiguous(), s), x)
    if s >= 1 and (H, W) == (h * s, w * s) and (x.is_cuda or not _lib.REQUIRE_CUDA) and ops.upsample_nearest_ok(x, s):
        return x if s == 1 else UpsampleNearestFn.apply(x, s)
    if size is not None:
        return torch.nn.functional.interpolate(x, size=(H, W), mode='nearest')
    return torch.nn.functional.interpolate(x, scale_factor=scale_factor, mode='nearest')


# ---- ResNet networks (csrc/resnet.h): dense BatchNorm (+ residual, ReLU), max pooling, reflection pad, activation + crop -----------------
_RESNET_NO_H16 = ("%s has no fp16 kernel: in the fp16 forward (evaluation / inference) the BatchNorm, the reflection pad, the crop with "
                  "its activation and the input affine live inside the convolution (conv2d_h16_fused); run this op in float32")


def _no_h16(what, *tensors):
    if any(t is not None and t.dtype == torch.float16 for t in tensors):
        raise NotImplementedError(_RESNET_NO_H16 % what)


class BatchNormActFn(Function):
    """y = act(BatchNorm(x) + res), act in {ACT_NONE, ACT_RELU}: nn.BatchNorm2d and the `out += identity; relu(out)` of torchvision's
    BasicBlock in one launch (two on large maps).  Training mode updates running_mean / running_var / num_batches_tracked on the device.
    Saved for backward: x, the output y (which the next layer holds anyway) and the [2, C] float64 batch statistics."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, act, training):
        x = x.contiguous()
        res = res.contiguous() if res is not None else None
        y, stats = ops.batchnorm_act_forward(x, res, gamma.detach(), beta.detach(), running_mean, running_var, num_batches_tracked, eps,
                                             momentum, act, training)
        ctx.save_for_backward(x, y, gamma, stats if stats is not None else x.new_empty(0))
        ctx.running = None if training else (running_mean, running_var)
        ctx.meta = (eps, act, res is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, gamma, stats = ctx.saved_tensors
        eps, act, has_res = ctx.meta
        rm, rv = ctx.running if ctx.running is not None else (None, None)
        dy = dy.contiguous()
        want_dres = has_res and ctx.needs_input_grad[1]
        dx, dres, dgamma, dbeta = ops.batchnorm_act_backward(dy, y, x, gamma.detach(), stats if ctx.running is None else None, rm, rv, eps, act,
                                                             want_dres)
        if want_dres and dres is None:
            dres = dy                       # no activation: the residual's gradient is the upstream gradient itself
        return dx, (dres if want_dres else None), dgamma, dbeta, None, None, None, None, None, None, None


def batchnorm_act(x, bn, act=ops.ACT_NONE, res=None):
    """act(bn(x) + res) for an nn.BatchNorm2d `bn` (a parameter and buffer container: its own forward is not called)."""
    _no_h16('batchnorm_act', x, res, bn.weight)
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("batchnorm_act: BatchNorm2d(affine=True, track_running_stats=True, momentum=<float>) only")
    return BatchNormActFn.apply(x, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum,
                                act, bn.training)


class MaxPool3x3s2Fn(Function):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1); the arg-max window slot is kept as uint8, the backward is a gather."""

    @staticmethod
    def forward(ctx, x):
        y, arg = ops.maxpool3x3s2_forward(x.contiguous())
        ctx.save_for_backward(arg)
        ctx.in_shape = tuple(x.shape)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        arg, = ctx.saved_tensors
        return ops.maxpool3x3s2_backward(dy.contiguous(), arg, ctx.in_shape)


def maxpool3x3s2(x):
    if x.dtype == torch.float16:
        return _h16_run(lambda t: ops.maxpool3x3s2_forward_h16(t.contiguous()), x)
    return MaxPool3x3s2Fn.apply(x)


class ReflectPad1Fn(Function):
    """cat([ReflectionPad2d(1)(upsample_nearest(x_i, s_i)) for i], 1): every source is written straight into its channel range of the one
    output (the padded copy has to be written anyway, so the concatenation costs nothing and the convolution behind it has one source)."""

    @staticmethod
    def forward(ctx, ups, pitch, *xs):
        xs = tuple(t.contiguous() for t in xs)
        ctx.ups = tuple(ups)
        ctx.shapes = tuple(tuple(t.shape) for t in xs)
        return ops.reflect_pad1_forward(xs, ctx.ups, pitch)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return (None, None) + tuple(ops.reflect_pad1_backward(dy.contiguous(), ctx.shapes, ctx.ups, ctx.needs_input_grad[2:]))


def reflect_pad1(xs, up=1, pitch=None):
    """xs: a tensor or a tuple of tensors (their channel concatenation); up: one factor (1 | 2) for all, or one per source; pitch: the
    output's width where it should exceed W + 2 (zero columns on the right)."""
    xs = tuple(xs) if isinstance(xs, (tuple, list)) else (xs,)
    ups = tuple(up) if isinstance(up, (tuple, list)) else (up,) * len(xs)
    _no_h16('reflect_pad1', *xs)
    if len(ups) != len(xs):
        raise ValueError("reflect_pad1: %d sources, %d factors" % (len(xs), len(ups)))
    return ReflectPad1Fn.apply(ups, pitch, *xs)


class ActCropFn(Function):
    """y = act(z[..., m:H-m, m:W-m]), act in {ACT_NONE, ACT_ELU, ACT_RELU, ACT_DISP}; backward from the saved output."""

    @staticmethod
    def forward(ctx, z, m, act, p0, p1, width=None):
        y = ops.act_crop_forward(z.contiguous(), m, act, p0, p1, width)
        ctx.save_for_backward(y)
        ctx.meta = (m, act, p0, p1, z.shape[-1])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        return ops.act_crop_backward(dy.contiguous(), y, *ctx.meta), None, None, None, None, None


def act_crop(z, m=0, act=ops.ACT_RELU, disp=(0.0, 1.0), width=None):
    """act(z) with m in {0, 1} border pixels dropped; ACT_DISP: disp[0] + disp[1] * sigmoid(z); width: the output's width where z has
    more than width + 2 m columns (a pitched map: the rest is dropped too)."""
    _no_h16('act_crop', z)
    return ActCropFn.apply(z, m, act, float(disp[0]), float(disp[1]), width)


class AffineFn(Function):
    @staticmethod
    def forward(ctx, x, s, t):
        ctx.s = s
        return ops.affine(x.contiguous(), s, t)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return ops.affine(dy.contiguous(), ctx.s, 0.0), None, None


def affine(x, s, t):
    _no_h16('affine', x)
    return AffineFn.apply(x, float(s), float(t))


def conv3x3_reflect(xs, weight, bias, cache, act=ops.ACT_ELU, up=1, disp=(0.0, 1.0)):
    """The decoder's Conv3x3 (ReflectionPad2d(1) + Conv2d(3)) and the activation behind it, on `xs` (a tensor, or a tuple standing for
    the channel concatenation), each source up-sampled by `up` first: reflect_pad1 -> the zero-pad "same" convolution on the
    (H + 2) x (W + 2) map, whose interior is exactly the valid convolution of the padded map -> act_crop(m = 1)."""
    if tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("conv3x3_reflect: 3x3 weights only, got %s" % (tuple(weight.shape),))
    first = xs[0] if isinstance(xs, (tuple, list)) else xs
    if first.dtype == torch.float16:        # fp16 forward: pad, up-sampling, concatenation, bias and activation in ONE launch
        return conv2d_h16_fused(xs, weight, cache, pad='reflect', up=up, bias=bias, act=act, disp=disp)
    s0 = up[0] if isinstance(up, (tuple, list)) else up
    W = s0 * first.shape[3]
    # a padded map wider than 320 columns whose width is no multiple of 32 does not fit the convolution kernels' tiles (KITTI's 642):
    # the pad kernel writes it at the next multiple of 32, zero columns on the right, which only reach outputs the crop drops
    pitch = -(-(W + 2) // 32) * 32 if (W + 2) > 320 and (W + 2) % 32 else None
    return act_crop(conv2d(reflect_pad1(xs, up, pitch), weight, bias, cache), 1, act, disp, width=W)


class LossCombineFn(Function):
    """loss = mean_i P[i] + weight * mean_i (S[i] / 2^i) from the per-scale device scalars, one launch each way (the reference does
    this with Python sums of 0-dim tensors: losses/multiview_photometric_loss.py:248-252, 275-280, 337-338; same operation order).
    Returns the 3-vector (loss, weighted smoothness, photometric); only [0] carries a gradient."""

    @staticmethod
    def forward(ctx, weight, n, *terms):
        ctx.meta = (float(weight), n, len(terms) - n)
        ctx.set_materialize_grads(False)
        out = ops.loss_combine_forward([t.detach().reshape(()) for t in terms[:n]], [t.detach().reshape(()) for t in terms[n:]],
                                       weight)
        smooth, photo = out[1], out[2]
        ctx.mark_non_differentiable(smooth, photo)
        return out[0], smooth, photo

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gs, _gp):
        weight, n, ns = ctx.meta
        if g is None:
            return (None,) * (2 + n + ns)
        d = ops.loss_combine_backward(g.contiguous(), n, ns, weight)
        return (None, None) + tuple(d[i] for i in range(n)) + tuple(d[8 + i] for i in range(ns))


def loss_combine(photometric, smoothness, weight):
    """(loss, weighted smoothness term, photometric term): 0-dim tensors, the last two without gradient (metrics)."""
    return LossCombineFn.apply(float(weight), len(photometric), *photometric, *smoothness)


class VelocityLossFn(Function):
    """Velocity supervision on J predicted [B,4,4] stacks (csrc/velocity.h; the reference's losses/velocity_loss.py:33-37 plus the
    weighted sum of models/VelSupModel.py:47-51, about 20 ATen launches each way): L = (1/J) sum_j mean_b | |t_pred| - |t_gt| |, one
    launch each way.  Returns (loss_in + weight * L, L) as 0-dim tensors; only the first carries a gradient."""

    @staticmethod
    def forward(ctx, weight, J, *tensors):
        pred, gt = list(tensors[:J]), list(tensors[J:2 * J])
        loss_in = tensors[2 * J] if len(tensors) > 2 * J else None
        ctx.meta = (float(weight), J, None if loss_in is None else tuple(loss_in.shape))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*pred, *gt)
        out = ops.velocity_loss_forward(pred, gt, weight, None if loss_in is None else loss_in.detach().reshape(1))
        total, L = out[1], out[0]
        ctx.mark_non_differentiable(L)
        return total, L

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gl):
        weight, J, in_shape = ctx.meta
        n_in = 2 * J + (in_shape is not None)
        if g is None:
            return (None,) * (2 + n_in)
        saved = ctx.saved_tensors
        d = ops.velocity_loss_backward(list(saved[:J]), list(saved[J:]), weight, g.reshape(1).contiguous())
        grads = tuple(d[j] if ctx.needs_input_grad[2 + j] else None for j in range(J)) + (None,) * J
        if in_shape is not None:
            grads += (g.reshape(in_shape),)
        return (None, None) + grads


def velocity_loss(pred_mats, gt_mats, weight=1.0, loss_in=None):
    """(loss_in + weight * L, L) for lists of J predicted and J ground-truth [B,4,4] transforms: 0-dim tensors, the second without
    gradient (the metric); without loss_in the first is weight * L.  Predictions and loss_in are float32; ground-truth poses may
    arrive as float64 (dataset poses) and are cast once.  The gradient reaches the predicted matrices and loss_in."""
    pred_mats, gt_mats = list(pred_mats), list(gt_mats)
    for j, t in enumerate(pred_mats):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError('velocity_loss: pred_mats[%d] must be a float32 tensor, got %s' % (j, getattr(t, 'dtype', type(t))))
    for j, t in enumerate(gt_mats):
        if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.float64):
            raise TypeError('velocity_loss: gt_mats[%d] must be a float32 or float64 tensor, got %s' % (j, getattr(t, 'dtype', type(t))))
    if loss_in is not None and (not torch.is_tensor(loss_in) or loss_in.dtype != torch.float32 or loss_in.numel() != 1):
        raise TypeError('velocity_loss: loss_in must be a float32 tensor of one element, got %s'
                        % (getattr(loss_in, 'dtype', type(loss_in)),))
    gt_mats = [t.detach().to(torch.float32).contiguous() for t in gt_mats]
    extra = () if loss_in is None else (loss_in,)
    return VelocityLossFn.apply(float(weight), len(pred_mats), *[t.contiguous() for t in pred_mats], *gt_mats, *extra)


class SupervisedLossFn(Function):
    """One scale of the supervised inverse-depth loss (l1 / mse / abs_rel / berhu / silog, optionally only where gt > 0)."""

    @staticmethod
    def forward(ctx, pred, gt, method, sparse):
        pred, gt = pred.contiguous(), gt.contiguous()
        loss, ws = ops.supervised_loss_forward(pred, gt, method, sparse)
        ctx.save_for_backward(pred, gt, ws)
        ctx.meta = (method, sparse)
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, gt, ws = ctx.saved_tensors
        method, sparse = ctx.meta
        g = g.reshape(1).to(torch.float32).contiguous()
        return ops.supervised_loss_backward(pred, gt, ws, g, method, sparse), None, None, None


def supervised_loss(pred, gt, method, sparse):
    return SupervisedLossFn.apply(pred, gt, method, sparse)


class ViewSynthesisFn(Function):
    """warped[j] = grid_sample(ref[j], project(reconstruct(1/inv_depth))) for the J context views of one scale.
    Differentiable w.r.t. inv_depth and the [J,B,4,4] pose matrices (the context image is data)."""

    @staticmethod
    def forward(ctx, inv_depth, ref, K, refK, T, padding_mode=0):
        inv_depth, ref, K, refK, T = (t.contiguous() for t in (inv_depth, ref, K, refK, T))
        warped = ops.view_synthesis_forward(inv_depth, ref, K, refK, T.detach(), padding_mode)
        ctx.save_for_backward(inv_depth, ref, K, refK, T)
        ctx.padding_mode = padding_mode
        return warped

    @staticmethod
    @once_differentiable
    def backward(ctx, d_warped):
        inv_depth, ref, K, refK, T = ctx.saved_tensors
        d_inv, dT = ops.view_synthesis_backward(d_warped.contiguous(), inv_depth, ref, K, refK, T.detach(), ctx.padding_mode)
        return d_inv, None, None, None, dT, None


def view_synthesis(inv_depth, ref, K, refK, T, padding_mode='zeros'):
    """padding_mode: 'zeros' | 'border' | 'reflection' (F.grid_sample semantics, align_corners=True)."""
    if padding_mode not in ops.PADDING_MODES:
        raise ValueError('Unknown padding_mode {}'.format(padding_mode))
    return ViewSynthesisFn.apply(inv_depth, ref, K, refK, T, ops.PADDING_MODES[padding_mode])


class NrsProjectFn(Function):
    """(unit directions [3,h,w], ray surface [3,h,w]) -> expected candidate coordinates [h,w,2] (row, col): the softmax over the
    41x41 patch of ray-surface dot products of GenericCamera.project, fused; differentiable w.r.t. both inputs."""

    @staticmethod
    def forward(ctx, direction, ray, temperature):
        direction, ray = direction.contiguous(), ray.contiguous()
        coords, stat = ops.nrs_project_forward(direction, ray, temperature)
        ctx.save_for_backward(direction, ray, coords, stat)
        ctx.temperature = temperature
        return coords

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        direction, ray, coords, stat = ctx.saved_tensors
        gdir, gray = ops.nrs_project_backward(direction, ray, coords, stat, g.contiguous(), ctx.temperature,
                                              want_dir=ctx.needs_input_grad[0], want_ray=ctx.needs_input_grad[1])
        return gdir, gray, None


def nrs_project(direction, ray, temperature):
    return NrsProjectFn.apply(direction, ray, temperature)


class SparseConvFn(Function):
    """out[n] = sum_i kern[i]^T . feats[nbr[n][i]] over the active sites (ME.MinkowskiConvolution, stride 1, no bias)."""

    @staticmethod
    def forward(ctx, feats, kern, nbr, count, ks):
        feats, kern = feats.contiguous(), kern.contiguous()
        ctx.save_for_backward(feats, kern, nbr, count)
        ctx.ks = ks
        return ops.sparse_conv(feats, kern.detach(), nbr, count, ks, flip=False)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        feats, kern, nbr, count = ctx.saved_tensors
        dout = dout.contiguous()
        dfeats = dkern = None
        if ctx.needs_input_grad[0]:
            dfeats = ops.sparse_conv(dout, kern.detach().transpose(1, 2).contiguous(), nbr, count, ctx.ks, flip=True)
        if ctx.needs_input_grad[1]:
            dkern = ops.sparse_conv_backward_weight(feats, dout, nbr, count, ctx.ks)
        return dfeats, dkern, None, None, None


def sparse_conv(feats, kern, nbr, count, ks):
    return SparseConvFn.apply(feats, kern, nbr, count, ks)


class SparseMaxPoolFn(Function):
    """ME.MinkowskiMaxPooling(3, 2) on feature rows: fine rows (imap_in of the [B, h, w] grid) -> coarse rows (sites_out / count_out)."""

    @staticmethod
    def forward(ctx, fin, imap_in, sites_out, count_out, cap_out, h, w):
        fin = fin.contiguous()
        fout, arg = ops.sparse_maxpool_forward(fin, imap_in, sites_out, count_out, cap_out, h, w)
        ctx.save_for_backward(arg)
        ctx.cap_in = fin.shape[0]
        return fout

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (arg,) = ctx.saved_tensors
        return ops.sparse_maxpool_backward(dout.contiguous(), arg, ctx.cap_in), None, None, None, None, None, None


def sparse_maxpool(fin, imap_in, sites_out, count_out, cap_out, h, w):
    return SparseMaxPoolFn.apply(fin, imap_in, sites_out, count_out, cap_out, h, w)


class SparseDensifyFn(Function):
    """feature rows -> dense [B, C, h, w], zeros at inactive cells (densify_features, reference minkowski.py:60-83)."""

    @staticmethod
    def forward(ctx, feats, imap, sites, count, B, h, w):
        ctx.save_for_backward(sites, count)
        ctx.cap = feats.shape[0]
        return ops.sparse_densify(feats.contiguous(), imap, B, h * w).view(B, feats.shape[1], h, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sites, count = ctx.saved_tensors
        B, C, h, w = g.shape
        return ops.sparse_gather(g.contiguous().view(B, C, h * w), sites, count, ctx.cap), None, None, None, None, None, None


def sparse_densify(feats, imap, sites, count, B, h, w):
    return SparseDensifyFn.apply(feats, imap, sites, count, B, h, w)


class SparseGatherFn(Function):
    """dense [B, C, h, w] -> feature rows at the active sites (the dense half of map_add_features, reference minkowski.py:116-136)."""

    @staticmethod
    def forward(ctx, dense, imap, sites, count, cap):
        B, C, h, w = dense.shape
        ctx.save_for_backward(imap)
        ctx.shape = (B, C, h, w)
        return ops.sparse_gather(dense.contiguous().view(B, C, h * w), sites, count, cap)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (imap,) = ctx.saved_tensors
        B, C, h, w = ctx.shape
        return ops.sparse_densify(g.contiguous(), imap, B, h * w).view(B, C, h, w), None, None, None, None


def sparse_gather(dense, imap, sites, count, cap):
    return SparseGatherFn.apply(dense, imap, sites, count, cap)


REDUCE_MIN, REDUCE_MEAN = 0, 1


class PhotometricFn(Function):
    """mean over pixels of min/mean over candidates of (w*SSIM-loss + (1-w)*L1); scalar float32.  Without clipping the scalar is
    finished on the device (pixel mean as float32) and backward hands the upstream gradient to the kernel as a device scalar: no
    ATen launch around the kernels (round 4; the `d * g` pass over the [J,B,3,H,W] gradient alone was 25 us per scale)."""

    @staticmethod
    def forward(ctx, warped, ref, target, ssim_w, C1, C2, automask, reduce_op, clip_loss=0.0):
        warped, ref, target = warped.contiguous(), ref.contiguous(), target.contiguous()
        J, B, _, H, W = warped.shape
        ctx.meta = (ssim_w, C1, C2, automask, reduce_op, B * H * W, clip_loss > 0.0)
        if clip_loss > 0.0:
            loss_sum, argmin = ops.photometric_forward(warped, ref, target, ssim_w, C1, C2, automask, reduce_op, clip_loss)
            ctx.save_for_backward(warped, target, argmin)
            return (loss_sum / float(B * H * W)).to(torch.float32).reshape(())
        loss, argmin = ops.photometric_forward(warped, ref, target, ssim_w, C1, C2, automask, reduce_op)
        ctx.save_for_backward(warped, target, argmin)
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        warped, target, argmin = ctx.saved_tensors
        ssim_w, C1, C2, automask, reduce_op, n, clip = ctx.meta
        up = g.reshape(1).to(torch.float32).contiguous()
        d = ops.photometric_backward(warped, target, argmin, 1.0 / n, up, ssim_w, C1, C2, automask, reduce_op, clip)
        return d, None, None, None, None, None, None, None, None


class PhotometricL1Fn(Function):
    """L1-only photometric loss (ssim_loss_weight == 0) with the 'min' reduce op and / or clipping: the reference reduces and clips
    per-CHANNEL candidate maps then (multiview_photometric_loss.py:205-219, 238-246); csrc/loss.hip: l1cand_*_kernel."""

    @staticmethod
    def forward(ctx, warped, ref, target, automask, reduce_op, clip_loss):
        warped, ref, target = warped.contiguous(), ref.contiguous(), target.contiguous()
        J, B, _, H, W = warped.shape
        loss, rec = ops.photometric_l1_forward(warped, ref, target, automask, reduce_op, clip_loss)
        ctx.save_for_backward(warped, target, rec)
        ctx.meta = (automask, reduce_op, B * H * W)
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        warped, target, rec = ctx.saved_tensors
        automask, reduce_op, n = ctx.meta
        up = g.reshape(1).to(torch.float32).contiguous()
        return ops.photometric_l1_backward(warped, target, rec, 1.0 / n, up, automask, reduce_op), None, None, None, None, None


def warp_photometric(inv_depth, ref, target, K, refK, T, ssim_w, C1, C2, automask, reduce_op, clip_loss=0.0, padding_mode='zeros'):
    """view_synthesis + photometric terms of one scale.  (Round 5's single-kernel form -- the warp inside the photometric tile loaders --
    measured -0.3 % twice, profiles/r05_ab_loss_fuse.txt, and was removed in round 6.)"""
    if padding_mode not in ops.PADDING_MODES:
        raise ValueError('Unknown padding_mode {}'.format(padding_mode))
    warped = view_synthesis(inv_depth, ref, K, refK, T, padding_mode)
    return photometric(warped, ref, target, ssim_w, C1, C2, automask, reduce_op, clip_loss)


def photometric(warped, ref, target, ssim_w, C1, C2, automask, reduce_op, clip_loss=0.0):
    if ssim_w == 0.0 and (reduce_op == REDUCE_MIN or clip_loss > 0.0):
        return PhotometricL1Fn.apply(warped, ref, target, automask, reduce_op, clip_loss)
    return PhotometricFn.apply(warped, ref, target, ssim_w, C1, C2, automask, reduce_op, clip_loss)


class SmoothnessFn(Function):
    """mean|Sx| + mean|Sy| of the edge-aware first differences of a (mean-normalised) inverse depth map."""

    @staticmethod
    def forward(ctx, inv_norm, image):
        inv_norm, image = inv_norm.contiguous(), image.contiguous()
        B, _, H, W = image.shape
        sums = ops.smoothness_forward(inv_norm, image)
        ctx.save_for_backward(inv_norm, image)
        nx, ny = float(B * H * (W - 1)), float(B * (H - 1) * W)
        ctx.meta = (nx, ny)
        return (sums[0] / nx + sums[1] / ny).to(torch.float32).reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        inv_norm, image = ctx.saved_tensors
        nx, ny = ctx.meta
        return ops.smoothness_backward(inv_norm, image, 1.0 / nx, 1.0 / ny) * g, None


def smoothness(inv_norm, image):
    return SmoothnessFn.apply(inv_norm, image)


class SmoothnessNormFn(Function):
    """mean|Sx| + mean|Sy| of the edge-aware first differences of inv_depth / clamp(mean_hw(inv_depth), 1e-6): the reference's
    calc_smoothness_loss (multiview_photometric_loss.py:255-285) for ONE scale, the mean normalisation fused into the kernels
    (3 launches forward, 2 backward; the ATen form around SmoothnessFn is ~10 + ~12)."""

    @staticmethod
    def forward(ctx, inv_depth, image):
        inv_depth, image = inv_depth.contiguous(), image.contiguous()
        loss, mean = ops.smoothness_norm_forward(inv_depth, image)
        ctx.save_for_backward(inv_depth, image, mean)
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        inv_depth, image, mean = ctx.saved_tensors
        up = g.reshape(1).to(torch.float32).contiguous()
        return ops.smoothness_norm_backward(inv_depth, image, mean, up), None


def smoothness_norm(inv_depth, image):
    return SmoothnessNormFn.apply(inv_depth, image)


# The scales of the multi-view loss in one launch per kernel (PNSFM_LOSS_MS=0 / set_loss_ms(False): one set of launches per scale, the
# former path, the A/B switch and the reference of tests/loss_ms_cases.py).
_LOSS_MS = os.environ.get('PNSFM_LOSS_MS', '1') != '0'
_LOSS_MS_USED = [False]


def set_loss_ms(on):
    """Switch the all-scales loss node on or off; returns the previous setting."""
    global _LOSS_MS
    prev, _LOSS_MS = _LOSS_MS, bool(on)
    return prev


def loss_ms_used():
    """Whether the last multiview_loss_terms call ran the all-scales node (False: the per-scale path)."""
    return _LOSS_MS_USED[0]


class MultiviewLossTermsFn(Function):
    """The photometric and smoothness terms of n scales that share the context images, the target, the intrinsics and the poses (every
    inverse-depth map at the image's resolution): view synthesis, photometric terms and smoothness of ALL scales, one launch per kernel,
    the unwarped automask candidates evaluated once.  Outputs: the n photometric scalars, then (with_smooth) the n smoothness scalars,
    0-dim views of two [n] tensors.  Backward returns every scale's complete d_inv_depth (photometric + smoothness term, summed in
    the smoothness kernel) and the pose gradient summed over the scales inside the finish kernel.  Bit for bit the per-scale nodes'
    results (csrc/loss.hip: the same kernels, a table of one scale)."""

    @staticmethod
    def forward(ctx, ref, target, K, refK, T, ssim_w, C1, C2, automask, reduce_op, padding_mode, with_smooth, *inv_depths):
        ref, target, K, refK, T = (t.contiguous() for t in (ref, target, K, refK, T))
        invs = [d.contiguous() for d in inv_depths]
        n = len(invs)
        J, B, _, H, W = ref.shape
        warped = ops.view_synthesis_forward_ms(invs, ref, K, refK, T.detach(), padding_mode)
        idmap = ops.photometric_identity_forward(ref, target, ssim_w, C1, C2) if automask else None
        photo, argmin = ops.photometric_forward_ms(warped, idmap, target, ssim_w, C1, C2, automask, reduce_op)
        outs = [photo[i] for i in range(n)]
        mean = None
        if with_smooth:
            smooth, mean = ops.smoothness_norm_forward_ms(invs, [target] * n)
            outs += [smooth[i] for i in range(n)]
        ctx.save_for_backward(ref, target, K, refK, T, warped, argmin, mean, *invs)
        ctx.meta = (ssim_w, C1, C2, automask, reduce_op, padding_mode, with_smooth, n, B * H * W)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        ref, target, K, refK, T, warped, argmin, mean = ctx.saved_tensors[:8]
        invs = list(ctx.saved_tensors[8:])
        ssim_w, C1, C2, automask, reduce_op, padding_mode, with_smooth, n, npix = ctx.meta

        def upstream(gs):      # a term nothing was computed from has no gradient: a zero scalar keeps the one launch
            return [(g if g is not None else torch.zeros((), device=ref.device)).reshape(1).to(torch.float32).contiguous() for g in gs]

        d_warped = ops.photometric_backward_ms(warped, target, argmin, 1.0 / npix, upstream(grads[:n]), ssim_w, C1, C2, automask,
                                               reduce_op)
        d_inv, dT = ops.view_synthesis_backward_ms(d_warped, invs, ref, K, refK, T.detach(), padding_mode)
        d_invs = [d_inv[i] for i in range(n)]
        if with_smooth:
            ops.smoothness_norm_backward_ms(invs, [target] * n, mean, upstream(grads[n:2 * n]), d_invs)
        return (None, None, None, None, dT) + (None,) * 7 + tuple(d_invs)


def multiview_loss_terms(inv_depths, refs, image, K, refK, T, ssim_w, C1, C2, automask, reduce_op, clip_loss=0.0,
                         padding_mode='zeros', with_smooth=True):
    """(photometric, smoothness): two lists of n 0-dim tensors (smoothness empty without with_smooth) for loss_combine, or None
    where the all-scales node does not apply -- the switch is off, a scale is not at the image's resolution, clipping is on, or the
    configuration takes the L1-only kernels -- and the caller runs the per-scale path.  loss_ms_used() reports which."""
    if padding_mode not in ops.PADDING_MODES:
        raise ValueError('Unknown padding_mode {}'.format(padding_mode))
    n = len(inv_depths)
    ok = (_LOSS_MS and 1 <= n <= ops.LOSS_MAX_SCALES and clip_loss <= 0.0 and not (ssim_w == 0.0 and reduce_op == REDUCE_MIN)
          and all(tuple(d.shape[-2:]) == tuple(image.shape[-2:]) for d in inv_depths))
    _LOSS_MS_USED[0] = bool(ok)
    if not ok:
        return None
    outs = MultiviewLossTermsFn.apply(refs, image, K, refK, T, ssim_w, C1, C2, bool(automask), reduce_op,
                                      ops.PADDING_MODES[padding_mode], bool(with_smooth), *inv_depths)
    return list(outs[:n]), list(outs[n:])


# ---- depth evaluation (include/pnsfm.h "depth evaluation"; csrc/depth_eval.h) ------------------------------------------------------
# Forward only, like the fp16 forward: evaluation runs under torch.no_grad(); with a gradient-requiring input the result carries a
# node whose backward raises, for fp32 and fp16 alike.
_EVAL_ONLY_FWD = "the depth-evaluation kernels are forward only (post-processing and metrics run under torch.no_grad())"


class _EvalForwardOnlyFn(Function):
    @staticmethod
    def forward(ctx, fn, *args):
        return fn(*args)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(_EVAL_ONLY_FWD)


def post_process_inv_depth(inv, inv_flipped, method='mean'):
    """Flip-and-fuse post-processing of an inverse-depth map and the map predicted from the mirrored image (the reference's
    utils/depth.py:229-255) in ONE launch; [B,1,H,W] fp32 or fp16 -> inv's dtype (fp32 arithmetic, one rounding)."""
    if method not in ops.PP_METHODS:
        raise ValueError('Unknown post-process method {}'.format(method))
    run = lambda a, b: ops.post_process_inv_depth(a.contiguous(), b.contiguous(), ops.PP_METHODS[method])      # noqa: E731
    if torch.is_grad_enabled() and (inv.requires_grad or inv_flipped.requires_grad):
        return _EvalForwardOnlyFn.apply(run, inv, inv_flipped)
    return run(inv, inv_flipped)


def depth_metrics(gt, pred, min_depth, max_depth, window=None, scale_output='resize', use_gt_scale=True, pred_is_inverse=False,
                  details=False):
    """[abs_rel, sqr_rel, rmse, rmse_log, a1, a2, a3] of packnet_sfm.utils.depth.compute_depth_metrics as a [7] fp32 DEVICE tensor, in a
    fixed number of launches and without a host sync.  gt [B,1,Hg,Wg], pred [B,1,Hp,Wp], fp32 or fp16 each (arithmetic is fp32: for
    fp16 storage the result is the Python function's on .float() inputs).  window = (y1, y2, x1, x2): the rows / columns of gt that
    count (None: all; the Garg crop: utils.depth.crop_window).  pred_is_inverse: pred is INVERSE depth, inverted per tap before the
    resize (inv2depth without its pass).
    details=True -> (metrics, rows [B,8] = per-image metrics + valid-pixel count, medians [B,2] = (gt, sampled prediction) of each
    image or None without use_gt_scale, sampled [B,1,Hg,Wg] = the prediction the kernels saw at every ground-truth pixel)."""
    if scale_output not in ops.SCALE_OUTPUTS:
        raise NotImplementedError('Depth scale function {} not implemented.'.format(scale_output))
    if torch.is_grad_enabled() and (gt.requires_grad or pred.requires_grad):
        raise NotImplementedError(_EVAL_ONLY_FWD)
    if window is None:
        window = (0, gt.shape[2], 0, gt.shape[3])
    metrics, rows, ws, sampled = ops.depth_metrics(gt.contiguous(), pred.contiguous(), min_depth, max_depth, window,
                                                   ops.SCALE_OUTPUTS[scale_output], use_gt_scale, pred_is_inverse, dump=details)
    if not details:
        return metrics
    B = gt.shape[0]
    return metrics, rows, (ws[:2 * B].view(torch.float32).reshape(B, 2) if use_gt_scale else None), sampled


# ---- depth output (include/pnsfm.h "depth output"; csrc/depth_output.h) -------------------------------------------------------------
def viz_inv_depth_u8(inv, lut8, rgb=None, normalizer=None, percentile=95, filter_zeros=False, bgr=False, details=False):
    """The reference's viz_inv_depth (utils/depth.py:66-100) for a batch, as bytes, in a fixed number of launches and without a host
    sync.  inv [B,1,H,W] and rgb [B,3,H,W] | None: fp32 or fp16 (arithmetic is fp32: an fp16 map gives the result of its .float()
    copy); lut8: uint8 [N,3] on inv's device, the colour table as bytes (rint(table * 255)), 1 <= N <= 256.  normalizer: None -- the
    `percentile` of each image's values (of its values > 0 with filter_zeros), exactly np.percentile's float32 result -- or a float.
    -> uint8 [B,H,W,3] = lut8[index], or with rgb [B,2H,W,3] with the frame on top (what scripts/infer.py concatenates); bgr swaps
    the channel order of both halves.
    details=True -> (out, index uint8 [B,H,W] = the table index of every pixel, normalisers fp32 [B])."""
    if torch.is_grad_enabled() and (inv.requires_grad or (rgb is not None and rgb.requires_grad)):
        raise NotImplementedError("the depth-output kernels are forward only (inference and logging run under torch.no_grad())")
    out, index, ws = ops.viz_inv_depth(inv.contiguous(), rgb.contiguous() if rgb is not None else None, lut8.contiguous(), percentile,
                                       filter_zeros, None if normalizer is None else float(normalizer), bgr, want_index=details)
    if not details:
        return out
    return out, index, ws[:inv.shape[0]].view(torch.float32)


def depth_png16(inv):
    """The values write_depth's .png branch stores for inv2depth(inv) (utils/depth.py:35-63): uint16, inv's shape,
    min(trunc((1 / max(inv, 1e-6)) * 256), 65535); fp32 or fp16 storage, fp32 arithmetic, one launch."""
    if torch.is_grad_enabled() and inv.requires_grad:
        raise NotImplementedError("the depth-output kernels are forward only (inference and logging run under torch.no_grad())")
    return ops.depth_png16(inv.contiguous())
