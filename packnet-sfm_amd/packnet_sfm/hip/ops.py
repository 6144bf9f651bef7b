"""Tensor-level wrappers over the C ABI of libpnsfm_hip.so (no autograd here; see functional.py).

Every wrapper validates dtype / contiguity / device, allocates outputs with torch (PyTorch is the device
allocator and stream owner -- plumbing, not compute) and enqueues the HIP kernels on torch's current stream.
"""
import ctypes
import os
import threading

import torch

from . import _lib


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream       # (device index) -> hipStream_t as int: no Stream object per launch
except AttributeError:                                      # pragma: no cover
    _raw_stream = None


# a raw hipStream_t (int) and the device index it belongs to: every launch of THIS THREAD on THAT device goes there instead of torch's
# current stream (stream_override).  Per thread (a process-global override also redirected launches of another thread --
# a second device's autograd worker, a prefetch thread -- onto the wrong stream, even a stream of another device).
_TLS = threading.local()


class stream_override:
    """`with stream_override(raw_handle):` -- the ops inside enqueue on that HIP stream WITHOUT switching torch's current stream
    (torch.cuda.stream costs ~20 us per enter / exit).  Only for code that calls nothing but these ops: a torch operation inside would
    still go to torch's current stream.  Allocations stay in the current stream's pool: the caller orders their reuse (functional.py)."""

    def __init__(self, raw, device_index=None):
        self.ov = (raw, device_index)

    def __enter__(self):
        self.prev = getattr(_TLS, 'ov', None)
        _TLS.ov = self.ov
        return self

    def __exit__(self, *exc):
        _TLS.ov = self.prev
        return False


def current_raw_stream(device):
    """torch's current stream of `device` as an int handle."""
    if _raw_stream is not None:
        return int(_raw_stream(device.index))
    return int(torch.cuda.current_stream(device).cuda_stream)


def launch_stream_raw(device):
    """The raw stream (int) a launch for `device` goes to right now: this thread's override, else torch's current stream; 0 for the
    host-emulated build's CPU tensors."""
    if device.type != 'cuda':
        return 0
    ov = getattr(_TLS, 'ov', None)
    if ov is not None and (ov[1] is None or ov[1] == device.index):
        return ov[0]
    if _raw_stream is not None:
        return int(_raw_stream(device.index))
    return int(torch.cuda.current_stream(device).cuda_stream)


def stream_wait_stream(waiter_raw, signaler_raw):
    _lib.check(_lib.get().pnsfm_stream_wait_stream(ctypes.c_void_p(waiter_raw), ctypes.c_void_p(signaler_raw)), "stream_wait_stream")


def _stream(t):
    """torch's CURRENT stream of t's device as a hipStream_t.  ~800 launches per training step go through here: the raw-handle
    query costs ~0.3 us against ~5 us for torch.cuda.current_stream(...).cuda_stream (round 5 host profile)."""
    if not t.is_cuda:
        return ctypes.c_void_p(0)
    ov = getattr(_TLS, 'ov', None)
    if ov is not None and (ov[1] is None or ov[1] == t.device.index):
        return ctypes.c_void_p(ov[0])
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(t.device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _chk(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if _lib.REQUIRE_CUDA and not t.is_cuda:
            raise RuntimeError("packnet_sfm HIP op got a %s tensor: the HIP kernels run on MI355X only, "
                               "there is no CPU fallback" % t.device)
        if not t.is_contiguous():
            raise RuntimeError("packnet_sfm HIP op needs contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("packnet_sfm HIP op got tensors on different devices")


def _f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("packnet_sfm HIP op needs float32 tensors, got %s" % t.dtype)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# ---------------------------------------------------------------------------------------------- conv2d
def tune_shipped_entries():
    return int(_lib.get().pnsfm_tune_shipped_entries())


def conv2d_packed_sizes(Cin, Cout, ks):
    lib = _lib.get()
    return (int(lib.pnsfm_conv2d_packed_elems_fwd(Cin, Cout, ks)), int(lib.pnsfm_conv2d_packed_elems_bwd(Cin, Cout, ks)))


WGRAD_EPI_ADD, WGRAD_EPI_TAPT = 1, 2      # PNSFM_WGRAD_EPI_* of include/pnsfm.h


def conv2d_pack_tapT_supported(Cin, Cout, ks):
    """Do the packers read this layer's transposed taps in place (conv2d_pack(tapT=True), a (w, pf, pb, True) table entry)?"""
    return bool(_lib.get().pnsfm_conv2d_pack_tapt_supported(Cin, Cout, ks))


def conv2d_pack(w, wp_fwd=None, wp_bwd=None, want_fwd=True, want_bwd=True, tapT=False):
    """w: [Cout, Cin, k, k] (reference layout) -> packed forward / backward-data weights.  tapT: the images of w.transpose(2, 3),
    read in place."""
    _chk(w, wp_fwd, wp_bwd); _f32(w)
    Cout, Cin, ks, ks2 = w.shape
    assert ks == ks2
    nf, nb = conv2d_packed_sizes(Cin, Cout, ks)
    if want_fwd and wp_fwd is None:
        wp_fwd = torch.empty(nf, dtype=torch.float32, device=w.device)
    if want_bwd and wp_bwd is None:
        wp_bwd = torch.empty(nb, dtype=torch.float32, device=w.device)
    if tapT:
        rc = _lib.get().pnsfm_conv2d_pack_weights_t(_ptr(w), _ptr(wp_fwd if want_fwd else None),
                                                    _ptr(wp_bwd if want_bwd else None), Cin, Cout, ks, 1, _stream(w))
    else:
        rc = _lib.get().pnsfm_conv2d_pack_weights(_ptr(w), _ptr(wp_fwd if want_fwd else None),
                                                  _ptr(wp_bwd if want_bwd else None), Cin, Cout, ks, _stream(w))
    _lib.check(rc, "conv2d_pack_weights")
    return wp_fwd, wp_bwd


def conv2d_pack_table_build(entries, device):
    """entries: [(w, wp_fwd, wp_bwd)] (or (w, wp_fwd, wp_bwd, tapT): the images of w.transpose(2, 3), read in place) with w
    [Cout, Cin, k, k] and packed buffers of conv2d_packed_sizes().  Returns
    (table tensor on `device`, number of items, total blocks, indices of the entries the table covers) -- entries whose shape
    does not take the split-bf16 layout in both directions are left out (pack them with conv2d_pack)."""
    import ctypes
    lib = _lib.get()
    isz = int(lib.pnsfm_conv2d_pack_item_bytes())
    host = (ctypes.c_ubyte * (isz * max(1, len(entries))))()
    n, blocks, covered = 0, 0, []
    for i, ent in enumerate(entries):
        w, pf, pb = ent[:3]
        _chk(w, pf, pb); _f32(w, pf, pb)
        Cout, Cin, ks, _ = w.shape
        if len(ent) > 3 and ent[3]:
            rc = lib.pnsfm_conv2d_pack_item_fill_t(ctypes.addressof(host) + n * isz, _ptr(w), _ptr(pf), _ptr(pb), Cin, Cout, ks, blocks, 1)
        else:
            rc = lib.pnsfm_conv2d_pack_item_fill(ctypes.addressof(host) + n * isz, _ptr(w), _ptr(pf), _ptr(pb), Cin, Cout, ks, blocks)
        if rc < 0:
            _lib.check(rc, "conv2d_pack_item_fill")
        if rc > 0:
            n += 1
            blocks += rc
            covered.append(i)
    table = torch.frombuffer(bytearray(bytes(host)[:max(1, n) * isz]), dtype=torch.uint8).to(device)
    return table, n, blocks, covered


def conv2d_pack_table_run(table, n, blocks):
    if n:
        _lib.check(_lib.get().pnsfm_conv2d_pack_table(_ptr(table), n, blocks, _stream(table)), "conv2d_pack_table")


def conv2d_forward(x, wp_fwd, bias, Cout, ks):
    _chk(x, wp_fwd, bias); _f32(x, wp_fwd, bias)
    B, Cin, H, W = x.shape
    y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    rc = _lib.get().pnsfm_conv2d_forward(_ptr(x), _ptr(wp_fwd), _ptr(bias), _ptr(y), B, Cin, Cout, H, W, ks, _stream(x))
    _lib.check(rc, "conv2d_forward")
    return y


def conv2d_backward_data(dy, wp_bwd, Cin, ks, addend=None):
    """dx [B,Cin,H,W]; addend (optional): the tensor's other gradient, added in the launch's epilogue -- [B,Cin,H,W], dense or a
    channel slice of a wider dense tensor (any sample stride)."""
    _chk(dy, wp_bwd); _f32(dy, wp_bwd)
    B, Cout, H, W = dy.shape
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=dy.device)
    if addend is None:
        rc = _lib.get().pnsfm_conv2d_backward_data(_ptr(dy), _ptr(wp_bwd), _ptr(dx), B, Cin, Cout, H, W, ks, _stream(dy))
        _lib.check(rc, "conv2d_backward_data")
        return dx
    _f32(addend)
    if addend.device != dy.device:
        raise RuntimeError("conv2d_backward_data: addend lives on %s, dy on %s" % (addend.device, dy.device))
    if tuple(addend.shape) != (B, Cin, H, W):
        raise RuntimeError("conv2d_backward_data: addend %s does not match dx %s" % (tuple(addend.shape), (B, Cin, H, W)))
    st = addend.stride()
    if not (st[3] == 1 and st[2] == W and st[1] == H * W and (B == 1 or st[0] >= Cin * H * W)):
        addend = addend.contiguous()
        st = addend.stride()
    rc = _lib.get().pnsfm_conv2d_backward_data_add(_ptr(dy), _ptr(wp_bwd), _ptr(dx), _ptr(addend), int(st[0]) if B > 1 else Cin * H * W, B,
                                                   Cin, Cout, H, W, ks, _stream(dy))
    _lib.check(rc, "conv2d_backward_data_add")
    return dx


def _alloc_dw_db(Cout, Cin, ks, want_bias, device):
    """dw and dbias in one allocation (dbias right behind dw): a split-K weight gradient zero-fills both with one memset."""
    n = Cout * Cin * ks * ks
    buf = torch.empty((n + (Cout if want_bias else 0),), dtype=torch.float32, device=device)
    return buf[:n].view(Cout, Cin, ks, ks), (buf[n:] if want_bias else None)


def conv2d_backward_weight(x, dy, ks, want_bias=True, dw_out=None, db_out=None):
    """dw_out / db_out: write the gradients into these (contiguous, right-shaped) tensors instead of fresh ones -- the flat
    gradient arena of rccl/flat_adam.py hands out views of its all-reduce buckets here, so the weight gradient lands
    where the collective and the optimizer read it, with no gather copy."""
    _chk(x, dy); _f32(x, dy)
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    if dw_out is not None:
        _chk(dw_out, db_out); _f32(dw_out, db_out)
        if tuple(dw_out.shape) != (Cout, Cin, ks, ks) or (want_bias and (db_out is None or db_out.numel() != Cout)):
            raise RuntimeError("conv2d_backward_weight: gradient slot has the wrong shape")
        # fresh view objects: AccumulateGrad adopts a gradient only if nobody else holds the tensor object
        dw, db = dw_out.view(dw_out.shape), (db_out.view(db_out.shape) if want_bias else None)
    else:
        dw, db = _alloc_dw_db(Cout, Cin, ks, want_bias, x.device)
    rc = _lib.get().pnsfm_conv2d_backward_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), B, Cin, Cout, H, W, ks, _stream(x))
    _lib.check(rc, "conv2d_backward_weight")
    return dw, db


def conv2d_forward_cat(xs, wp_fwd, bias, Cout, ks):
    """conv(cat(xs, 1)) without the concatenated tensor; xs: 2 or 3 contiguous NCHW tensors of equal B, H, W.  Raises HipError when
    the shape is outside the split kernels' envelope (the caller concatenates instead)."""
    _chk(*xs, wp_fwd, bias); _f32(*xs, wp_fwd, bias)
    B, _, H, W = xs[0].shape
    C = [t.shape[1] for t in xs] + [0] * (3 - len(xs))
    y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=xs[0].device)
    rc = _lib.get().pnsfm_conv2d_forward_cat(_ptr(xs[0]), C[0], _ptr(xs[1]), C[1], _ptr(xs[2] if len(xs) > 2 else None), C[2],
                                             _ptr(wp_fwd), _ptr(bias), _ptr(y), B, Cout, H, W, ks, _stream(xs[0]))
    _lib.check(rc, "conv2d_forward_cat")
    return y


def conv2d_cat_wgrad_supported(channels, Cout, H, W, ks, B=1):
    """Will conv2d_backward_weight_cat take sources with these channel counts (list of 2 or 3)?  Pure query."""
    C = list(channels) + [0] * (3 - len(channels))
    return bool(_lib.get().pnsfm_conv2d_cat_wgrad_supported(C[0], C[1], C[2], Cout, B, H, W, ks))


def conv2d_backward_weight_cat(xs, dy, ks, want_bias=True, dw_out=None, db_out=None):
    _chk(*xs, dy); _f32(*xs, dy)
    B, _, H, W = xs[0].shape
    C = [t.shape[1] for t in xs] + [0] * (3 - len(xs))
    Cin, Cout = sum(C), dy.shape[1]
    if dw_out is not None:
        _chk(dw_out, db_out); _f32(dw_out, db_out)
        if tuple(dw_out.shape) != (Cout, Cin, ks, ks) or (want_bias and (db_out is None or db_out.numel() != Cout)):
            raise RuntimeError("conv2d_backward_weight_cat: gradient slot has the wrong shape")
        dw, db = dw_out.view(dw_out.shape), (db_out.view(db_out.shape) if want_bias else None)
    else:
        dw, db = _alloc_dw_db(Cout, Cin, ks, want_bias, dy.device)
    rc = _lib.get().pnsfm_conv2d_backward_weight_cat(_ptr(xs[0]), C[0], _ptr(xs[1]), C[1], _ptr(xs[2] if len(xs) > 2 else None), C[2],
                                                     _ptr(dy), _ptr(dw), _ptr(db), B, Cout, H, W, ks, _stream(dy))
    _lib.check(rc, "conv2d_backward_weight_cat")
    return dw, db


def conv2d_forward_strided(x, wp_fwd, bias, Cout, ks, stride):
    _chk(x, wp_fwd, bias); _f32(x, wp_fwd, bias)
    B, Cin, H, W = x.shape
    P = ks // 2
    Ho, Wo = (H + 2 * P - ks) // stride + 1, (W + 2 * P - ks) // stride + 1
    y = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    rc = _lib.get().pnsfm_conv2d_forward_strided(_ptr(x), _ptr(wp_fwd), _ptr(bias), _ptr(y), B, Cin, Cout, H, W, ks, stride,
                                                 _stream(x))
    _lib.check(rc, "conv2d_forward_strided")
    return y


def conv2d_backward_weight_strided(x, dy, ks, stride, want_bias=True, dw_out=None, db_out=None):
    _chk(x, dy); _f32(x, dy)
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    if dw_out is not None:      # gradient slots, as conv2d_backward_weight
        _chk(dw_out, db_out); _f32(dw_out, db_out)
        if tuple(dw_out.shape) != (Cout, Cin, ks, ks) or (want_bias and (db_out is None or db_out.numel() != Cout)):
            raise RuntimeError("conv2d_backward_weight_strided: gradient slot has the wrong shape")
        dw, db = dw_out.view(dw_out.shape), (db_out.view(db_out.shape) if want_bias else None)
    else:
        dw, db = _alloc_dw_db(Cout, Cin, ks, want_bias, x.device)
    rc = _lib.get().pnsfm_conv2d_backward_weight_strided(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), B, Cin, Cout, H, W, ks, stride,
                                                         _stream(x))
    _lib.check(rc, "conv2d_backward_weight_strided")
    return dw, db


# Row windows (include/pnsfm.h "Row windows"): x [2B, Cin, 2r, W] holds the batched border strips of the collapsed packing block --
# the leading half the strips whose frame rows are the FIRST r, the trailing half those whose frame rows are the LAST r; only the
# frame rows are computed: y / dy are [2B, Cout, r, W].
def _rows_shape(t, r, rows, what):
    B2, C, H, W = t.shape
    if r < 1 or H != rows or B2 % 2:
        raise RuntimeError("%s: expected [2B, C, %d, W] for r = %d, got %s" % (what, rows, r, tuple(t.shape)))
    return B2, C, W


def conv2d_forward_rows(x, wp_fwd, bias, Cout, ks, r):
    _chk(x, wp_fwd, bias); _f32(x, wp_fwd, bias)
    B2, Cin, W = _rows_shape(x, r, 2 * r, "conv2d_forward_rows")
    y = torch.empty((B2, Cout, r, W), dtype=torch.float32, device=x.device)
    rc = _lib.get().pnsfm_conv2d_forward_rows(_ptr(x), _ptr(wp_fwd), _ptr(bias), _ptr(y), B2, Cin, Cout, r, 2 * r, W, ks, r, B2 // 2,
                                              _stream(x))
    _lib.check(rc, "conv2d_forward_rows")
    return y


def conv2d_backward_data_rows(dy, wp_bwd, Cin, ks, r):
    """dx [2B, Cin, 2r, W] of conv2d_forward_rows from dy [2B, Cout, r, W]."""
    _chk(dy, wp_bwd); _f32(dy, wp_bwd)
    B2, Cout, W = _rows_shape(dy, r, r, "conv2d_backward_data_rows")
    dx = torch.empty((B2, Cin, 2 * r, W), dtype=torch.float32, device=dy.device)
    rc = _lib.get().pnsfm_conv2d_backward_data_rows(_ptr(dy), _ptr(wp_bwd), _ptr(dx), B2, Cin, Cout, 2 * r, r, W, ks, -r, B2 // 2,
                                                    _stream(dy))
    _lib.check(rc, "conv2d_backward_data_rows")
    return dx


def conv2d_backward_weight_rows(x, dy, ks, r, want_bias=True, dw_out=None, db_out=None, epi=0):
    """Weight (and bias) gradient of conv2d_forward_rows; dw_out / db_out: gradient slots, as conv2d_backward_weight.
    epi (WGRAD_EPI_*): ADD -- the gradient is added to what dw_out / db_out hold (needs them); TAPT -- dw with its taps swapped back."""
    if (epi & WGRAD_EPI_ADD) and dw_out is None:
        raise RuntimeError("conv2d_backward_weight_rows: adding into a gradient needs the destination")
    _chk(x, dy); _f32(x, dy)
    B2, Cin, W = _rows_shape(x, r, 2 * r, "conv2d_backward_weight_rows")
    if _rows_shape(dy, r, r, "conv2d_backward_weight_rows")[::2] != (B2, W):
        raise RuntimeError("conv2d_backward_weight_rows: dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    Cout = dy.shape[1]
    if dw_out is not None:
        _chk(dw_out, db_out); _f32(dw_out, db_out)
        if tuple(dw_out.shape) != (Cout, Cin, ks, ks) or (want_bias and (db_out is None or db_out.numel() != Cout)):
            raise RuntimeError("conv2d_backward_weight_rows: gradient slot has the wrong shape")
        dw, db = dw_out.view(dw_out.shape), (db_out.view(db_out.shape) if want_bias else None)
    else:
        dw, db = _alloc_dw_db(Cout, Cin, ks, want_bias, x.device)
    if epi:
        rc = _lib.get().pnsfm_conv2d_backward_weight_epi(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), B2, Cin, Cout, r, 2 * r, W, ks, r, B2 // 2,
                                                         int(epi), _stream(x))
    else:
        rc = _lib.get().pnsfm_conv2d_backward_weight_rows(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), B2, Cin, Cout, r, 2 * r, W, ks, r, B2 // 2,
                                                          _stream(x))
    _lib.check(rc, "conv2d_backward_weight_rows")
    return dw, db


# ------------------------------------------------------------------------------------------- groupnorm
ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2
GN_MAX_SPLIT = 64     # PNSFM_GN_MAX_SPLIT in include/pnsfm.h


_GN_WS = {}


def _gn_ws_doubles(B, C, G):
    k = (B, C, G)
    v = _GN_WS.get(k)
    if v is None:
        v = _GN_WS[k] = int(_lib.get().pnsfm_groupnorm_ws_doubles(B, C, G))
    return v


def groupnorm_act_forward(x, res, gamma, beta, G, eps, act):
    _chk(x, res, gamma, beta); _f32(x, res, gamma, beta)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    ms = torch.empty((2, B * G), dtype=torch.float32, device=x.device)       # mean | rstd in one allocation
    mean, rstd = ms[0], ms[1]
    # (no workspace tensor: the two-launch form keeps its partial sums in the stream's scratch buffer, the one-launch form has none)
    rc = _lib.get().pnsfm_groupnorm_act_forward(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd),
                                                None, B, C, HW, G, float(eps), act, _stream(x))
    _lib.check(rc, "groupnorm_act_forward")
    return y, mean, rstd


def groupnorm_act_backward(dy, x, res, gamma, beta, mean, rstd, G, act):
    _chk(dy, x, res, gamma, beta, mean, rstd); _f32(dy, x, res, gamma, beta, mean, rstd)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    dx = torch.empty_like(x)
    dgb = torch.empty((2, C), dtype=torch.float32, device=x.device)          # dgamma | dbeta in one allocation
    dgamma, dbeta = dgb[0].view_as(gamma), dgb[1].view_as(beta)
    rc = _lib.get().pnsfm_groupnorm_act_backward(_ptr(dy), _ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
                                                 _ptr(dx), _ptr(dgamma), _ptr(dbeta), None, B, C, HW, G, act, _stream(x))
    _lib.check(rc, "groupnorm_act_backward")
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------ packing / conv3d
def _is_channel_slice(x):
    """[B,C,H,W] whose images are dense but B-strided (a channel slice of a wider contiguous tensor)."""
    B, C, H, W = x.shape
    st = x.stride()
    return st[3] == 1 and st[2] == W and st[1] == H * W and st[0] >= C * H * W


def space_to_depth(x):
    """x may be contiguous or a channel slice of a wider contiguous NCHW tensor (no copy in either case)."""
    B, C, H, W = x.shape
    if x.is_contiguous() or not _is_channel_slice(x):
        x = x.contiguous()
    _chk(y := torch.empty((B, 4 * C, H // 2, W // 2), dtype=torch.float32, device=x.device)); _f32(x)
    if _lib.REQUIRE_CUDA and not x.is_cuda:
        raise RuntimeError("packnet_sfm HIP op got a %s tensor: the HIP kernels run on MI355X only" % x.device)
    _lib.check(_lib.get().pnsfm_space_to_depth(_ptr(x), _ptr(y), B, C, H, W, x.stride(0) if B > 1 else C * H * W, _stream(x)),
               "space_to_depth")
    return y


def depth_to_space(x):
    _chk(x); _f32(x)
    B, C4, H, W = x.shape
    assert C4 % 4 == 0
    C = C4 // 4
    y = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.get().pnsfm_depth_to_space(_ptr(x), _ptr(y), B, C, H, W, _stream(x)), "depth_to_space")
    return y


def _nf_of(w3):
    """Number of 3-D feature maps of a Conv3d(1, NF, 3) weight [NF,1,3,3,3] (or [NF,27])."""
    nf = w3.shape[0]
    if w3.numel() != nf * 27:
        raise RuntimeError("conv3d: weight must be [NF,1,3,3,3]")
    return nf


def conv3d_forward(p, w3, b3):
    """p [B,D,H,W] -> [B,NF*D,H,W] (channel f*D+d), NF = w3.shape[0] in {4, 8}.  b3 None = no bias."""
    _chk(p, w3, b3); _f32(p, w3, b3)
    B, D, H, W = p.shape
    nf = _nf_of(w3)
    out = torch.empty((B, nf * D, H, W), dtype=torch.float32, device=p.device)
    _lib.check(_lib.get().pnsfm_conv3d_forward(_ptr(p), _ptr(w3), _ptr(b3), _ptr(out), B, D, H, W, nf, _stream(p)),
               "conv3d_forward")
    return out


def conv3d_backward_data(dout, w3):
    _chk(dout, w3); _f32(dout, w3)
    B, DF, H, W = dout.shape
    nf = _nf_of(w3)
    D = DF // nf
    dp = torch.empty((B, D, H, W), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.get().pnsfm_conv3d_backward_data(_ptr(dout), _ptr(w3), _ptr(dp), B, D, H, W, nf, _stream(dout)),
               "conv3d_backward_data")
    return dp


def conv3d_backward_weight(p, dout):
    _chk(p, dout); _f32(p, dout)
    B, D, H, W = p.shape
    nf = dout.shape[1] // D
    dw3 = torch.empty((nf, 1, 3, 3, 3), dtype=torch.float32, device=p.device)
    db3 = torch.empty((nf,), dtype=torch.float32, device=p.device)
    ws = torch.empty((8 * 28,), dtype=torch.float64, device=p.device)
    _lib.check(_lib.get().pnsfm_conv3d_backward_weight(_ptr(p), _ptr(dout), _ptr(dw3), _ptr(db3), _ptr(ws), B, D, H, W, nf,
                                                       _stream(p)), "conv3d_backward_weight")
    return dw3, db3


def set_pack3d_fold(on):
    """include/pnsfm.h, pnsfm_set_pack3d_fold: 0 = the unfolded launch sequences of the packing / unpacking blocks; returns the previous setting."""
    return _lib.get().pnsfm_set_pack3d_fold(int(on))


def conv3d_forward_d2s(p, w3, b3):
    """depth_to_space(conv3d_forward(p, w3, b3)): p [B,D,H,W] -> [B,NF*D/4,2H,2W], one launch where the fold applies (pnsfm.h)."""
    _chk(p, w3, b3); _f32(p, w3, b3)
    B, D, H, W = p.shape
    nf = _nf_of(w3)
    lib = _lib.get()
    y = torch.empty((B, nf * D // 4, 2 * H, 2 * W), dtype=torch.float32, device=p.device)
    tmp = None if lib.pnsfm_conv3d_d2s_folded(_ptr(p), _ptr(y), D, W) else torch.empty((B, nf * D, H, W), dtype=torch.float32, device=p.device)
    _lib.check(lib.pnsfm_conv3d_forward_d2s(_ptr(p), _ptr(w3), _ptr(b3), _ptr(tmp), _ptr(y), B, D, H, W, nf, _stream(p)), "conv3d_forward_d2s")
    return y


def conv3d_rows_folded(p):
    """Does the row window of the three *_rows ops below apply to the strips p [2B,D,S,w] (contiguous)?  pnsfm.h, pnsfm_conv3d_rows_folded
    (torch's allocations are 16-byte aligned: p stands for the output too)."""
    S = p.shape[2]
    return S >= 3 and S % 2 == 1 and p.dtype == torch.float32 and bool(_lib.get().pnsfm_conv3d_rows_folded(_ptr(p), _ptr(p), p.shape[3]))


def conv3d_rows_window_ok(W):
    """conv3d_rows_folded for 16-byte aligned strips of width W that do not exist yet."""
    return bool(_lib.get().pnsfm_conv3d_rows_folded(None, None, int(W)))


def conv3d_forward_rows(p, w3, b3, Bh, tapT=False):
    """Border strips p [2B,D,S,w], S = 2r + 1: the Conv3d rows strip_select(., dim=2) keeps, [2B,NF*D,2r,w].
    tapT: with the taps of w3.transpose(3, 4), read in place."""
    _chk(p, w3, b3); _f32(p, w3, b3)
    B, D, S, W = p.shape
    nf = _nf_of(w3)
    out = torch.empty((B, nf * D, S - 1, W), dtype=torch.float32, device=p.device)
    if tapT:
        rc = _lib.get().pnsfm_conv3d_forward_rows_t(_ptr(p), _ptr(w3), _ptr(b3), _ptr(out), B, D, S, W, nf, Bh, 1, _stream(p))
    else:
        rc = _lib.get().pnsfm_conv3d_forward_rows(_ptr(p), _ptr(w3), _ptr(b3), _ptr(out), B, D, S, W, nf, Bh, _stream(p))
    _lib.check(rc, "conv3d_forward_rows")
    return out


def conv3d_backward_data_rows(dout, w3, S, Bh, tapT=False):
    _chk(dout, w3); _f32(dout, w3)
    B, DF, Ho, W = dout.shape
    nf = _nf_of(w3)
    D = DF // nf
    assert Ho == S - 1
    dp = torch.empty((B, D, S, W), dtype=torch.float32, device=dout.device)
    if tapT:
        rc = _lib.get().pnsfm_conv3d_backward_data_rows_t(_ptr(dout), _ptr(w3), _ptr(dp), B, D, S, W, nf, Bh, 1, _stream(dout))
    else:
        rc = _lib.get().pnsfm_conv3d_backward_data_rows(_ptr(dout), _ptr(w3), _ptr(dp), B, D, S, W, nf, Bh, _stream(dout))
    _lib.check(rc, "conv3d_backward_data_rows")
    return dp


def _dw3_dst(p, nf, dw3_out, db3_out, epi, what):
    if dw3_out is None:
        if epi & WGRAD_EPI_ADD:
            raise RuntimeError("%s: adding into a gradient needs the destination" % what)
        return (torch.empty((nf, 1, 3, 3, 3), dtype=torch.float32, device=p.device), torch.empty((nf,), dtype=torch.float32, device=p.device))
    _chk(dw3_out, db3_out); _f32(dw3_out, db3_out)
    if dw3_out.numel() != nf * 27 or (db3_out is not None and db3_out.numel() != nf):
        raise RuntimeError("%s: gradient slot has the wrong shape" % what)
    # (fresh view objects: see conv2d_backward_weight; db3_out None: the bias gradient is not stored)
    return dw3_out.view(nf, 1, 3, 3, 3), (None if db3_out is None else db3_out.view(nf))


def conv3d_backward_weight_rows(p, dout, Bh, dw3_out=None, db3_out=None, epi=0):
    """epi (WGRAD_EPI_*): ADD -- the gradients are added to what dw3_out / db3_out hold; TAPT -- dw3 with its (y, x) taps swapped back."""
    _chk(p, dout); _f32(p, dout)
    B, D, S, W = p.shape
    nf = dout.shape[1] // D
    assert dout.shape[2] == S - 1
    dw3, db3 = _dw3_dst(p, nf, dw3_out, db3_out, epi, "conv3d_backward_weight_rows")
    if epi:
        rc = _lib.get().pnsfm_conv3d_backward_weight_rows_epi(_ptr(p), _ptr(dout), _ptr(dw3), _ptr(db3), B, D, S, W, nf, Bh, int(epi), _stream(p))
    else:
        rc = _lib.get().pnsfm_conv3d_backward_weight_rows(_ptr(p), _ptr(dout), _ptr(dw3), _ptr(db3), B, D, S, W, nf, Bh, _stream(p))
    _lib.check(rc, "conv3d_backward_weight_rows")
    return dw3, db3


def conv3d_backward_data_ring(dout, w3):
    """conv3d_backward_data(F.pad(dout, (1, 1, 1, 1)), w3) without the padded tensor: dout [B,NF*D,Hd,Wd] -> [B,D,Hd+2,Wd+2]."""
    _chk(dout, w3); _f32(dout, w3)
    B, DF, Hd, Wd = dout.shape
    nf = _nf_of(w3)
    D = DF // nf
    dp = torch.empty((B, D, Hd + 2, Wd + 2), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.get().pnsfm_conv3d_backward_data_ring(_ptr(dout), _ptr(w3), _ptr(dp), B, D, Hd, Wd, nf, _stream(dout)),
               "conv3d_backward_data_ring")
    return dp


def conv3d_backward_weight_ring(p, dout, dw3_out=None, db3_out=None, epi=0):
    """conv3d_backward_weight(p, F.pad(dout, (1, 1, 1, 1))) without the padded tensor: p [B,D,Hd+2,Wd+2], dout [B,NF*D,Hd,Wd].
    dw3_out / db3_out / epi: as conv3d_backward_weight_rows."""
    _chk(p, dout); _f32(p, dout)
    B, D, H, W = p.shape
    nf = dout.shape[1] // D
    assert tuple(dout.shape) == (B, nf * D, H - 2, W - 2)
    dw3, db3 = _dw3_dst(p, nf, dw3_out, db3_out, epi, "conv3d_backward_weight_ring")
    _lib.check(_lib.get().pnsfm_conv3d_backward_weight_ring(_ptr(p), _ptr(dout), _ptr(dw3), _ptr(db3), B, D, H - 2, W - 2, nf, int(epi),
                                                            _stream(p)), "conv3d_backward_weight_ring")
    return dw3, db3


def conv3d_ring_ok():
    """Do the two *_ring ops apply?  The window is read through the buffer descriptors of the default weight-gradient kernel;
    PNSFM_CONV3D_WGRAD_RING=0 (round 3's kernel, an A/B switch) reads whole frames only."""
    return os.environ.get('PNSFM_CONV3D_WGRAD_RING', '1')[:1] != '0'


# ------------------------------------------------------------------- composed packing convolution: bias
def pack_bias_eff_forward(W2, b2, b3):
    """(bias_eff [C], Ssum [C,d]) of the composed packing convolution: include/pnsfm.h, pnsfm_pack_bias_eff_forward."""
    _chk(W2, b2, b3); _f32(W2, b2, b3)
    C, d = W2.shape[0], b3.numel()
    blk = W2[0].numel() // d
    Ssum = torch.empty((C, d), dtype=torch.float32, device=W2.device)
    bias = torch.empty((C,), dtype=torch.float32, device=W2.device)
    _lib.check(_lib.get().pnsfm_pack_bias_eff_forward(_ptr(W2), _ptr(b2), _ptr(b3), _ptr(Ssum), _ptr(bias), C, d, blk, _stream(W2)),
               "pack_bias_eff_forward")
    return bias, Ssum


def pack_bias_eff_backward_add(g, Ssum, b3, dWeff_full, k, db3, dW2, db2=None):
    """pack_bias_eff_backward adding into its destinations: db3 [d] and dW2 [C, d*D, k, k] receive dst + (the plain result), db2 [C]
    (optional) db2 + g."""
    _chk(g, Ssum, b3, dWeff_full, db3, dW2, db2); _f32(g, Ssum, b3, dWeff_full, db3, dW2, db2)
    C, d = Ssum.shape
    D = dWeff_full.shape[1] // d
    assert tuple(dWeff_full.shape) == (C, d * D, k + 2, k + 2) and g.numel() == C
    assert db3.numel() == d and dW2.numel() == C * d * D * k * k and (db2 is None or db2.numel() == C)
    _lib.check(_lib.get().pnsfm_pack_bias_eff_backward_add(_ptr(g), _ptr(Ssum), _ptr(b3), _ptr(dWeff_full), _ptr(db3), _ptr(dW2), _ptr(db2), C, d,
                                                           D, k, _stream(g)), "pack_bias_eff_backward_add")


def pack_bias_eff_backward(g, Ssum, b3, dWeff_full, k, want_db3=True, want_dW2=True):
    """g [C] = d(bias_eff); dWeff_full [C, d*D, k+2, k+2] = the composition's gradient on the padded taps.
    Returns (db3 [d] or None, dW2 [C, d*D, k, k] or None)."""
    _chk(g, Ssum, b3, dWeff_full); _f32(g, Ssum, b3, dWeff_full)
    C, d = Ssum.shape
    D = dWeff_full.shape[1] // d
    assert tuple(dWeff_full.shape) == (C, d * D, k + 2, k + 2) and g.numel() == C
    db3 = torch.empty((d,), dtype=torch.float32, device=g.device) if want_db3 else None
    dW2 = torch.empty((C, d * D, k, k), dtype=torch.float32, device=g.device) if want_dW2 else None
    _lib.check(_lib.get().pnsfm_pack_bias_eff_backward(_ptr(g), _ptr(Ssum), _ptr(b3), _ptr(dWeff_full), _ptr(db3), _ptr(dW2), C, d, D,
                                                       k, _stream(g)), "pack_bias_eff_backward")
    return db3, dW2


# --------------------------------------------------------------------------------- nearest up-sampling
def upsample_nearest_ok(x, s):
    return x.dim() == 4 and x.dtype == torch.float32 and s >= 1 and (x.shape[3] * s) % 4 == 0 and x.numel() * s * s < 2 ** 32


def upsample_nearest_forward(x, s):
    _chk(x); _f32(x)
    B, C, h, w = x.shape
    y = torch.empty((B, C, h * s, w * s), dtype=torch.float32, device=x.device)
    _lib.check(_lib.get().pnsfm_upsample_nearest_forward(_ptr(x), _ptr(y), B * C, h, w, s, _stream(x)), "upsample_nearest_forward")
    return y


def upsample_nearest_backward(dy, s):
    _chk(dy); _f32(dy)
    B, C, Ho, Wo = dy.shape
    h, w = Ho // s, Wo // s
    dx = torch.empty((B, C, h, w), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.get().pnsfm_upsample_nearest_backward(_ptr(dy), _ptr(dx), B * C, h, w, s, _stream(dy)), "upsample_nearest_backward")
    return dx


# ------------------------------------------------------------------------------------- ResNet networks
ACT_DISP = 3                      # act_crop only: p0 + p1 * sigmoid(z)
BN_PATH_FUSED, BN_PATH_CHUNKED, BN_PATH_EVAL = 0, 1, 2
BN_FUSE_UNITS = 2048              # kBnFuseUnits of csrc/resnet.h: path 0 up to this many float4 (HW % 4 == 0) or floats per channel


def batchnorm_last_path():
    """The path the last batchnorm_act launch (either direction) took: BN_PATH_*; -1 before the first."""
    return int(_lib.get().pnsfm_batchnorm_last_path())


def _bn_shape(x):
    if x.dim() < 2:
        raise ValueError("batchnorm_act needs a [B, C, ...] tensor, got %s" % (tuple(x.shape),))
    B, C = x.shape[0], x.shape[1]
    return B, C, (x.numel() // (B * C) if B * C else 0)


def batchnorm_act_forward(x, res, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, act, training):
    """y = act(BN(x) + res) -> (y, stats): stats [2, C] float64 = mean | rstd (None in eval mode).  In training mode the running
    statistics and the step counter (all nullable) are updated on the device."""
    _chk(x, res, gamma, beta, running_mean, running_var, num_batches_tracked); _f32(x, res, gamma, beta, running_mean, running_var)
    B, C, HW = _bn_shape(x)
    if training and B * HW == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise RuntimeError("batchnorm_act: num_batches_tracked must be int64")
    y = torch.empty_like(x)
    stats = torch.empty((2, C), dtype=torch.float64, device=x.device) if training else None
    rc = _lib.get().pnsfm_batchnorm_act_forward(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                                _ptr(num_batches_tracked), _ptr(y), _ptr(stats), B, C, HW, float(eps), float(momentum),
                                                act, 1 if training else 0, _stream(x))
    _lib.check(rc, "batchnorm_act_forward")
    return y, stats


def batchnorm_act_backward(dy, y, x, gamma, stats, running_mean, running_var, eps, act, want_dres):
    """-> (dx, dres or None, dgamma, dbeta).  stats: the forward's [2, C] float64 (training) or None (eval: running statistics).  With
    act == ACT_NONE the residual's gradient is dy itself: nothing is written for it (the caller hands dy on)."""
    _chk(dy, y, x, gamma, stats, running_mean, running_var); _f32(dy, y, x, gamma, running_mean, running_var)
    B, C, HW = _bn_shape(x)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if (want_dres and act != ACT_NONE) else None
    dgb = torch.empty((2, C), dtype=torch.float32, device=x.device)
    rc = _lib.get().pnsfm_batchnorm_act_backward(_ptr(dy), _ptr(y), _ptr(x), _ptr(gamma), _ptr(stats), _ptr(running_mean), _ptr(running_var),
                                                 _ptr(dx), _ptr(dres), _ptr(dgb[0]), _ptr(dgb[1]), B, C, HW, float(eps), act,
                                                 0 if stats is None else 1, _stream(x))
    _lib.check(rc, "batchnorm_act_backward")
    return dx, dres, dgb[0], dgb[1]


def _planes(x, what):
    if x.dim() < 2:
        raise ValueError("%s needs a [..., H, W] tensor, got %s" % (what, tuple(x.shape)))
    H, W = x.shape[-2], x.shape[-1]
    return (x.numel() // (H * W) if H * W else 0), H, W


def maxpool3x3s2_forward(x):
    """x [..., H, W] -> (y [..., Ho, Wo], arg uint8 of y's shape: the window slot of the maximum)."""
    _chk(x); _f32(x)
    N, H, W = _planes(x, "maxpool3x3s2")
    shape = tuple(x.shape[:-2]) + ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    arg = torch.empty(shape, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.get().pnsfm_maxpool3x3s2_forward(_ptr(x), _ptr(y), _ptr(arg), N, H, W, _stream(x)), "maxpool3x3s2_forward")
    return y, arg


def maxpool3x3s2_backward(dy, arg, in_shape):
    _chk(dy, arg); _f32(dy)
    dx = torch.empty(tuple(in_shape), dtype=torch.float32, device=dy.device)
    N, H, W = _planes(dx, "maxpool3x3s2")
    _lib.check(_lib.get().pnsfm_maxpool3x3s2_backward(_ptr(dy), _ptr(arg), _ptr(dx), N, H, W, _stream(dy)), "maxpool3x3s2_backward")
    return dx


def reflect_pad1_forward(xs, ups, pitch=None):
    """pitch: the output's width (>= W + 2; default W + 2), the columns from W + 2 on zero.  xs: [B, C_i, h_i, w_i] tensors, ups: one up-sampling factor (1 | 2) each, with every s_i h_i x s_i w_i the same H x W ->
    [B, sum C_i, H + 2, W + 2]: each source (nearest up-sampled by its factor, then) reflection-padded by 1 into its channel range."""
    _chk(*xs); _f32(*xs)
    B = xs[0].shape[0]
    H, W = ups[0] * xs[0].shape[2], ups[0] * xs[0].shape[3]
    for t, s in zip(xs, ups):
        if t.dim() != 4 or t.shape[0] != B or (s * t.shape[2], s * t.shape[3]) != (H, W) or s not in (1, 2):
            raise ValueError("reflect_pad1: sources %s with factors %s do not share one batch and size" % ([tuple(t.shape) for t in xs], list(ups)))
    Ctot = sum(t.shape[1] for t in xs)
    Wp = W + 2 if pitch is None else int(pitch)
    if Wp < W + 2:
        raise ValueError("reflect_pad1: pitch %d is narrower than the padded map (%d)" % (Wp, W + 2))
    y = torch.empty((B, Ctot, H + 2, Wp), dtype=torch.float32, device=xs[0].device)
    c0 = 0
    for t, s in zip(xs, ups):
        C, h, w = t.shape[1:]
        _lib.check(_lib.get().pnsfm_reflect_pad1_forward(_ptr(t), _ptr(y), B, C, h, w, s, Ctot, c0, Wp, _stream(t)), "reflect_pad1_forward")
        c0 += C
    return y


def reflect_pad1_backward(dy, shapes, ups, needs):
    """dy [B, sum C_i, H + 2, W + 2] -> one gradient (or None where `needs` says so) per source of reflect_pad1_forward."""
    _chk(dy); _f32(dy)
    B, Ctot = dy.shape[0], dy.shape[1]
    out, c0 = [], 0
    for shape, s, need in zip(shapes, ups, needs):
        C, h, w = shape[1:]
        dx = None
        if need:
            dx = torch.empty(tuple(shape), dtype=torch.float32, device=dy.device)
            _lib.check(_lib.get().pnsfm_reflect_pad1_backward(_ptr(dy), _ptr(dx), B, C, h, w, s, Ctot, c0, dy.shape[3], _stream(dy)), "reflect_pad1_backward")
        out.append(dx)
        c0 += C
    return out


def act_crop_forward(z, m, act, p0=0.0, p1=1.0, width=None):
    """width: the output's width where z is wider than width + 2 m (a pitched map of reflect_pad1_forward); default: all of z."""
    _chk(z); _f32(z)
    N, Hz, Wz = _planes(z, "act_crop")
    H, W = Hz - 2 * m, (Wz - 2 * m if width is None else int(width))
    if W + 2 * m > Wz:
        raise ValueError("act_crop: width %d + crop does not fit the %d columns" % (W, Wz))
    if m not in (0, 1) or H < 1 or W < 1:
        raise ValueError("act_crop: crop %d of a %d x %d map" % (m, Hz, Wz))
    y = torch.empty(tuple(z.shape[:-2]) + (H, W), dtype=torch.float32, device=z.device)
    _lib.check(_lib.get().pnsfm_act_crop_forward(_ptr(z), _ptr(y), N, H, W, m, Wz, act, float(p0), float(p1), _stream(z)), "act_crop_forward")
    return y


def act_crop_backward(dy, y, m, act, p0=0.0, p1=1.0, in_width=None):
    _chk(dy, y); _f32(dy, y)
    N, H, W = _planes(y, "act_crop")
    Wz = W + 2 * m if in_width is None else int(in_width)
    dz = torch.empty(tuple(y.shape[:-2]) + (H + 2 * m, Wz), dtype=torch.float32, device=y.device)
    _lib.check(_lib.get().pnsfm_act_crop_backward(_ptr(dy), _ptr(y), _ptr(dz), N, H, W, m, Wz, act, float(p0), float(p1), _stream(y)),
               "act_crop_backward")
    return dz


def affine(x, s, t):
    """x * s + t."""
    _chk(x); _f32(x)
    y = torch.empty_like(x)
    if x.numel():
        _lib.check(_lib.get().pnsfm_affine(_ptr(x), _ptr(y), x.numel(), float(s), float(t), _stream(x)), "affine")
    return y


# ------------------------------------------------------------------------------- scalar tail of the loss
def loss_combine_forward(photometric, smoothness, weight):
    """photometric / smoothness: lists of 0-dim device tensors -> out3 = (loss, weighted smoothness, photometric)."""
    n, ns = len(photometric), len(smoothness)
    ts = list(photometric) + list(smoothness)
    _chk(*ts); _f32(*ts)
    P = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in photometric])
    S = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in smoothness])
    out = torch.empty((3,), dtype=torch.float32, device=ts[0].device)
    _lib.check(_lib.get().pnsfm_loss_combine_forward(ctypes.byref(P), n, ctypes.byref(S), ns, float(weight), _ptr(out), _stream(out)), "loss_combine_forward")
    return out


def loss_combine_backward(g, n, ns, weight):
    """g: 0-dim device tensor -> [16]: entries i < n = d/dP[i], 8 + i (i < ns) = d/dS[i]."""
    _chk(g); _f32(g)
    dout = torch.empty((16,), dtype=torch.float32, device=g.device)
    _lib.check(_lib.get().pnsfm_loss_combine_backward(_ptr(g), n, ns, float(weight), _ptr(dout), _stream(g)), "loss_combine_backward")
    return dout


# ------------------------------------------------------------------------------- velocity supervision
def _velocity_tables(pred_mats, gt_mats):
    """The two host tables of device pointers (include/pnsfm.h "velocity supervision") for lists of [B,4,4] fp32 stacks."""
    J = len(pred_mats)
    if J < 1 or len(gt_mats) != J:
        raise ValueError("velocity_loss needs as many ground-truth stacks as predicted ones, at least one (got %d, %d)" % (len(gt_mats), J))
    ts = list(pred_mats) + list(gt_mats)
    _chk(*ts); _f32(*ts)
    B = pred_mats[0].shape[0]
    for t in ts:
        if tuple(t.shape) != (B, 4, 4):
            raise ValueError("velocity_loss needs [B,4,4] stacks of one batch size, got %s" % (tuple(t.shape),))
    n = max(J, 1)                                  # the library checks J against its maximum: pass every pointer through
    P = (ctypes.c_void_p * n)(*[t.data_ptr() for t in pred_mats])
    G = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gt_mats])
    return P, G, J, B


def velocity_loss_forward(pred_mats, gt_mats, weight, loss_in=None):
    """pred_mats / gt_mats: lists of J [B,4,4] stacks -> out2 = (L, loss_in + weight * L); loss_in: 1-element device tensor or None."""
    P, G, J, B = _velocity_tables(pred_mats, gt_mats)
    _chk(pred_mats[0], loss_in); _f32(loss_in)
    out = torch.empty((2,), dtype=torch.float32, device=pred_mats[0].device)
    _lib.check(_lib.get().pnsfm_velocity_loss_forward(ctypes.byref(P), ctypes.byref(G), J, B, float(weight), _ptr(loss_in), _ptr(out),
                                                      _stream(out)), "velocity_loss_forward")
    return out


def velocity_loss_backward(pred_mats, gt_mats, weight, upstream):
    """upstream: 1-element device tensor = d/d(out2[1]) -> [J,B,4,4]: the gradient of every predicted stack, all entries written."""
    P, G, J, B = _velocity_tables(pred_mats, gt_mats)
    _chk(pred_mats[0], upstream); _f32(upstream)
    dpred = torch.empty((J, B, 4, 4), dtype=torch.float32, device=upstream.device)
    _lib.check(_lib.get().pnsfm_velocity_loss_backward(ctypes.byref(P), ctypes.byref(G), J, B, float(weight), _ptr(upstream),
                                                       _ptr(dpred), _stream(dpred)), "velocity_loss_backward")
    return dpred


# ------------------------------------------------------------------------------------------ invdepth
def invdepth_act_forward(x, min_depth):
    _chk(x); _f32(x)
    y = torch.empty_like(x)
    _lib.check(_lib.get().pnsfm_invdepth_act_forward(_ptr(x), _ptr(y), x.numel(), float(min_depth), _stream(x)),
               "invdepth_act_forward")
    return y


def invdepth_act_backward(dy, y, min_depth):
    _chk(dy, y); _f32(dy, y)
    dx = torch.empty_like(y)
    _lib.check(_lib.get().pnsfm_invdepth_act_backward(_ptr(dy), _ptr(y), _ptr(dx), y.numel(), float(min_depth), _stream(y)),
               "invdepth_act_backward")
    return dx


def invdepth_conv_forward(x, w, bias, min_depth):
    """x [B,C,H,W], w [1,C,3,3], bias [1] -> sigmoid(conv3x3(x) + b) / min_depth, [B,1,H,W]."""
    _chk(x, w, bias); _f32(x, w, bias)
    B, C, H, W = x.shape
    if tuple(w.shape) != (1, C, 3, 3) or bias is None or bias.numel() != 1:
        raise RuntimeError("invdepth_conv: weight must be [1,%d,3,3] with a bias of one element" % C)
    y = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.get().pnsfm_invdepth_conv_forward(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, C, H, W, float(min_depth),
                                                      _stream(x)), "invdepth_conv_forward")
    return y


def invdepth_conv_backward(x, w, dz):
    """dz [B,1,H,W] = gradient at the conv output -> (dx [B,C,H,W], dw [1,C,3,3], db [1])."""
    _chk(x, w, dz); _f32(x, w, dz)
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    buf = torch.empty((C * 9 + 1,), dtype=torch.float32, device=x.device)      # db right behind dw: one fill
    dw, db = buf[:C * 9].view(1, C, 3, 3), buf[C * 9:]
    _lib.check(_lib.get().pnsfm_invdepth_conv_backward(_ptr(x), _ptr(w), _ptr(dz), _ptr(dx), _ptr(dw), _ptr(db), B, C, H, W,
                                                       _stream(x)), "invdepth_conv_backward")
    return dx, dw, db


def pose_vec2mat_forward(vec):
    _chk(vec); _f32(vec)
    N = vec.shape[0]
    mat = torch.empty((N, 4, 4), dtype=torch.float32, device=vec.device)
    _lib.check(_lib.get().pnsfm_pose_vec2mat_forward(_ptr(vec), _ptr(mat), N, _stream(vec)), "pose_vec2mat_forward")
    return mat


def pose_vec2mat_backward(vec, dmat):
    _chk(vec, dmat); _f32(vec, dmat)
    N = vec.shape[0]
    dvec = torch.empty((N, 6), dtype=torch.float32, device=vec.device)
    _lib.check(_lib.get().pnsfm_pose_vec2mat_backward(_ptr(vec), _ptr(dmat), _ptr(dvec), N, _stream(vec)),
               "pose_vec2mat_backward")
    return dvec


# ---------------------------------------------------------------------------------------------- loss
PADDING_MODES = {'zeros': 0, 'border': 1, 'reflection': 2}     # F.grid_sample's padding_mode (align_corners=True)


def view_synthesis_forward(inv_depth, ref, K, refK, T, padding_mode=0):
    """inv_depth [B,1,H,W]; ref [J,B,3,H,W]; K, refK [B,3,3]; T [J,B,4,4] -> warped [J,B,3,H,W]."""
    _chk(inv_depth, ref, K, refK, T); _f32(inv_depth, ref, K, refK, T)
    J, B, _, H, W = ref.shape
    warped = torch.empty_like(ref)
    _lib.check(_lib.get().pnsfm_view_synthesis_forward(_ptr(inv_depth), _ptr(ref), _ptr(K), _ptr(refK), _ptr(T), _ptr(warped),
                                                       J, B, H, W, int(padding_mode), _stream(ref)), "view_synthesis_forward")
    return warped


def view_synthesis_backward(d_warped, inv_depth, ref, K, refK, T, padding_mode=0):
    _chk(d_warped, inv_depth, ref, K, refK, T); _f32(d_warped, inv_depth, ref, K, refK, T)
    J, B, _, H, W = ref.shape
    d_inv = torch.empty_like(inv_depth)
    dT = torch.empty_like(T)
    _lib.check(_lib.get().pnsfm_view_synthesis_backward(_ptr(d_warped), _ptr(inv_depth), _ptr(ref), _ptr(K), _ptr(refK), _ptr(T),
                                                        _ptr(d_inv), _ptr(dT), J, B, H, W, int(padding_mode), _stream(ref)),
               "view_synthesis_backward")
    return d_inv, dT


def _upstream_ptr(upstream):
    """the optional float32 device scalar that a backward kernel multiplies its gradient by (None: null pointer = 1)"""
    _chk(upstream); _f32(upstream)
    return _ptr(upstream)


def photometric_forward(warped, ref, target, ssim_weight, C1, C2, automask, reduce_op, clip_loss=0.0):
    """-> (loss, argmin uint8[B,H,W]).  loss: float32[1] = pixel mean of the reduced photometric map; with clip_loss > 0 (candidates
    clamped at mean + clip_loss*std) float64[1] = its pixel SUM, which the caller divides."""
    _chk(warped, ref, target); _f32(warped, ref, target)
    J, B, _, H, W = warped.shape
    clip = clip_loss > 0.0
    loss = torch.empty((1,), dtype=torch.float64 if clip else torch.float32, device=warped.device)
    argmin = torch.empty((B, H, W), dtype=torch.uint8, device=warped.device)
    _lib.check(_lib.get().pnsfm_photometric_forward(_ptr(warped), _ptr(ref), _ptr(target), _ptr(loss if clip else None),
                                                    _ptr(None if clip else loss), _ptr(argmin), J, B, H, W, float(ssim_weight),
                                                    float(C1), float(C2), int(automask), int(reduce_op), float(clip_loss),
                                                    _stream(warped)), "photometric_forward")
    return loss, argmin


def photometric_backward(warped, target, argmin, grad_scale, upstream, ssim_weight, C1, C2, automask, reduce_op, clip=False):
    """d_warped = grad_scale * upstream[0] * d(loss_sum)/d(warped); `upstream`: float32 device scalar (or None)."""
    _chk(warped, target, argmin); _f32(warped, target)
    J, B, _, H, W = warped.shape
    d_warped = torch.empty_like(warped)
    _lib.check(_lib.get().pnsfm_photometric_backward(_ptr(warped), _ptr(target), _ptr(argmin), _ptr(d_warped), float(grad_scale),
                                                     _upstream_ptr(upstream), J, B, H, W, float(ssim_weight), float(C1), float(C2),
                                                     int(automask), int(reduce_op), int(bool(clip)), _stream(warped)),
               "photometric_backward")
    return d_warped


def photometric_l1_forward(warped, ref, target, automask, reduce_op, clip_loss):
    """L1-only photometric loss on per-channel candidate maps -> (loss float32[1], rec int32[B,H,W])."""
    _chk(warped, ref, target); _f32(warped, ref, target)
    J, B, _, H, W = warped.shape
    loss = torch.empty((1,), dtype=torch.float32, device=warped.device)
    rec = torch.empty((B, H, W), dtype=torch.int32, device=warped.device)
    _lib.check(_lib.get().pnsfm_photometric_l1_forward(_ptr(warped), _ptr(ref), _ptr(target), _ptr(loss), _ptr(rec), J, B, H, W,
                                                       int(automask), int(reduce_op), float(clip_loss), _stream(warped)),
               "photometric_l1_forward")
    return loss, rec


def photometric_l1_backward(warped, target, rec, grad_scale, upstream, automask, reduce_op):
    _chk(warped, target, rec); _f32(warped, target)
    J, B, _, H, W = warped.shape
    d_warped = torch.empty_like(warped)
    _lib.check(_lib.get().pnsfm_photometric_l1_backward(_ptr(warped), _ptr(target), _ptr(rec), _ptr(d_warped), float(grad_scale),
                                                        _upstream_ptr(upstream), J, B, H, W, int(automask), int(reduce_op),
                                                        _stream(warped)),
               "photometric_l1_backward")
    return d_warped


def smoothness_norm_forward(inv_depth, image):
    """-> (loss float32[1], mean float32[B]): smoothness of inv_depth / clamp(mean_hw(inv_depth), 1e-6)."""
    _chk(inv_depth, image); _f32(inv_depth, image)
    B, _, H, W = image.shape
    loss = torch.empty((1,), dtype=torch.float32, device=image.device)
    mean = torch.empty((B,), dtype=torch.float32, device=image.device)
    _lib.check(_lib.get().pnsfm_smoothness_norm_forward(_ptr(inv_depth), _ptr(image), _ptr(loss), _ptr(mean), B, H, W, _stream(image)),
               "smoothness_norm_forward")
    return loss, mean


def smoothness_norm_backward(inv_depth, image, mean, upstream):
    _chk(inv_depth, image, mean); _f32(inv_depth, image, mean)
    B, _, H, W = image.shape
    d = torch.empty_like(inv_depth)
    _lib.check(_lib.get().pnsfm_smoothness_norm_backward(_ptr(inv_depth), _ptr(image), _ptr(mean), _upstream_ptr(upstream), _ptr(d),
                                                         B, H, W, _stream(image)), "smoothness_norm_backward")
    return d


# ---- all scales in one launch (include/pnsfm.h "all scales in one launch") ----
LOSS_MAX_SCALES = 8      # PNSFM_LOSS_MAX_SCALES of include/pnsfm.h (the library refuses more: "n must be 1..8 scales")


def _ptr_table(tensors):
    """HOST array of the device pointers of `tensors` (None: null).  Lengths are not checked here: the library refuses n < 1 and
    n > LOSS_MAX_SCALES (the smoothness wrappers, which need a first image for B and the device, refuse an empty list themselves)"""
    return (ctypes.c_void_p * max(len(tensors), 1))(*[None if t is None else t.data_ptr() for t in tensors])


def _upstream_table(upstream, n):
    """the optional list of n float32 device scalars that a backward kernel multiplies each scale's gradient by"""
    if upstream is None:
        return None
    if len(upstream) != n:
        raise ValueError("need one upstream scalar per scale (got %d for %d scales)" % (len(upstream), n))
    _chk(*upstream); _f32(*upstream)
    return ctypes.byref(_ptr_table(upstream))


def view_synthesis_forward_ms(inv_depths, ref, K, refK, T, padding_mode=0):
    """inv_depths: n x [B,1,H,W] -> warped [n,J,B,3,H,W], one launch."""
    _chk(ref, K, refK, T, *inv_depths); _f32(ref, K, refK, T, *inv_depths)
    J, B, _, H, W = ref.shape
    n = len(inv_depths)
    warped = torch.empty((max(n, 1),) + tuple(ref.shape), dtype=torch.float32, device=ref.device)
    _lib.check(_lib.get().pnsfm_view_synthesis_forward_ms(ctypes.byref(_ptr_table(inv_depths)), n, _ptr(ref), _ptr(K), _ptr(refK), _ptr(T),
                                                          _ptr(warped), J, B, H, W, int(padding_mode), _stream(ref)),
               "view_synthesis_forward_ms")
    return warped


def view_synthesis_backward_ms(d_warped, inv_depths, ref, K, refK, T, padding_mode=0):
    """d_warped [n,J,B,3,H,W] -> (d_inv [n,B,1,H,W], dT [J,B,4,4] summed over the scales), two launches."""
    _chk(d_warped, ref, K, refK, T, *inv_depths); _f32(d_warped, ref, K, refK, T, *inv_depths)
    J, B, _, H, W = ref.shape
    n = len(inv_depths)
    d_inv = torch.empty((max(n, 1), B, 1, H, W), dtype=torch.float32, device=ref.device)
    dT = torch.empty_like(T)
    _lib.check(_lib.get().pnsfm_view_synthesis_backward_ms(_ptr(d_warped), ctypes.byref(_ptr_table(inv_depths)), n, _ptr(ref), _ptr(K),
                                                           _ptr(refK), _ptr(T), ctypes.byref(_ptr_table([d_inv[i] for i in range(n)])),
                                                           _ptr(dT), J, B, H, W, int(padding_mode), _stream(ref)),
               "view_synthesis_backward_ms")
    return d_inv, dT


def photometric_identity_forward(ref, target, ssim_weight, C1, C2):
    """-> id [J,B,H,W]: the per-pixel loss of the unwarped candidates ref[j] against target."""
    _chk(ref, target); _f32(ref, target)
    J, B, _, H, W = ref.shape
    idmap = torch.empty((J, B, H, W), dtype=torch.float32, device=ref.device)
    _lib.check(_lib.get().pnsfm_photometric_identity_forward(_ptr(ref), _ptr(target), _ptr(idmap), J, B, H, W, float(ssim_weight),
                                                             float(C1), float(C2), _stream(ref)), "photometric_identity_forward")
    return idmap


def photometric_forward_ms(warped, idmap, target, ssim_weight, C1, C2, automask, reduce_op):
    """warped [n,J,B,3,H,W] -> (loss float32[n], argmin uint8[n,B,H,W]); idmap: photometric_identity_forward's, needed under automask."""
    _chk(warped, idmap, target); _f32(warped, idmap, target)
    n, J, B, _, H, W = warped.shape
    loss = torch.empty((n,), dtype=torch.float32, device=warped.device)
    argmin = torch.empty((n, B, H, W), dtype=torch.uint8, device=warped.device)
    _lib.check(_lib.get().pnsfm_photometric_forward_ms(_ptr(warped), _ptr(idmap), _ptr(target), _ptr(loss), _ptr(argmin), n, J, B, H, W,
                                                       float(ssim_weight), float(C1), float(C2), int(automask), int(reduce_op),
                                                       _stream(warped)), "photometric_forward_ms")
    return loss, argmin


def photometric_backward_ms(warped, target, argmin, grad_scale, upstream, ssim_weight, C1, C2, automask, reduce_op):
    """d_warped [n,J,B,3,H,W]; upstream: list of n float32 device scalars (or None)."""
    _chk(warped, target, argmin); _f32(warped, target)
    n, J, B, _, H, W = warped.shape
    d_warped = torch.empty_like(warped)
    _lib.check(_lib.get().pnsfm_photometric_backward_ms(_ptr(warped), _ptr(target), _ptr(argmin), _ptr(d_warped), float(grad_scale),
                                                        _upstream_table(upstream, n), n, J, B, H, W, float(ssim_weight), float(C1),
                                                        float(C2), int(automask), int(reduce_op), _stream(warped)),
               "photometric_backward_ms")
    return d_warped


def _sn_tables(inv_depths, images):
    n = len(inv_depths)
    if n < 1:
        raise ValueError("smoothness_norm: needs at least one scale")
    if len(images) != n:
        raise ValueError("need one image per inverse-depth map (got %d for %d)" % (len(images), n))
    _chk(*inv_depths, *images); _f32(*inv_depths, *images)
    B = images[0].shape[0]
    for d, im in zip(inv_depths, images):
        if tuple(im.shape) != (B, 3) + tuple(d.shape[-2:]) or tuple(d.shape[:2]) != (B, 1):
            raise ValueError("smoothness_norm: inverse depth %s does not go with image %s" % (tuple(d.shape), tuple(im.shape)))
    Hs = (ctypes.c_int * n)(*[d.shape[-2] for d in inv_depths])
    Ws = (ctypes.c_int * n)(*[d.shape[-1] for d in inv_depths])
    return n, B, ctypes.byref(_ptr_table(inv_depths)), ctypes.byref(_ptr_table(images)), ctypes.byref(Hs), ctypes.byref(Ws)


def smoothness_norm_forward_ms(inv_depths, images):
    """n scales, each at its own resolution -> (loss float32[n], mean float32[n,B]), three launches."""
    n, B, pi, pim, pH, pW = _sn_tables(inv_depths, images)
    dev = images[0].device
    loss = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
    mean = torch.empty((max(n, 1), B), dtype=torch.float32, device=dev)
    _lib.check(_lib.get().pnsfm_smoothness_norm_forward_ms(pi, pim, pH, pW, n, _ptr(loss), _ptr(mean), B, _stream(images[0])),
               "smoothness_norm_forward_ms")
    return loss, mean


def smoothness_norm_backward_ms(inv_depths, images, mean, upstream, d_inv=None):
    """-> the list of n gradients.  d_inv: optional list of n tensors that hold another term of the gradient; the smoothness term is
    then ADDED to them in place (one rounded sum per element) and they are returned."""
    n, B, pi, pim, pH, pW = _sn_tables(inv_depths, images)
    _chk(mean); _f32(mean)
    acc = d_inv is not None
    if acc:
        _chk(*d_inv); _f32(*d_inv)
        if len(d_inv) != n or any(g.shape != d.shape for g, d in zip(d_inv, inv_depths)):
            raise ValueError("smoothness_norm_backward_ms: d_inv must match the inverse-depth maps")
    else:
        d_inv = [torch.empty_like(d) for d in inv_depths]
    _lib.check(_lib.get().pnsfm_smoothness_norm_backward_ms(pi, pim, pH, pW, n, _ptr(mean), _upstream_table(upstream, n),
                                                            ctypes.byref(_ptr_table(d_inv)), int(acc), B, _stream(images[0])),
               "smoothness_norm_backward_ms")
    return list(d_inv)


def smoothness_forward(inv_norm, image):
    _chk(inv_norm, image); _f32(inv_norm, image)
    B, _, H, W = image.shape
    sums = torch.empty((2,), dtype=torch.float64, device=image.device)
    _lib.check(_lib.get().pnsfm_smoothness_forward(_ptr(inv_norm), _ptr(image), _ptr(sums), B, H, W, _stream(image)),
               "smoothness_forward")
    return sums


def smoothness_backward(inv_norm, image, gx, gy):
    _chk(inv_norm, image); _f32(inv_norm, image)
    B, _, H, W = image.shape
    d = torch.empty_like(inv_norm)
    _lib.check(_lib.get().pnsfm_smoothness_backward(_ptr(inv_norm), _ptr(image), _ptr(d), float(gx), float(gy), B, H, W,
                                                    _stream(image)), "smoothness_backward")
    return d


# ---------------------------------------------------------------------------------- supervised loss
SUP_METHODS = {'l1': 0, 'mse': 1, 'abs_rel': 2, 'berhu': 3, 'silog': 4}


def supervised_loss_forward(pred, gt, method, sparse):
    """pred, gt: same-shape fp32 tensors -> (loss [1] fp32, ws for the backward call)."""
    _chk(pred, gt); _f32(pred, gt)
    if pred.shape != gt.shape:
        raise RuntimeError("supervised_loss: prediction %s and ground truth %s differ in shape" % (tuple(pred.shape), tuple(gt.shape)))
    loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
    ws = torch.empty((8 + 1024,), dtype=torch.float64, device=pred.device)
    _lib.check(_lib.get().pnsfm_supervised_loss_forward(_ptr(pred), _ptr(gt), _ptr(loss), _ptr(ws), pred.numel(), int(method),
                                                        int(bool(sparse)), _stream(pred)), "supervised_loss_forward")
    return loss, ws


def supervised_loss_backward(pred, gt, ws, grad_out, method, sparse):
    _chk(pred, gt, ws, grad_out); _f32(pred, gt, grad_out)
    dpred = torch.empty_like(pred)
    _lib.check(_lib.get().pnsfm_supervised_loss_backward(_ptr(pred), _ptr(gt), _ptr(ws), _ptr(grad_out), _ptr(dpred),
                                                         pred.numel(), int(method), int(bool(sparse)), _stream(pred)),
               "supervised_loss_backward")
    return dpred


# ---------------------------------------------------------------------------------- depth evaluation
PP_METHODS = {'mean': 0, 'max': 1, 'min': 2}
SCALE_OUTPUTS = {'resize': 0, 'top-center': 1}


def _f32_or_h16(*tensors):
    for t in tensors:
        if t.dtype not in (torch.float32, torch.float16):
            raise RuntimeError("packnet_sfm depth-evaluation op needs float32 or float16 tensors, got %s" % t.dtype)


def _b1hw(t, what):
    if t.dim() != 4 or t.shape[1] != 1:
        raise RuntimeError("%s must be [B,1,H,W], got %s" % (what, tuple(t.shape)))


def post_process_inv_depth(inv, inv_flipped, method):
    """inv, inv_flipped: [B,1,H,W], fp32 or fp16 -> the flip-and-fuse map in inv's dtype (one launch)."""
    _chk(inv, inv_flipped); _f32_or_h16(inv, inv_flipped); _b1hw(inv, "post_process_inv_depth: inv_depth")
    if inv.shape != inv_flipped.shape:
        raise RuntimeError("post_process_inv_depth: %s and its flipped counterpart %s differ in shape" % (tuple(inv.shape), tuple(inv_flipped.shape)))
    B, _, H, W = inv.shape
    out = torch.empty_like(inv)
    h = [int(t.dtype == torch.float16) for t in (inv, inv_flipped, out)]
    _lib.check(_lib.get().pnsfm_post_process_inv_depth(_ptr(inv), h[0], _ptr(inv_flipped), h[1], _ptr(out), h[2], B, H, W, int(method),
                                                       _stream(inv)), "post_process_inv_depth")
    return out


def depth_metrics(gt, pred, min_depth, max_depth, window, scale_output, use_gt_scale, pred_is_inverse, dump=False):
    """gt [B,1,Hg,Wg], pred [B,1,Hp,Wp] (fp32 or fp16 each); window = (y1, y2, x1, x2) rows / columns of gt that count.
    -> (metrics [7] fp32, rows [B,8] fp32, ws int32 words (its first 2B words: the fp32 medians), sampled [B,1,Hg,Wg] fp32 | None),
    all on gt's device; nothing is copied to the host."""
    _chk(gt, pred); _f32_or_h16(gt, pred); _b1hw(gt, "depth_metrics: gt"); _b1hw(pred, "depth_metrics: pred")
    if pred.shape[0] != gt.shape[0]:
        raise RuntimeError("depth_metrics: gt %s and pred %s differ in batch size" % (tuple(gt.shape), tuple(pred.shape)))
    B, _, Hg, Wg = gt.shape
    lib = _lib.get()
    metrics = torch.empty((7,), dtype=torch.float32, device=gt.device)
    rows = torch.empty((B, 8), dtype=torch.float32, device=gt.device)
    ws = torch.empty((int(lib.pnsfm_depth_metrics_ws_bytes(B)) // 8,), dtype=torch.float64, device=gt.device).view(torch.int32)
    sampled = torch.empty((B, 1, Hg, Wg), dtype=torch.float32, device=gt.device) if dump else None
    y1, y2, x1, x2 = (int(v) for v in window)
    _lib.check(lib.pnsfm_depth_metrics(_ptr(gt), int(gt.dtype == torch.float16), _ptr(pred), int(pred.dtype == torch.float16),
                                       _ptr(metrics), _ptr(rows), _ptr(ws), _ptr(sampled), B, Hg, Wg, pred.shape[2], pred.shape[3],
                                       float(min_depth), float(max_depth), y1, y2, x1, x2, int(scale_output), int(bool(use_gt_scale)),
                                       int(bool(pred_is_inverse)), _stream(gt)), "depth_metrics")
    return metrics, rows, ws, sampled


# ---------------------------------------------------------------------------------- depth output
VIZ_MAX_PIXELS = 1 << 24


def viz_inv_depth_check(B, H, W, N, percentile):
    """The argument rules of pnsfm_viz_inv_depth that do not need a tensor (the library refuses the same with an error code)."""
    if B < 1 or H < 1 or W < 1:
        raise RuntimeError("viz_inv_depth: empty tensor [%d,1,%d,%d]" % (B, H, W))
    if H * W > VIZ_MAX_PIXELS:
        raise RuntimeError("viz_inv_depth: %d x %d pixels are above 2^24 (the fp32 sample count must be exact)" % (H, W))
    if not 1 <= N <= 256:
        raise RuntimeError("viz_inv_depth: colour table of %d rows (1..256)" % N)
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError("Percentiles must be in the range [0, 100]")


def viz_inv_depth(inv, rgb, lut8, percentile, filter_zeros, normalizer, bgr, want_index=False):
    """inv [B,1,H,W], rgb [B,3,H,W] | None (fp32 or fp16 each), lut8 uint8 [N,3] on inv's device; normalizer: float | None.
    -> (out uint8 [B,H,W,3] or [B,2H,W,3] with the frame on top, index uint8 [B,H,W] | None, ws int32 words whose first B words are
    the fp32 normalisers), all on inv's device; nothing is copied to the host."""
    _chk(inv, rgb, lut8); _f32_or_h16(inv); _b1hw(inv, "viz_inv_depth: inv_depth")
    B, _, H, W = inv.shape
    if lut8.dtype != torch.uint8 or lut8.dim() != 2 or lut8.shape[1] != 3:
        raise RuntimeError("viz_inv_depth: the colour table must be uint8 [N,3], got %s %s" % (lut8.dtype, tuple(lut8.shape)))
    viz_inv_depth_check(B, H, W, lut8.shape[0], percentile)
    if rgb is not None:
        _f32_or_h16(rgb)
        if tuple(rgb.shape) != (B, 3, H, W):
            raise RuntimeError("viz_inv_depth: rgb %s does not match inv_depth %s" % (tuple(rgb.shape), tuple(inv.shape)))
    lib = _lib.get()
    out = torch.empty((B, 2 * H if rgb is not None else H, W, 3), dtype=torch.uint8, device=inv.device)
    index = torch.empty((B, H, W), dtype=torch.uint8, device=inv.device) if want_index else None
    ws = torch.empty((int(lib.pnsfm_viz_inv_depth_ws_bytes(B)) // 8,), dtype=torch.float64, device=inv.device).view(torch.int32)
    _lib.check(lib.pnsfm_viz_inv_depth(_ptr(inv), int(inv.dtype == torch.float16), _ptr(rgb), int(rgb is not None and rgb.dtype == torch.float16),
                                       _ptr(lut8), lut8.shape[0], _ptr(out), _ptr(index), _ptr(ws), B, H, W, float(percentile),
                                       int(bool(filter_zeros)), int(normalizer is not None), float(normalizer or 0.0), int(bool(bgr)),
                                       _stream(inv)), "viz_inv_depth")
    return out, index, ws


def depth_png16(inv):
    """inv: fp32 or fp16, any shape -> uint16 of the same shape: min(trunc((1 / max(inv, 1e-6)) * 256), 65535) (one launch)."""
    _chk(inv); _f32_or_h16(inv)
    if inv.numel() == 0:
        raise RuntimeError("depth_png16: empty tensor")
    out = torch.empty(inv.shape, dtype=torch.uint16, device=inv.device)
    _lib.check(_lib.get().pnsfm_depth_png16(_ptr(inv), int(inv.dtype == torch.float16), _ptr(out), inv.numel(), _stream(inv)), "depth_png16")
    return out


# ------------------------------------------------------------------------------------------------ NRS
def nrs_project_forward(direction, ray, temperature):
    """direction, ray: [3,h,w] -> (coords [h,w,2] = expected (row, col), stat [h,w,2] for backward)."""
    _chk(direction, ray); _f32(direction, ray)
    _, h, w = direction.shape
    coords = torch.empty((h, w, 2), dtype=torch.float32, device=ray.device)
    stat = torch.empty((h, w, 2), dtype=torch.float32, device=ray.device)
    _lib.check(_lib.get().pnsfm_nrs_project_forward(_ptr(direction), _ptr(ray), _ptr(coords), _ptr(stat), h, w, float(temperature),
                                                    _stream(ray)), "nrs_project_forward")
    return coords, stat


def nrs_project_backward(direction, ray, coords, stat, gcoords, temperature, want_dir=True, want_ray=True):
    _chk(direction, ray, coords, stat, gcoords); _f32(direction, ray, coords, stat, gcoords)
    _, h, w = direction.shape
    gdir = torch.empty_like(direction) if want_dir else None
    gray = torch.empty_like(ray) if want_ray else None
    _lib.check(_lib.get().pnsfm_nrs_project_backward(_ptr(direction), _ptr(ray), _ptr(coords), _ptr(stat), _ptr(gcoords), _ptr(gdir),
                                                     _ptr(gray), h, w, float(temperature), _stream(ray)), "nrs_project_backward")
    return gdir, gray


# ------------------------------------------------------------------------------------- input pipeline
def resample8(img, kk, bounds, out_size, axis):
    """One axis of PIL's 8-bit separable resample.  img: uint8 [N,H,W,C] (NHWC); kk int32 [out, ksize]; bounds int32 [out, 2]."""
    _chk(img, kk, bounds)
    if img.dtype != torch.uint8 or kk.dtype != torch.int32 or bounds.dtype != torch.int32:
        raise RuntimeError("resample8: uint8 image, int32 coefficient tables expected")
    N, H, W, C = img.shape
    oH, oW = (H, out_size) if axis == 1 else (out_size, W)
    out = torch.empty((N, oH, oW, C), dtype=torch.uint8, device=img.device)
    _lib.check(_lib.get().pnsfm_resample8(_ptr(img), _ptr(out), _ptr(kk), _ptr(bounds), kk.shape[1], N, H, W, oH, oW, C, axis,
                                          _stream(img)), "resample8")
    return out


# struct JitterOps of csrc/augment.hip: 4 op codes, 4 blend factors, hue_add, enabled, 3 'color' matrix diagonal entries, has_color
JITTER_RECORD = '4i4f2i3fi'
JITTER_RECORD_BYTES = 56


def jitter_record(order=(-1, -1, -1, -1), factors=(1.0, 1.0, 1.0, 1.0), hue_add=0, enabled=0, color=None):
    import struct
    c = tuple(float(v) for v in color) if color is not None else (1.0, 1.0, 1.0)
    return struct.pack(JITTER_RECORD, *order, *[float(f) for f in factors], int(hue_add), int(enabled), *c, 1 if color is not None else 0)


def jitter_totensor(img, ops_records, want_original=True):
    """img: uint8 [N,H,W,3]; ops_records: uint8 tensor holding N packed 56-byte JitterOps records (JITTER_RECORD) -> (jittered, original) float32
    [N,3,H,W] (original is None unless requested)."""
    _chk(img, ops_records)
    N, H, W, C = img.shape
    if img.dtype != torch.uint8 or C != 3 or ops_records.dtype != torch.uint8 or ops_records.numel() != JITTER_RECORD_BYTES * N:
        raise RuntimeError("jitter_totensor: uint8 [N,H,W,3] image and N %d-byte operation records expected" % JITTER_RECORD_BYTES)
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=img.device)
    orig = torch.empty((N, 3, H, W), dtype=torch.float32, device=img.device) if want_original else None
    ws = torch.empty((N,), dtype=torch.int64, device=img.device)
    _lib.check(_lib.get().pnsfm_jitter_totensor(_ptr(img), _ptr(ops_records), _ptr(ws), _ptr(out), _ptr(orig), N, H, W, _stream(img)),
               "jitter_totensor")
    return out, orig


def _depth_window(depth, window, what):
    """depth: fp32 [N,h,w] or [N,1,h,w], contiguous -> (N, row stride, image stride, (y0, x0, h, w)) with the window inside the map."""
    _chk(depth); _f32(depth)
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3 or depth.numel() == 0:
        raise RuntimeError("%s: depth maps must be a non-empty [N,h,w] or [N,1,h,w], got %s" % (what, tuple(depth.shape)))
    N, h0, w0 = depth.shape
    y0, x0, h, w = (0, 0, h0, w0) if window is None else (int(v) for v in window)
    if not (0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= h0 and x0 + w <= w0):
        raise RuntimeError("%s: window (y0 %d, x0 %d, h %d, w %d) leaves the %dx%d map" % (what, y0, x0, h, w, h0, w0))
    return N, w0, h0 * w0, (y0, x0, h, w)


def depth_resize_preserve(depth, shape, window=None):
    """resize_depth_preserve (reference datasets/augmentations.py:56-98) of N maps.  depth: fp32 [N,h,w] or [N,1,h,w]; window = (y0, x0,
    h, w): the crop_depth window, read in place; shape = (H, W) -> fp32 [N,1,H,W]."""
    N, row_stride, img_stride, (y0, x0, h, w) = _depth_window(depth, window, "depth_resize_preserve")
    H, W = int(shape[0]), int(shape[1])
    out = torch.empty((N, 1, H, W), dtype=torch.float32, device=depth.device)
    _lib.check(_lib.get().pnsfm_depth_resize_preserve(_ptr(depth), img_stride, row_stride, N, y0, x0, h, w, _ptr(out), H, W, H / h, W / w,
                                                      _stream(depth)), "depth_resize_preserve")
    return out


def depth_resize_nearest(depth, shape, window=None):
    """resize_depth (cv2.resize INTER_NEAREST, augmentations.py:35-53) of N maps, by the rule stated in include/pnsfm.h (not pinned
    against OpenCV itself).  Arguments and result as depth_resize_preserve."""
    N, row_stride, img_stride, (y0, x0, h, w) = _depth_window(depth, window, "depth_resize_nearest")
    H, W = int(shape[0]), int(shape[1])
    out = torch.empty((N, 1, H, W), dtype=torch.float32, device=depth.device)
    _lib.check(_lib.get().pnsfm_depth_resize_nearest(_ptr(depth), img_stride, row_stride, N, y0, x0, h, w, _ptr(out), H, W,
                                                     1.0 / (float(H) / h), 1.0 / (float(W) / w), _stream(depth)), "depth_resize_nearest")
    return out


def totensor8(img, dtype=torch.float32):
    """ToTensor without jitter.  img: uint8 [N,H,W,3] -> [N,3,H,W] float32 (bit-identical to jitter_totensor's original) or float16 (that
    value rounded once)."""
    _chk(img)
    if img.dim() != 4 or img.dtype != torch.uint8 or img.shape[3] != 3 or img.numel() == 0:
        raise RuntimeError("totensor8: non-empty uint8 [N,H,W,3] image expected")
    if dtype not in (torch.float32, torch.float16):
        raise RuntimeError("totensor8: float32 or float16 output, got %s" % dtype)
    N, H, W, _ = img.shape
    out = torch.empty((N, 3, H, W), dtype=dtype, device=img.device)
    _lib.check(_lib.get().pnsfm_totensor8(_ptr(img), _ptr(out), int(dtype == torch.float16), N, H, W, _stream(img)), "totensor8")
    return out


# -------------------------------------------------------------------------------------- sparse tensors (PackNet-SAN)
def _i32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.int32:
            raise RuntimeError("packnet_sfm HIP op needs int32 index tensors, got %s" % t.dtype)


def sparse_compact(src, cap=None):
    """src: fp32 tensor over the cells of a [B, h, w] grid (a depth map or a 0/1 mask); active = src > 0.
    -> (imap int32 [ncell], sites int32 [cap or ncell], count int32 [1] on the device).  cap=None sizes `sites` for every cell (the
    caller trims it once it knows the count); otherwise rows past `cap` are dropped."""
    _chk(src); _f32(src)
    ncell = src.numel()
    dev = src.device
    imap = torch.empty((ncell,), dtype=torch.int32, device=dev)
    sites = torch.empty((ncell if cap is None else max(cap, 1),), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((int(_lib.get().pnsfm_sparse_compact_ws_ints(ncell)),), dtype=torch.int32, device=dev)
    _lib.check(_lib.get().pnsfm_sparse_compact(_ptr(src), ncell, _ptr(imap), _ptr(sites), sites.numel() if cap is None else cap,
                                               _ptr(count), _ptr(ws), _stream(src)), "sparse_compact")
    return imap, sites, count


def sparse_pool_cells(imap, B, h, w):
    _chk(imap); _i32(imap)
    mask = torch.empty((B * ((h + 1) // 2) * ((w + 1) // 2),), dtype=torch.float32, device=imap.device)     # odd grids: ceil
    _lib.check(_lib.get().pnsfm_sparse_pool_cells(_ptr(imap), B, h, w, _ptr(mask), _stream(imap)), "sparse_pool_cells")
    return mask


def sparse_neighbors(imap, sites, count, cap, h, w, ks):
    _chk(imap, sites, count); _i32(imap, sites, count)
    nbr = torch.empty((max(cap, 1), ks * ks), dtype=torch.int32, device=imap.device)
    _lib.check(_lib.get().pnsfm_sparse_neighbors(_ptr(imap), _ptr(sites), _ptr(count), cap, h, w, ks, _ptr(nbr), _stream(imap)),
               "sparse_neighbors")
    return nbr


def sparse_conv(feats, kern, nbr, count, ks, flip=False):
    """feats [cap, Cin], kern [ks*ks, Cin, Cout] -> [cap, Cout] (rows past count are zero)."""
    _chk(feats, kern, nbr, count); _f32(feats, kern); _i32(nbr, count)
    cap, Cin = feats.shape
    KK, Cin2, Cout = kern.shape
    if KK != ks * ks or Cin2 != Cin:
        raise RuntimeError("sparse_conv: kernel %s does not match %d input channels / k=%d" % (tuple(kern.shape), Cin, ks))
    out = torch.empty((cap, Cout), dtype=torch.float32, device=feats.device)
    _lib.check(_lib.get().pnsfm_sparse_conv(_ptr(feats), _ptr(kern), _ptr(nbr), _ptr(count), _ptr(out), cap, Cin, Cout, ks,
                                            1 if flip else 0, _stream(feats)), "sparse_conv")
    return out


def sparse_conv_backward_weight(feats, dout, nbr, count, ks):
    _chk(feats, dout, nbr, count); _f32(feats, dout); _i32(nbr, count)
    cap, Cin = feats.shape
    Cout = dout.shape[1]
    dk = torch.empty((ks * ks, Cin, Cout), dtype=torch.float32, device=feats.device)
    _lib.check(_lib.get().pnsfm_sparse_conv_backward_weight(_ptr(feats), _ptr(dout), _ptr(nbr), _ptr(count), _ptr(dk), cap, Cin, Cout,
                                                            ks, _stream(feats)), "sparse_conv_backward_weight")
    return dk


def sparse_maxpool_forward(fin, imap_in, sites_out, count_out, cap_out, h, w):
    _chk(fin, imap_in, sites_out, count_out); _f32(fin); _i32(imap_in, sites_out, count_out)
    C = fin.shape[1]
    fout = torch.empty((cap_out, C), dtype=torch.float32, device=fin.device)
    arg = torch.empty((cap_out, C), dtype=torch.int32, device=fin.device)
    _lib.check(_lib.get().pnsfm_sparse_maxpool_forward(_ptr(fin), _ptr(imap_in), _ptr(sites_out), _ptr(count_out), _ptr(fout), _ptr(arg),
                                                       cap_out, C, h, w, _stream(fin)), "sparse_maxpool_forward")
    return fout, arg


def sparse_maxpool_backward(dout, arg, cap_in):
    _chk(dout, arg); _f32(dout); _i32(arg)
    cap_out, C = dout.shape
    din = torch.empty((cap_in, C), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.get().pnsfm_sparse_maxpool_backward(_ptr(dout), _ptr(arg), _ptr(din), cap_out, cap_in, C, _stream(dout)),
               "sparse_maxpool_backward")
    return din


def sparse_densify(feats, imap, B, hw):
    _chk(feats, imap); _f32(feats); _i32(imap)
    C = feats.shape[1]
    dense = torch.empty((B, C, hw), dtype=torch.float32, device=feats.device)
    _lib.check(_lib.get().pnsfm_sparse_densify(_ptr(feats), _ptr(imap), _ptr(dense), B, C, hw, _stream(feats)), "sparse_densify")
    return dense


def sparse_gather(dense, sites, count, cap):
    """dense [B, C, hw] -> rows [cap, C] at the active sites (zeros past count)."""
    _chk(dense, sites, count); _f32(dense); _i32(sites, count)
    B, C, hw = dense.shape
    rows = torch.empty((cap, C), dtype=torch.float32, device=dense.device)
    _lib.check(_lib.get().pnsfm_sparse_gather(_ptr(dense), _ptr(sites), _ptr(count), _ptr(rows), cap, C, hw, _stream(dense)),
               "sparse_gather")
    return rows


# ---------------------------------------------------------------------------------------------- adam
def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, grad_scale, step):
    _chk(param, grad, exp_avg, exp_avg_sq); _f32(param, grad, exp_avg, exp_avg_sq)
    _lib.check(_lib.get().pnsfm_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(lr),
                                          float(beta1), float(beta2), float(eps), float(weight_decay), float(grad_scale),
                                          int(step), _stream(param)), "adam_step")


def adam_flat_step(param, grad, exp_avg, exp_avg_sq, hp):
    """Adam on flat fp32 buffers with device-resident state hp = float[12]: [step, lr, beta1, beta2, eps, weight_decay, grad_scale, 1-beta1, 1-beta2, ...]."""
    _chk(param, grad, exp_avg, exp_avg_sq, hp); _f32(param, grad, exp_avg, exp_avg_sq, hp)
    _lib.check(_lib.get().pnsfm_adam_flat_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(hp),
                                               _stream(param)), "adam_flat_step")


def adam_fused_plan(conv_items, segments, device):
    """Device tables of the two-launch optimizer tail (include/pnsfm.h: pnsfm_adam_pack_table / pnsfm_adam_segments).
    conv_items: [(w, g, m, v, hp, wp_fwd, wp_bwd)] with w a [Cout, Cin, k, k] VIEW into the parameter arena and g, m, v the same slices
    of the other arenas; segments: [(p, g, m, v, hp)] flat slices.  Returns (item table, n items, blocks, indices of the conv items the
    table took, segment table, n segments, blocks); conv items it did not take must be added to `segments` by the caller."""
    lib = _lib.get()
    isz = int(lib.pnsfm_adam_pack_item_bytes())
    host = (ctypes.c_ubyte * (isz * max(1, len(conv_items))))()
    n, blocks, covered = 0, 0, []
    for i, (w, g, m, v, hp, pf, pb) in enumerate(conv_items):
        _chk(w, g, m, v, hp, pf, pb); _f32(w, g, m, v, hp, pf, pb)
        Cout, Cin, ks, _ = w.shape
        rc = lib.pnsfm_adam_pack_item_fill(ctypes.addressof(host) + n * isz, _ptr(w), _ptr(g), _ptr(m), _ptr(v), _ptr(hp), _ptr(pf), _ptr(pb),
                                           Cin, Cout, ks, blocks)
        if rc < 0:
            _lib.check(rc, "adam_pack_item_fill")
        if rc > 0:
            n += 1
            blocks += rc
            covered.append(i)
    table = torch.frombuffer(bytearray(bytes(host)[:max(1, n) * isz]), dtype=torch.uint8).to(device)
    return table, n, blocks, covered


def adam_segment_table(segments, device):
    lib = _lib.get()
    ssz = int(lib.pnsfm_adam_seg_bytes())
    host = (ctypes.c_ubyte * (ssz * max(1, len(segments))))()
    blocks = 0
    for i, (p, g, m, v, hp) in enumerate(segments):
        _chk(p, g, m, v, hp); _f32(p, g, m, v, hp)
        rc = lib.pnsfm_adam_seg_fill(ctypes.addressof(host) + i * ssz, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(hp), p.numel(), blocks)
        if rc < 0:
            _lib.check(rc, "adam_seg_fill")
        blocks += rc
    table = torch.frombuffer(bytearray(bytes(host)[:max(1, len(segments)) * ssz]), dtype=torch.uint8).to(device)
    return table, len(segments), blocks


def adam_pack_table_run(table, n, blocks):
    if n:
        _lib.check(_lib.get().pnsfm_adam_pack_table(_ptr(table), n, blocks, _stream(table)), "adam_pack_table")


def adam_segments_run(table, n, blocks):
    if n:
        _lib.check(_lib.get().pnsfm_adam_segments(_ptr(table), n, blocks, _stream(table)), "adam_segments")


def adam_flat_update(param, grad, exp_avg, exp_avg_sq, hp, tick):
    """adam_flat_step on a slice of the arenas; tick: advance the group's step counter first (one slice per group and step)."""
    _chk(param, grad, exp_avg, exp_avg_sq, hp); _f32(param, grad, exp_avg, exp_avg_sq, hp)
    _lib.check(_lib.get().pnsfm_adam_flat_update(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(hp),
                                                 1 if tick else 0, _stream(param)), "adam_flat_update")


# ------------------------------------------------------------------------------- batched region ops
class _RegionOp(ctypes.Structure):          # mirrors pnsfm_region_op (include/pnsfm.h)
    _fields_ = [('src', ctypes.c_void_p), ('dst', ctypes.c_void_p), ('n', ctypes.c_int * 4), ('src_stride', ctypes.c_longlong * 4),
                ('dst_stride', ctypes.c_longlong * 4), ('op', ctypes.c_int)]


REGION_COPY, REGION_ADD, REGION_ZERO = 0, 1, 2
MAX_REGION_OPS = 12


def region_ops(items):
    """items: list of (op, dst_view, src_view | None).  Views are <= 4-D windows (any strides) of fp32 tensors on one device; shapes of
    dst and src must match.  ONE kernel launch per MAX_REGION_OPS items (csrc/elementwise.hip: region_ops_kernel)."""
    if not items:
        return
    ref = items[0][1]
    from . import _seq
    sq = _seq.get()
    if sq is not None:
        sq.region_ops([(int(op), dst, src) for op, dst, src in items], launch_stream_raw(ref.device))
        return
    for i0 in range(0, len(items), MAX_REGION_OPS):
        chunk = items[i0:i0 + MAX_REGION_OPS]
        arr = (_RegionOp * len(chunk))()
        for k, (op, dst, src) in enumerate(chunk):
            if dst.dtype != torch.float32 or (src is not None and src.dtype != torch.float32):
                raise RuntimeError("region_ops needs float32 tensors")
            if _lib.REQUIRE_CUDA and not dst.is_cuda:
                raise RuntimeError("packnet_sfm HIP op got a %s tensor: the HIP kernels run on MI355X only, there is no CPU fallback" % dst.device)
            if dst.dim() > 4 or (src is not None and tuple(src.shape) != tuple(dst.shape)) or dst.device != ref.device:
                raise RuntimeError("region_ops: windows must be <= 4-D, of equal shape, on one device")
            pad = 4 - dst.dim()
            shape = (1,) * pad + tuple(dst.shape)
            if 0 in shape:
                raise RuntimeError("region_ops: empty window")
            arr[k].dst = dst.data_ptr()
            arr[k].src = src.data_ptr() if src is not None else None
            arr[k].op = int(op)
            for d in range(4):
                arr[k].n[d] = shape[d]
                arr[k].dst_stride[d] = 0 if d < pad else dst.stride(d - pad)
                arr[k].src_stride[d] = 0 if (src is None or d < pad) else src.stride(d - pad)
        _lib.check(_lib.get().pnsfm_region_ops(ctypes.byref(arr), len(chunk), _stream(ref)), "region_ops")



# ------------------------------------------------------------------------- fp16 forward (evaluation / inference)
# include/pnsfm.h "fp16 forward": fp16 storage, fp32 arithmetic, one round-to-nearest-even per kernel output.  Forward only.
def _h16(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float16:
            raise RuntimeError("packnet_sfm fp16 HIP op needs float16 tensors, got %s" % t.dtype)


def conv2d_pack_h16(w, out=None):
    """w [Cout, Cin, k, k] fp16 (a plain layer) or fp32 (the composed weight of a collapsed packing layer) -> packed fp16 operand image
    of the fp16 forward kernel."""
    _chk(w, out)
    if w.dtype not in (torch.float16, torch.float32):
        raise RuntimeError("conv2d_pack_h16: weight must be float16 or float32, got %s" % w.dtype)
    Cout, Cin, ks, _ = w.shape
    n = int(_lib.get().pnsfm_conv2d_packed_elems_h16(Cin, Cout, ks))
    if out is None or out.numel() != n or out.device != w.device:
        out = torch.empty(n, dtype=torch.float16, device=w.device)
    _h16(out)
    _lib.check(_lib.get().pnsfm_conv2d_pack_weights_h16(_ptr(w), 1 if w.dtype == torch.float32 else 0, _ptr(out), Cin, Cout, ks,
                                                         _stream(w)), "conv2d_pack_weights_h16")
    return out


def conv2d_forward_h16(xs, wp, bias, Cout, ks):
    """xs: 1..3 fp16 NCHW tensors (their channel concatenation is the input); wp from conv2d_pack_h16; bias fp32 [Cout] or None."""
    xs = tuple(xs)
    if not 1 <= len(xs) <= 3:
        raise RuntimeError("conv2d_forward_h16: 1 to 3 input tensors")
    _chk(*xs, wp, bias); _h16(*xs, wp); _f32(bias)
    B, _, H, W = xs[0].shape
    for t in xs[1:]:
        if t.shape[0] != B or tuple(t.shape[2:]) != (H, W):
            raise RuntimeError("conv2d_forward_h16: inputs of different batch / spatial sizes")
    C = [t.shape[1] for t in xs] + [0] * (3 - len(xs))
    P = [xs[i] if i < len(xs) else None for i in range(3)]
    y = torch.empty((B, Cout, H, W), dtype=torch.float16, device=xs[0].device)
    rc = _lib.get().pnsfm_conv2d_forward_h16(_ptr(P[0]), C[0], _ptr(P[1]), C[1], _ptr(P[2]), C[2], _ptr(wp), _ptr(bias), _ptr(y), B,
                                             Cout, H, W, ks, _stream(xs[0]))
    _lib.check(rc, "conv2d_forward_h16")
    return y


def groupnorm_act_forward_h16(x, res, gamma, beta, G, eps, act):
    _chk(x, res, gamma, beta); _h16(x, res, gamma, beta)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    ms = torch.empty((2, B * G), dtype=torch.float32, device=x.device)
    rc = _lib.get().pnsfm_groupnorm_act_forward_h16(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(ms[0]), _ptr(ms[1]), B, C,
                                                    HW, G, float(eps), act, _stream(x))
    _lib.check(rc, "groupnorm_act_forward_h16")
    return y


def conv3d_forward_h16(p, w3, b3):
    _chk(p, w3, b3); _h16(p, w3, b3)
    B, D, H, W = p.shape
    nf = _nf_of(w3)
    out = torch.empty((B, nf * D, H, W), dtype=torch.float16, device=p.device)
    _lib.check(_lib.get().pnsfm_conv3d_forward_h16(_ptr(p), _ptr(w3), _ptr(b3), _ptr(out), B, D, H, W, nf, _stream(p)), "conv3d_forward_h16")
    return out


def space_to_depth_h16(x):
    x = x.contiguous()
    _chk(x); _h16(x)
    B, C, H, W = x.shape
    y = torch.empty((B, 4 * C, H // 2, W // 2), dtype=torch.float16, device=x.device)
    _lib.check(_lib.get().pnsfm_space_to_depth_h16(_ptr(x), _ptr(y), B, C, H, W, _stream(x)), "space_to_depth_h16")
    return y


def depth_to_space_h16(x):
    _chk(x); _h16(x)
    B, C4, H, W = x.shape
    assert C4 % 4 == 0
    y = torch.empty((B, C4 // 4, 2 * H, 2 * W), dtype=torch.float16, device=x.device)
    _lib.check(_lib.get().pnsfm_depth_to_space_h16(_ptr(x), _ptr(y), B, C4 // 4, H, W, _stream(x)), "depth_to_space_h16")
    return y


def upsample_nearest_forward_h16(x, s):
    _chk(x); _h16(x)
    B, C, h, w = x.shape
    y = torch.empty((B, C, h * s, w * s), dtype=torch.float16, device=x.device)
    _lib.check(_lib.get().pnsfm_upsample_nearest_forward_h16(_ptr(x), _ptr(y), B * C, h, w, s, _stream(x)), "upsample_nearest_forward_h16")
    return y


def invdepth_conv_forward_h16(x, w, bias, min_depth):
    _chk(x, w, bias); _h16(x, w, bias)
    B, C, H, W = x.shape
    if tuple(w.shape) != (1, C, 3, 3) or bias is None or bias.numel() != 1:
        raise RuntimeError("invdepth_conv: weight must be [1,%d,3,3] with a bias of one element" % C)
    y = torch.empty((B, 1, H, W), dtype=torch.float16, device=x.device)
    _lib.check(_lib.get().pnsfm_invdepth_conv_forward_h16(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, C, H, W, float(min_depth), _stream(x)),
               "invdepth_conv_forward_h16")
    return y


def region_ops_h16(items):
    """region_ops on fp16 windows (one launch per MAX_REGION_OPS items)."""
    if not items:
        return
    ref = items[0][1]
    for i0 in range(0, len(items), MAX_REGION_OPS):
        chunk = items[i0:i0 + MAX_REGION_OPS]
        arr = (_RegionOp * len(chunk))()
        for k, (op, dst, src) in enumerate(chunk):
            _h16(dst, src)
            if _lib.REQUIRE_CUDA and not dst.is_cuda:
                raise RuntimeError("packnet_sfm HIP op got a %s tensor: the HIP kernels run on MI355X only, there is no CPU fallback" % dst.device)
            if dst.dim() > 4 or (src is not None and tuple(src.shape) != tuple(dst.shape)) or dst.device != ref.device:
                raise RuntimeError("region_ops: windows must be <= 4-D, of equal shape, on one device")
            pad = 4 - dst.dim()
            shape = (1,) * pad + tuple(dst.shape)
            if 0 in shape:
                raise RuntimeError("region_ops: empty window")
            arr[k].dst = dst.data_ptr()
            arr[k].src = src.data_ptr() if src is not None else None
            arr[k].op = int(op)
            for d in range(4):
                arr[k].n[d] = shape[d]
                arr[k].dst_stride[d] = 0 if d < pad else dst.stride(d - pad)
                arr[k].src_stride[d] = 0 if (src is None or d < pad) else src.stride(d - pad)
        _lib.check(_lib.get().pnsfm_region_ops_h16(ctypes.byref(arr), len(chunk), _stream(ref)), "region_ops_h16")


# ---- fp16 forward: ResNet networks (include/pnsfm.h) ------------------------------------------------------------------------------
class _ConvH16G(ctypes.Structure):          # mirrors pnsfm_conv_h16g (include/pnsfm.h)
    _fields_ = [('x', ctypes.c_void_p * 3), ('C', ctypes.c_int * 3), ('up', ctypes.c_int * 3), ('wp', ctypes.c_void_p),
                ('scale', ctypes.c_void_p), ('shift', ctypes.c_void_p), ('res', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('B', ctypes.c_int), ('Cout', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int), ('ks', ctypes.c_int),
                ('stride', ctypes.c_int), ('pad_reflect', ctypes.c_int), ('act', ctypes.c_int), ('p0', ctypes.c_float),
                ('p1', ctypes.c_float), ('pre', ctypes.c_int), ('pre_a', ctypes.c_float), ('pre_b', ctypes.c_float)]


def conv2d_h16g_out_shape(xs, ups, Cout, ks, stride):
    B = xs[0].shape[0]
    H, W = xs[0].shape[2] * ups[0], xs[0].shape[3] * ups[0]
    R = ks // 2
    return B, Cout, (H + 2 * R - ks) // stride + 1, (W + 2 * R - ks) // stride + 1


def conv2d_forward_h16g(xs, wp, Cout, ks, stride=1, reflect=False, ups=None, scale=None, shift=None, res=None, act=ACT_NONE,
                        disp=(0.0, 1.0), pre_affine=None, out=None):
    """y = act(scale * conv(G(xs), w) + shift + res) in ONE launch (two with a K split): xs 1..3 fp16 NCHW tensors, source i up-sampled by
    ups[i] in {1, 2} onto the common H x W grid and concatenated along the channels; zero or reflect padding of ks // 2; stride 1 | 2;
    scale / shift fp32 [Cout] or None; res fp16 of the output's shape or None; pre_affine (a, b): in-bounds inputs become
    fp16(fma(x, a, b)).  out: a contiguous fp16 tensor of the output's shape to write into."""
    xs = tuple(xs)
    if not 1 <= len(xs) <= 3:
        raise RuntimeError("conv2d_forward_h16g: 1 to 3 input tensors")
    ups = (1,) * len(xs) if ups is None else tuple(int(u) for u in ups)
    if len(ups) != len(xs) or any(u not in (1, 2) for u in ups):
        raise ValueError("conv2d_forward_h16g: one up-sampling factor (1 | 2) per source, got %s for %d sources" % (ups, len(xs)))
    _chk(*xs, wp, scale, shift, res, out); _h16(*xs, wp, res, out); _f32(scale, shift)
    shape = conv2d_h16g_out_shape(xs, ups, Cout, ks, stride)
    B, H, W = xs[0].shape[0], xs[0].shape[2] * ups[0], xs[0].shape[3] * ups[0]
    for t, u in zip(xs, ups):
        if t.dim() != 4 or t.shape[0] != B or (t.shape[2] * u, t.shape[3] * u) != (H, W):
            raise RuntimeError("conv2d_forward_h16g: inputs of different batch / (up-sampled) spatial sizes")
    if reflect and (H < 2 or W < 2 or H <= ks // 2 or W <= ks // 2):
        raise ValueError("conv2d_forward_h16g: reflection padding needs an input larger than the pad (and at least 2 x 2), got %d x %d"
                         % (H, W))
    for v, n in ((scale, 'scale'), (shift, 'shift')):
        if v is not None and v.numel() != Cout:
            raise RuntimeError("conv2d_forward_h16g: %s must have %d elements" % (n, Cout))
    if res is not None and tuple(res.shape) != shape:
        raise RuntimeError("conv2d_forward_h16g: residual of shape %s, output %s" % (tuple(res.shape), shape))
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=xs[0].device)
    elif tuple(out.shape) != shape:
        raise RuntimeError("conv2d_forward_h16g: out of shape %s, output %s" % (tuple(out.shape), shape))
    d = _ConvH16G()
    for i, (t, u) in enumerate(zip(xs, ups)):
        d.x[i], d.C[i], d.up[i] = t.data_ptr(), t.shape[1], u - 1
    d.wp, d.y = wp.data_ptr(), out.data_ptr()
    d.scale = None if scale is None else scale.data_ptr()
    d.shift = None if shift is None else shift.data_ptr()
    d.res = None if res is None else res.data_ptr()
    d.B, d.Cout, d.H, d.W, d.ks, d.stride, d.pad_reflect, d.act = B, Cout, H, W, ks, stride, 1 if reflect else 0, int(act)
    d.p0, d.p1 = float(disp[0]), float(disp[1])
    if pre_affine is not None:
        d.pre, d.pre_a, d.pre_b = 1, float(pre_affine[0]), float(pre_affine[1])
    _lib.check(_lib.get().pnsfm_conv2d_forward_h16g(ctypes.byref(d), _stream(xs[0])), "conv2d_forward_h16g")
    return out


def bn_fold_h16(gamma, beta, running_mean, running_var, eps, out=None):
    """fp16 [C] x 4 -> fp32 [2, C]: scale = gamma / sqrt(var + eps) | shift = beta - mean * scale, computed in fp64."""
    _chk(gamma, beta, running_mean, running_var, out); _h16(gamma, beta, running_mean, running_var); _f32(out)
    C = gamma.numel()
    if any(t.numel() != C for t in (beta, running_mean, running_var)):
        raise RuntimeError("bn_fold_h16: the four tensors must have one length")
    if out is None:
        out = torch.empty((2, C), dtype=torch.float32, device=gamma.device)
    elif tuple(out.shape) != (2, C):
        raise RuntimeError("bn_fold_h16: out must be [2, %d]" % C)
    _lib.check(_lib.get().pnsfm_bn_fold_h16(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), float(eps), _ptr(out), C,
                                            _stream(gamma)), "bn_fold_h16")
    return out


def maxpool3x3s2_forward_h16(x, out=None):
    """x [..., H, W] fp16 -> y [..., Ho, Wo] fp16 (no arg-max plane: forward only)."""
    _chk(x, out); _h16(x, out)
    N, H, W = _planes(x, "maxpool3x3s2")
    shape = tuple(x.shape[:-2]) + ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=x.device)
    elif tuple(out.shape) != shape:
        raise RuntimeError("maxpool3x3s2_forward_h16: out of shape %s, output %s" % (tuple(out.shape), shape))
    _lib.check(_lib.get().pnsfm_maxpool3x3s2_forward_h16(_ptr(x), _ptr(out), N, H, W, _stream(x)), "maxpool3x3s2_forward_h16")
    return out


def conv2d_last_config():
    out = (ctypes.c_int * 8)()
    _lib.get().pnsfm_conv2d_last_config(out)
    return list(out)


# ---------------------------------------------------------------------------------------------- prof
def calib_mfma(sink, blocks, iters):
    """The bare six-product bf16 MFMA stream (csrc/calib.hip); returns the bf16 flops of the launch."""
    _chk(sink); _f32(sink)
    assert sink.numel() >= blocks * 256
    _lib.check(_lib.get().pnsfm_calib_mfma(_ptr(sink), blocks, iters, _stream(sink)), "calib_mfma")
    return blocks * 4.0 * iters * 24.0 * (2.0 * 32 * 32 * 16)


def calib_copy(src, dst):
    _chk(src, dst); _f32(src, dst)
    assert src.numel() == dst.numel()
    _lib.check(_lib.get().pnsfm_calib_copy(_ptr(src), _ptr(dst), src.numel(), _stream(src)), "calib_copy")
    return 2.0 * 4.0 * src.numel()


def prof_enable(on):
    _lib.get().pnsfm_prof_enable(1 if on else 0)


def prof_reset():
    _lib.get().pnsfm_prof_reset()


def prof_collect(kind):
    ms, fl, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_longlong(0)
    _lib.get().pnsfm_prof_collect(kind, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n))
    return ms.value, fl.value, n.value


def prof_dump(path):
    _lib.check(_lib.get().pnsfm_prof_dump(path.encode()), "prof_dump")
