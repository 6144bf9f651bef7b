"""Cases of the all-scales entry points of csrc/loss.hip (include/pnsfm.h "all scales in one launch"), shared by the emulated CPU
tests (tests/test_loss_ms_emulated.py) and the GPU tests (tests/test_gpu_loss_ms.py).

The reference of every comparison is the per-scale path (HF.set_loss_ms(False): one set of launches per scale, the autograd engine
summing the gradients), and every comparison is torch.equal: the per-pixel fp64 pins of tests/loss_cases.py hold the per-scale
kernels, bit equality carries them over, no tolerance is introduced here.

Shapes (B, H, W): (1, 3, 3) both reflect multipliers on one pixel; (1, 16, 16) exactly one tile; (2, 17, 33) the tile edge crossed in
both directions with a live sample index; (1, 2, 258) the block edge of the 256-pixel kernels.  The photometric kernels refuse H < 3
(per scale and all scales alike), so (1, 2, 258) runs the node's 256-pixel kernels -- view synthesis and smoothness, forward and
backward -- against their per-scale calls, and (1, 3, 258) is ADDED for the whole node across that block edge.

The identity map.  The per-scale photometric kernel has two outputs, the selection byte per pixel and the pixel sum, so "its
unwarped candidates per pixel" are observed through exactly those: with warped := ref every candidate of the per-scale kernel is an
identity value, and (a) under 'mean' with one context the kernel's scalar is the pixel sum of the identity values, accumulated in
float64, where the sum of these float32 values is exact in any order (asserted), so it equals the float64 sum of the map bit for bit
only if the multiset of values agrees; (b) under 'min' with two contexts the selection byte of every pixel must be the argmin
of the map's two values; (c) the all-scales kernel reading the map must reproduce the per-scale kernel's scalar and bytes when the
warped candidates are real (the node comparison above, automask cases)."""
import ctypes
import functools
import os
import sys

import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for _p in (_ROOT, os.path.join(_ROOT, 'packnet-sfm_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loss_cases as LC  # noqa: E402

SSIM_W, C1, C2 = LC.SSIM_W, LC.C1, LC.C2
SMOOTH_W = 0.1
NODE_SHAPES = [(1, 3, 3), (1, 16, 16), (2, 17, 33), (1, 3, 258)]
THIN_SHAPE = (1, 2, 258)
NS, JS = (1, 4), (1, 2)
VARIANTS = (('min', True), ('min', False), ('mean', False))       # (reduce op, automask)


def _sid(shape):
    return 'x'.join(str(s) for s in shape)


NODE_CASES = [dict(id='ms-%s-n%d-J%d-%s%s-%s' % (_sid(s), n, J, r, '-auto' if a else '', m), shape=s, n=n, J=J, red=r, auto=a, mode=m)
              for s in NODE_SHAPES for n in NS for J in JS for r, a in VARIANTS for m in LC.PADDING]
THIN_CASES = [dict(id='ms-%s-n%d-J%d-%s' % (_sid(THIN_SHAPE), n, J, m), shape=THIN_SHAPE, n=n, J=J, mode=m)
              for n in NS for J in JS for m in LC.PADDING]
ID_CASES = [dict(id='id-%s-J%d' % (_sid(s), J), shape=s, J=J) for s in NODE_SHAPES for J in JS]
MIXED = ((8, 12), (4, 6), (2, 3), (2, 2))


def ids(cases):
    return [c['id'] for c in cases]


@functools.lru_cache(maxsize=None)
def inputs(shape, J, n):
    """float32 CPU inputs: n DIFFERENT inverse-depth maps [B,1,H,W], ref [J,B,3,H,W], target [B,3,H,W], K, refK [B,3,3], T [J,B,4,4]
    (loss_cases.vs_inputs with a 'medium' pose: samples leave the frame on every side)."""
    B, H, W = shape
    rho, ref, K, refK, T = LC.vs_inputs((B, J, H, W), 'medium')
    g = torch.Generator().manual_seed(LC._key(shape, J, n, 77))
    invs = tuple((rho * (0.75 + 0.5 * torch.rand(rho.shape, generator=g))).contiguous() for _ in range(n))
    for a in range(n):
        for b in range(a):
            assert not torch.equal(invs[a], invs[b])
    target = torch.rand(B, 3, H, W, generator=g)
    return invs, ref, target, K, refK, T


def _reduce(red):
    from packnet_sfm.hip import functional as HF
    return HF.REDUCE_MIN if red == 'min' else HF.REDUCE_MEAN


def _node_run(device, case, ms):
    """(photometric scalars, smoothness scalars, d_inv of every scale, dT) of one path, all on the CPU"""
    from packnet_sfm.hip import functional as HF
    invs, ref, target, K, refK, T = inputs(case['shape'], case['J'], case['n'])
    invs = [d.to(device).clone().requires_grad_(True) for d in invs]      # (a copy: .to() of a CPU tensor is the cached tensor itself)
    ref, target, K, refK = LC._to(device, ref, target, K, refK)
    T = T.to(device).clone().requires_grad_(True)
    prev = HF.set_loss_ms(ms)
    try:
        terms = HF.multiview_loss_terms(invs, ref, target, K, refK, T, SSIM_W, C1, C2, case['auto'], _reduce(case['red']), 0.0,
                                        case['mode'])
        assert HF.loss_ms_used() == ms
        if ms:
            photo, smooth = terms
        else:
            assert terms is None
            photo = [HF.warp_photometric(d, ref, target, K, refK, T, SSIM_W, C1, C2, case['auto'], _reduce(case['red']), 0.0, case['mode'])
                     for d in invs]
            smooth = [HF.smoothness_norm(d, target) for d in invs]
        loss, _s, _p = HF.loss_combine(photo, smooth, SMOOTH_W)
        loss.backward()
    finally:
        HF.set_loss_ms(prev)
    LC._sync(device)
    cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
    return cpu(photo), cpu(smooth), cpu([d.grad for d in invs]), T.grad.cpu().clone(), loss.detach().cpu().clone()


def run_node(device, case):
    """The all-scales node against the per-scale path: every scalar, every d_inv, dT and the combined loss, torch.equal."""
    got, want = _node_run(device, case, True), _node_run(device, case, False)
    for i in range(case['n']):
        assert torch.equal(got[0][i], want[0][i]), ('photometric', i, got[0][i], want[0][i])
        assert torch.equal(got[1][i], want[1][i]), ('smoothness', i, got[1][i], want[1][i])
        assert torch.equal(got[2][i], want[2][i]), ('d_inv', i, (got[2][i] - want[2][i]).abs().max())
        assert float(want[2][i].abs().max()) > 0.0
    assert torch.equal(got[3], want[3]), ('dT', (got[3] - want[3]).abs().max())
    B, H, W = case['shape']      # (on nine pixels the unwarped candidates can win everywhere: a zero pose gradient on both sides)
    assert B * H * W < LC.SMALL or float(want[3].abs().max()) > 0.0
    assert torch.equal(got[4], want[4])


def run_thin(device, case):
    """H = 2: the 256-pixel kernels of the node (view synthesis, smoothness) at their block edge, all scales against per scale."""
    from packnet_sfm.hip import ops
    n, J = case['n'], case['J']
    invs, ref, target, K, refK, T = inputs(case['shape'], J, n)
    invs = list(LC._to(device, *invs))
    ref, target, K, refK, T = LC._to(device, ref, target, K, refK, T)
    mode = ops.PADDING_MODES[case['mode']]
    warped = ops.view_synthesis_forward_ms(invs, ref, K, refK, T, mode)
    g = torch.Generator().manual_seed(LC._key(case['shape'], J, n, 5))
    d_warped = (torch.rand(warped.shape, generator=g) - 0.5).to(device)
    d_inv, dT = ops.view_synthesis_backward_ms(d_warped, invs, ref, K, refK, T, mode)
    up = [torch.rand(1, generator=g).to(device) for _ in range(n)]
    loss, mean = ops.smoothness_norm_forward_ms(invs, [target] * n)
    d_sm = ops.smoothness_norm_backward_ms(invs, [target] * n, mean, up)
    dT_want = None
    # dT: the finish kernel adds the scales as ((dT[n-1] + dT[n-2]) + ...) + dT[0], the association torch's autograd engine produces
    # today for per-scale nodes (the node created last runs first).  That order is torch's, not the kernels': if an upgrade of torch
    # changes it, this comparison and run_node's dT break by an ulp without the kernel being wrong -- adjust the kernel's order then.
    for i in reversed(range(n)):
        assert torch.equal(warped[i], ops.view_synthesis_forward(invs[i], ref, K, refK, T, mode))
        di, dTi = ops.view_synthesis_backward(d_warped[i].contiguous(), invs[i], ref, K, refK, T, mode)
        assert torch.equal(d_inv[i], di)
        dT_want = dTi if dT_want is None else dT_want + dTi
        li, mi = ops.smoothness_norm_forward(invs[i], target)
        assert torch.equal(loss[i:i + 1], li) and torch.equal(mean[i], mi)
        assert torch.equal(d_sm[i], ops.smoothness_norm_backward(invs[i], target, mi, up[i]))
    assert torch.equal(dT, dT_want)
    LC._sync(device)


def run_identity(device, case):
    """pnsfm_photometric_identity_forward against the unwarped candidates of the per-scale kernel (module docstring)."""
    from packnet_sfm.hip import functional as HF, ops
    B, H, W = case['shape']
    J = case['J']
    _invs, ref, target, _K, _rK, _T = inputs(case['shape'], J, 1)
    ref, target = LC._to(device, ref, target)
    idmap = ops.photometric_identity_forward(ref, target, SSIM_W, C1, C2)
    assert tuple(idmap.shape) == (J, B, H, W)
    idc = idmap.cpu()
    assert bool(torch.isfinite(idc).all()) and float(idc.min()) >= 0.0 and float(idc.max()) <= 1.0 and float(idc.max()) > 0.0
    # (a) 'mean', one context at a time, warped := ref: the scalar is the exact pixel sum of the map
    for j in range(J):
        loss, _ = ops.photometric_forward(ref[j:j + 1].contiguous(), ref[j:j + 1].contiguous(), target, SSIM_W, C1, C2, False, HF.REDUCE_MEAN)
        v = idc[j].double().flatten()
        total = v.sum()
        assert float(total) == float(v.flip(0).sum()) == float(v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(1))].sum()), \
            'the float64 sum of the map is not exact: the comparison below would depend on the order'
        want = (total * (1.0 / float(B * H * W))).float()
        assert torch.equal(loss.cpu().reshape(()), want), (j, loss, want)
    # (b) 'min' without automask over J contexts, warped := ref: the byte is the first smallest identity value of the pixel
    _loss, argmin = ops.photometric_forward(ref, ref, target, SSIM_W, C1, C2, False, HF.REDUCE_MIN)
    assert torch.equal(argmin.cpu().long(), idc.argmin(0))
    # ... and with automask every pair (warped_j, ref_j) ties: candidates 0, 2, ... compete with the same values, first smallest wins
    _loss, argmin = ops.photometric_forward(ref, ref, target, SSIM_W, C1, C2, True, HF.REDUCE_MIN)
    assert torch.equal(argmin.cpu().long(), 2 * idc.argmin(0))
    # (c) the all-scales kernel reading the map, warped := ref: scalar and bytes of the per-scale kernel
    loss_ps, arg_ps = ops.photometric_forward(ref, ref, target, SSIM_W, C1, C2, True, HF.REDUCE_MIN)
    loss_ms, arg_ms = ops.photometric_forward_ms(ref.unsqueeze(0).contiguous(), idmap, target, SSIM_W, C1, C2, True, HF.REDUCE_MIN)
    assert torch.equal(loss_ms.cpu(), loss_ps.cpu()) and torch.equal(arg_ms[0].cpu(), arg_ps.cpu())
    LC._sync(device)


@functools.lru_cache(maxsize=None)
def mixed_inputs(B=2):
    g = torch.Generator().manual_seed(LC._key(B, 4242))
    invs = tuple((0.05 + 0.95 * torch.rand(B, 1, h, w, generator=g)) for h, w in MIXED)
    images = tuple(torch.rand(B, 3, h, w, generator=g) for h, w in MIXED)
    ups = tuple(torch.rand(1, generator=g) + 0.5 for _ in MIXED)
    others = tuple(torch.rand(B, 1, h, w, generator=g) - 0.5 for h, w in MIXED)
    return invs, images, ups, others


def run_smoothness_mixed(device):
    """pnsfm_smoothness_norm_*_ms on four resolutions in one launch against four per-scale calls; the accumulate flag against a + b."""
    from packnet_sfm.hip import ops
    invs, images, ups, others = (list(LC._to(device, *ts)) for ts in mixed_inputs())
    n = len(invs)
    loss, mean = ops.smoothness_norm_forward_ms(invs, images)
    d = ops.smoothness_norm_backward_ms(invs, images, mean, ups)
    d1 = ops.smoothness_norm_backward_ms(invs, images, mean, None)
    acc = [o.clone() for o in others]
    out = ops.smoothness_norm_backward_ms(invs, images, mean, ups, acc)
    for i in range(n):
        li, mi = ops.smoothness_norm_forward(invs[i], images[i])
        assert torch.equal(loss[i:i + 1], li) and torch.equal(mean[i], mi), i
        di = ops.smoothness_norm_backward(invs[i], images[i], mi, ups[i])
        assert torch.equal(d[i], di), i
        assert torch.equal(d1[i], ops.smoothness_norm_backward(invs[i], images[i], mi, None)), i
        assert out[i] is acc[i] and torch.equal(acc[i], others[i] + di), i
        assert float(di.abs().max()) > 0.0
    LC._sync(device)


def _loss_module(device, inv_shapes, B, H, W, switch, **kw):
    """loss, d_inv of every scale and the pose gradient of MultiViewPhotometricLoss on seeded inputs, all on the CPU"""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.losses.multiview_photometric_loss import MultiViewPhotometricLoss
    _i, ref, target, K, refK, T = inputs((B, H, W), 2, 1)
    g = torch.Generator().manual_seed(LC._key(B, H, W, len(inv_shapes), 9))
    invs = [(0.05 + 0.4 * torch.rand(B, 1, h, w, generator=g)).to(device).requires_grad_(True) for h, w in inv_shapes]
    ref, target, K, refK = LC._to(device, ref, target, K, refK)
    T = T.to(device).clone().requires_grad_(True)
    module = MultiViewPhotometricLoss(num_scales=len(inv_shapes), **kw)
    prev = HF.set_loss_ms(switch)
    try:
        out = module(target, [ref[0], ref[1]], invs, K, K, [T[0], T[1]])
        used = HF.loss_ms_used()
        out['loss'].sum().backward()
    finally:
        HF.set_loss_ms(prev)
    LC._sync(device)
    return used, [out['loss'].detach().cpu()] + [d.grad.cpu() for d in invs] + [T.grad.cpu()]


def run_fallback(device):
    """Where the node does not apply the module runs the per-scale path and says so; where it applies, both paths agree bit for bit."""
    B, H, W = 1, 16, 24
    full = [(H, W)] * 3
    cfgs = [(dict(clip_loss=0.0, photometric_reduce_op='min', automask_loss=True), [(16, 24), (8, 12), (4, 6)]),      # mixed resolutions
            (dict(clip_loss=0.5, photometric_reduce_op='min', automask_loss=True), full),                              # clipping
            (dict(clip_loss=0.0, ssim_loss_weight=0.0, photometric_reduce_op='min'), full)]                            # the L1-only kernels
    for kw, shapes in cfgs:
        used_on, got = _loss_module(device, shapes, B, H, W, True, **kw)
        used_off, want = _loss_module(device, shapes, B, H, W, False, **kw)
        assert not used_on and not used_off, kw
        assert all(torch.equal(a, b) for a, b in zip(got, want)), kw
    for kw in (dict(clip_loss=0.0, photometric_reduce_op='min', automask_loss=True), dict(clip_loss=0.0, smooth_loss_weight=0.0),
               dict(clip_loss=0.0, ssim_loss_weight=0.0, photometric_reduce_op='mean')):
        used_on, got = _loss_module(device, full, B, H, W, True, **kw)
        used_off, want = _loss_module(device, full, B, H, W, False, **kw)
        assert used_on and not used_off, kw
        assert all(torch.equal(a, b) for a, b in zip(got, want)), kw


def run_rejects(device):
    """n < 1, n above the table size, a null table entry and H < 2: -1 with an error text and no launch (outputs keep their fill)."""
    from packnet_sfm.hip import _lib, ops
    lib = _lib.get()
    P, S = ops._ptr, ops._stream
    f = lambda *s: torch.rand(*s).to(device)
    nan = lambda *s: torch.full(s, float('nan'), device=device)
    B, J, H, W, NMAX = 1, 1, 4, 4, 8
    inv, ref, target, K, T = f(B, 1, H, W), f(J, B, 3, H, W), f(B, 3, H, W), f(B, 3, 3), f(J, B, 4, 4)
    warped, d, dT, loss, mean = nan(NMAX + 1, J, B, 3, H, W), nan(B, 1, H, W), nan(J, B, 4, 4), nan(NMAX + 1), nan(NMAX + 1, B)
    argmin = torch.full((NMAX + 1, B, H, W), 0xAA, dtype=torch.uint8, device=device)
    idmap = nan(J, B, H, W)

    def table(ts, n):
        return ctypes.byref((ctypes.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in ts]))

    def ints(v, n):
        return ctypes.byref((ctypes.c_int * max(n, 1))(*([v] * max(n, 1))))

    def calls(n, invs, h, w):
        ti, td, tim = table(invs, n), table([d] * max(n, 1), n), table([target] * max(n, 1), n)
        yield lib.pnsfm_view_synthesis_forward_ms(ti, n, P(ref), P(K), P(K), P(T), P(warped), J, B, h, w, 0, S(ref))
        yield lib.pnsfm_view_synthesis_backward_ms(P(warped), ti, n, P(ref), P(K), P(K), P(T), td, P(dT), J, B, h, w, 0, S(ref))
        yield lib.pnsfm_smoothness_norm_forward_ms(ti, tim, ints(h, n), ints(w, n), n, P(loss), P(mean), B, S(ref))
        yield lib.pnsfm_smoothness_norm_backward_ms(ti, tim, ints(h, n), ints(w, n), n, P(inv), None, td, 0, B, S(ref))

    for n, invs, h, w, text in ((0, [inv], H, W, b'n must be'), (NMAX + 1, [inv] * (NMAX + 1), H, W, b'n must be'),
                                (2, [inv, None], H, W, b'is null'), (1, [inv], 1, W, b'bad shape'), (1, [inv], H, 1, b'bad shape')):
        for rc in calls(n, invs, h, w):
            assert rc == -1 and text in lib.pnsfm_last_error(), (n, h, w, rc, lib.pnsfm_last_error())
    # the photometric entry points take no pointer table but n, and H, W >= 3 as their per-scale forms
    for n, h, w, text in ((0, H, W, b'n must be'), (NMAX + 1, H, W, b'n must be'), (1, 2, W, b'bad shape'), (1, H, 2, b'bad shape')):
        assert lib.pnsfm_photometric_forward_ms(P(warped), P(idmap), P(target), P(loss), P(argmin), n, J, B, h, w, SSIM_W, C1, C2, 1, 0,
                                                S(ref)) == -1 and text in lib.pnsfm_last_error()
        assert lib.pnsfm_photometric_backward_ms(P(warped), P(target), P(argmin), P(warped), 1.0, None, n, J, B, h, w, SSIM_W, C1, C2, 1, 0,
                                                 S(ref)) == -1 and text in lib.pnsfm_last_error()
    assert lib.pnsfm_photometric_identity_forward(P(ref), P(target), P(idmap), J, B, 2, W, SSIM_W, C1, C2, S(ref)) == -1
    assert b'bad shape' in lib.pnsfm_last_error()
    assert lib.pnsfm_photometric_forward_ms(P(warped), None, P(target), P(loss), P(argmin), 1, J, B, H, W, SSIM_W, C1, C2, 1, 0, S(ref)) == -1
    assert b'identity map' in lib.pnsfm_last_error()
    LC._sync(device)
    assert all(bool(torch.isnan(t).all()) for t in (warped, d, dT, loss, mean, idmap)) and bool((argmin == 0xAA).all())
