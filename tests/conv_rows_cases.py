"""Cases of the row-window convolution (include/pnsfm.h "Row windows": pnsfm_conv2d_forward_rows / _backward_data_rows /
_backward_weight_rows) shared by tests/test_conv_rows_emulated.py (host-emulated kernels) and tests/test_conv_rows_gpu.py (gfx950).

Reference, stock torch on the host with autograd for the gradients: the batched strips x [2B, Cin, 2r, w] hold in their leading half
the strips whose frame rows are the first r (zero above) and in their trailing half those whose frame rows are the last r (zero below):
    top    = F.conv2d(F.pad(x[:B], (r, r, r, 0)), w, b)
    bottom = F.conv2d(F.pad(x[B:], (r, r, 0, r)), w, b)
Every case PINS the launch configuration (packnet_sfm.hip.tune, key_rows) and asserts through pnsfm_conv2d_last_config that the
pinned kernel is what ran; every case runs twice and the two results must be torch.equal.

Shapes (the smallest at which the window can go wrong): r in {1, 2} (k = 3, 5); B in {1, 2} (the half boundary is at b = B, not at 1);
Cin in {40, 96} (a ragged 16-channel chunk; a K split > 1); Cout = 40 (a ragged 32-row tile); w in {33, 45, 130} (tiles that straddle
rows, a ragged last tile, more than one tile per row).  None of these widths is a multiple of 4, which the split-bf16 and nine-taps
weight-gradient kernels need, so those two run at w in {24, 36, 40, 64} as well (3-group tiles, masked 4-pixel halves, 16- and
32-column tiles)."""
import torch
import torch.nn.functional as F

import parity_cases as P

# (r, B, Cin, w): every value with every r, and the pairs that interact (B = 2 with both r, Cin = 96 with both r, w = 130 with both r);
# the full product would repeat them on the host emulator at a minute per case
SHAPES = [(1, 1, 40, 33), (1, 2, 96, 45), (1, 2, 40, 130), (1, 1, 96, 130), (2, 1, 40, 45), (2, 2, 40, 33), (2, 1, 96, 33), (2, 1, 40, 130)]
COUT = 40


def data(r, B, Cin, w, Cout=COUT, seed=0):
    ks = 2 * r + 1
    g = torch.Generator().manual_seed(1000 * r + 100 * B + Cin + w + seed)
    x = torch.randn(2 * B, Cin, 2 * r, w, generator=g)
    wt = torch.randn(Cout, Cin, ks, ks, generator=g) * (2.0 / (Cin * ks * ks)) ** 0.5
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(2 * B, Cout, r, w, generator=g)
    return x, wt, b, dy


_REF = {}


def reference(r, B, Cin, w, Cout=COUT):
    """(y, dx, dw, db) of the reference formula; computed once per shape and shared."""
    k = (r, B, Cin, w, Cout)
    if k not in _REF:
        x, wt, b, dy = data(r, B, Cin, w, Cout)
        xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        top = F.conv2d(F.pad(xr[:B], (r, r, r, 0)), wr, br)
        bottom = F.conv2d(F.pad(xr[B:], (r, r, 0, r)), wr, br)
        y = torch.cat((top, bottom), 0)
        y.backward(dy)
        _REF[k] = (y.detach(), xr.grad, wr.grad, br.grad)
    return _REF[k]


def keys(r, B, Cin, w, Cout=COUT):
    from packnet_sfm.hip import tune
    ks = 2 * r + 1
    return (tune.key_rows(tune.FORWARD, 2 * B, Cin, Cout, r, 2 * r, w, ks),
            tune.key_rows(tune.BACKWARD_DATA, 2 * B, Cout, Cin, 2 * r, r, w, ks),
            tune.key_rows(tune.WGRAD, 2 * B, Cin, Cout, r, 2 * r, w, ks))


def run(dev, shape, fwd=None, bwd=None, wg=None, Cout=COUT):
    """The three launches of one shape under the pinned decisions (None: that launch is skipped), twice.  Returns
    {'y' | 'dx' | 'dw' | 'db': tensor, 'cfg_*': LastConfig}."""
    from packnet_sfm.hip import ops, tune
    r, B, Cin, w = shape
    ks = 2 * r + 1
    x, wt, b, dy = (t.to(dev) for t in data(r, B, Cin, w, Cout))
    wf, wb = ops.conv2d_pack(wt)
    kf, kb, kw = keys(r, B, Cin, w, Cout)
    pins = [(k, d) for k, d in ((kf, fwd), (kb, bwd), (kw, wg)) if d is not None]
    out = {}
    with tune.pinned(*pins):
        for rep in range(2):
            got = {}
            if fwd is not None:
                got['y'] = ops.conv2d_forward_rows(x, wf, b, Cout, ks, r)
                out['cfg_fwd'] = tune.last_config()
            if bwd is not None:
                got['dx'] = ops.conv2d_backward_data_rows(dy, wb, Cin, ks, r)
                out['cfg_bwd'] = tune.last_config()
            if wg is not None:
                got['dw'], got['db'] = ops.conv2d_backward_weight_rows(x, dy, ks, r)
                out['cfg_wg'] = tune.last_config()
            for n, t in got.items():
                if rep:
                    assert torch.equal(t, out[n]), 'two runs of %s differ' % n
                out[n] = t
    return out


def check(out, shape, tol_data, tol_w, Cout=COUT):
    """Prints each figure before asserting it."""
    yr, dxr, dwr, dbr = reference(*shape, Cout=Cout)
    errs = {n: P.err(out[n], ref) for n, ref in (('y', yr), ('dx', dxr), ('dw', dwr), ('db', dbr)) if n in out}
    print('rows', shape, ' '.join('%s %.2e' % kv for kv in errs.items()))
    for n, e in errs.items():
        tol = tol_w if n in ('dw', 'db') else tol_data
        assert e <= tol, '%s %s: relative error %.3e > %.1e' % (n, shape, e, tol)


# ---- test bodies -------------------------------------------------------------------------------------------------------------------
def shape_case(dev, shape, tol_data, tol_w):
    """Every shape on the split-bf16 forward / backward-data kernel (variant 3) and the generic weight gradient; Cin = 96 with a
    K split of 2 in both directions and a pixel split of 2."""
    from packnet_sfm.hip import tune
    r, B, Cin, w = shape
    split = 2 if Cin == 96 else 1
    out = run(dev, shape, tune.ConvDecision(1, 3, split=split), tune.ConvDecision(1, 3, split=split), tune.WgradDecision(0, split))
    assert out['cfg_fwd']['variant'] == 3 and out['cfg_fwd']['split'] == split, out['cfg_fwd']
    assert out['cfg_bwd']['variant'] == 3 and out['cfg_bwd']['split'] == split, out['cfg_bwd']
    assert out['cfg_wg']['variant'] == 100 and out['cfg_wg']['split'] == split, out['cfg_wg']
    check(out, shape, tol_data, tol_w)


# (shape, (variant, NT, narrow M tile, tile mode, K split)): every split-bf16 kernel build a row-window launch can take -- the LDS
# plans 3..6 and the ping-pong workgroup 7, each un-split and with a K split (Cin = Cout = 40: three 16-channel chunks in both
# directions, the last one ragged).  Tile modes: the 16-wide rectangles never fit a map of <= 4 rows (conv_geom_fixed wants 60 % of
# the tile's slots filled), the row bands fit r = 2 at w = 45 in both directions -- pinned there.  The short-map rectangles (tile mode 3: all rows of a map of
# < 4 rows) are what the strips' launches are for: w = 96 fits them in both directions at r = 1, w = 130 the forward of r = 2 (two rows
# x 64 columns, a ragged third tile) and the backward-data of r = 1; a third element names the one launch of a case that takes the mode.
_A, _B = (1, 2, 40, 45), (2, 1, 40, 45)
BX3_VARIANTS = [(_A, c) for c in ((3, 1, 0, 0, 1), (3, 2, 0, 0, 3), (4, 2, 0, 0, 1), (4, 1, 1, 0, 2), (5, 1, 0, 0, 1), (5, 2, 0, 0, 2),
                                  (6, 1, 0, 0, 1), (6, 1, 1, 0, 3), (7, 2, 0, 0, 1), (7, 1, 0, 0, 2))] + \
               [(_B, c) for c in ((3, 1, 0, 2, 1), (4, 1, 0, 2, 2), (5, 1, 0, 2, 1), (6, 1, 0, 2, 1), (7, 1, 0, 2, 3), (7, 2, 0, 0, 1),
                                  (3, 2, 0, 0, 2))] + \
               [((1, 2, 40, 96), (3, 1, 0, 3, 1)), ((1, 2, 40, 96), (7, 1, 0, 3, 2)), ((2, 1, 40, 130), (4, 1, 0, 3, 3), 'fwd'),
                ((1, 1, 40, 130), (6, 1, 0, 3, 1), 'bwd')]


def bx3_variant_case(dev, case, tol_data):
    from packnet_sfm.hip import tune
    shape, cfg = case[:2]
    which = case[2] if len(case) > 2 else 'both'
    variant, NT, narrow, tm, split = cfg
    dec = tune.ConvDecision(NT, variant, narrow, tm, split)
    out = run(dev, shape, dec if which != 'bwd' else None, dec if which != 'fwd' else None, None)
    for n in ('cfg_fwd', 'cfg_bwd'):
        c = out.get(n)
        assert c is None or (c['variant'] == variant and c['NT'] == NT and c['tm'] == tm and c['split'] == split), (n, c)
    check(out, shape, tol_data, None)


# (shape, (variant, NT, K split)) of the f32 kernels
F32_VARIANTS = [(s, c) for s in (_A, (2, 1, 40, 33)) for c in ((0, 1, 1), (0, 2, 2), (1, 1, 1), (1, 2, 2), (2, 1, 1), (2, 2, 2))]


def f32_variant_case(dev, case, tol_data):
    """The generic f32 kernels (register-staged, LDS-DMA, pipelined): what the launches run under the f32 arithmetic mode."""
    from packnet_sfm.hip import functional as HF, tune
    shape, cfg = case
    variant, NT, split = cfg
    prev = HF.get_conv_math()
    HF.set_conv_math('f32')
    try:
        dec = tune.ConvDecision(NT, variant, split=split)
        out = run(dev, shape, dec, dec, None)
    finally:
        HF.set_conv_math(prev)
    for c in (out['cfg_fwd'], out['cfg_bwd']):
        assert c['variant'] == variant and c['NT'] == NT and c['split'] == split, c
    check(out, shape, tol_data, None)


# weight-gradient kernels: (shape (r, B, Cin, w), Cout, decision fields, the build last_config must report)
#   generic (100): any width; split-bf16 (103, k = 3 | 5): w % 4 == 0 -- 16-column tiles (40), masked halves (36), 32-column tiles (64),
#   two ci tiles per wave, fewer co tiles per workgroup, the three-workgroups build; nine-taps (104, k = 3): tiles of 3 / 4 / 5 groups on the
#   full strip's grid, masked, one and two ci tiles per workgroup.  One multi-split case per kernel at least.
WGRAD_KERNEL_CASES = [
    ((1, 2, 96, 45), 40, dict(kernel=0, split=4), (100,)),
    ((2, 1, 40, 33), 40, dict(kernel=0, split=1), (100,)),
    ((1, 2, 96, 40), 40, dict(kernel=2, split=1, NT=1), (103, 3, 1)),
    ((1, 2, 40, 40), 40, dict(kernel=2, split=2, NT=2), (103, 3, 2)),
    ((1, 1, 40, 36), 40, dict(kernel=2, split=2, NT=1), (103, 3, 1)),
    ((1, 2, 40, 64), 40, dict(kernel=2, split=1, NT=1, wm=8), (103, 3, 1)),
    ((1, 1, 40, 64), 136, dict(kernel=2, split=4, NT=1), (103, 3, 1, 4)),
    ((2, 2, 40, 40), 40, dict(kernel=2, split=2, NT=1), (103, 5, 1)),
    ((2, 1, 40, 36), 40, dict(kernel=2, split=1, NT=1, wm=1), (103, 5, 1)),
    ((1, 2, 96, 40), 40, dict(kernel=3, split=1, WCI=2, TG=5, TR=4), (104, 2, 5, 4)),
    ((1, 2, 40, 40), 40, dict(kernel=3, split=3, WCI=1, TG=4, TR=4), (104, 1, 4, 4)),
    ((1, 1, 40, 24), 40, dict(kernel=3, split=2, WCI=2, TG=3, TR=4), (104, 2, 3, 4)),
    ((1, 2, 40, 36), 40, dict(kernel=3, split=1, WCI=1, TG=5, TR=4), (104, 1, 5, 4)),
    ((1, 2, 40, 64), 40, dict(kernel=3, split=2, WCI=2, TG=4, TR=4), (104, 2, 4, 4)),
]


def wgrad_kernel_case(dev, case, tol_w):
    from packnet_sfm.hip import tune
    shape, Cout, fields, build = case
    out = run(dev, shape, None, None, tune.WgradDecision(**fields), Cout=Cout)
    c = out['cfg_wg']
    assert c.build[:len(build)] == build, (c.build, build)
    assert c['split'] == fields['split'], c
    check(out, shape, None, tol_w, Cout=Cout)


def refusal_case(dev):
    """A row window asked of the kernels that have none -- the 1x1 kernels, the stem's forward and weight-gradient kernels -- is an
    error with a message (no launch), under both arithmetic modes."""
    import pytest
    from packnet_sfm.hip import _lib, functional as HF, ops
    prev = HF.get_conv_math()
    try:
        for math in ('bx3', 'f32'):
            HF.set_conv_math(math)
            for Cin, ks, w in ((64, 1, 32), (3, 5, 64)):
                r = max(1, ks // 2)
                x = torch.randn(2, Cin, 2 * r, w).to(dev)
                wt = torch.randn(16, Cin, ks, ks).to(dev)
                dy = torch.randn(2, 16, r, w).to(dev)
                wf, wb = ops.conv2d_pack(wt)
                with pytest.raises(_lib.HipError, match='row window'):
                    ops.conv2d_forward_rows(x, wf, None, 16, ks, r)
                if ks == 1 or math == 'bx3':      # (the stem has a weight-gradient kernel of its own under the split arithmetic only)
                    with pytest.raises(_lib.HipError, match='row window'):
                        ops.conv2d_backward_weight_rows(x, dy, ks, r)
                if ks == 1:
                    with pytest.raises(_lib.HipError, match='row window'):
                        ops.conv2d_backward_data_rows(dy, wb, Cin, ks, r)
    finally:
        HF.set_conv_math(prev)


# ---- block level: PackLayerConv3d with the frame-rows strips against the full-strip form (the class attribute strip_frame_rows)
BLOCK_CASES = [(k, hw) for k in (3, 5) for hw in ((2 * (k // 2) + 1, 2 * (k // 2) + 2), (3 * (k // 2) + 1, 24), (12, 40))]


def block_case(dev, k, hw, tol_data, tol_w):
    """Output of the collapsed convolution, dP and the four parameter gradients of the two forms.  The first two map sizes are smaller
    than two strips: leading and trailing strips overlap."""
    from packnet_sfm.networks.layers.packnet.layers01 import PackLayerConv3d
    h, w = hw
    torch.manual_seed(10 * k + h)
    blk = PackLayerConv3d(16, k, d=8).to(dev)
    blk.collapse = True
    P0 = torch.randn(1, 64, h, w)      # (one image: the strips' 512 input channels make the host emulator slow)
    g0 = torch.randn(1, 16, h, w)
    res = []
    for rows in (False, True):
        blk.strip_frame_rows = rows
        blk.zero_grad()
        x = P0.to(dev).requires_grad_(True)
        y = blk._conv_collapsed(x)
        y.backward(g0.to(dev))
        base = blk.conv.conv_base
        res.append((y.detach(), x.grad, base.weight.grad.clone(), base.bias.grad.clone(), blk.conv3d.weight.grad.clone(),
                    blk.conv3d.bias.grad.clone()))
    names = ('output', 'dP', 'dW2', 'db2', 'dW3', 'db3')
    errs = [P.err(a, b) for a, b in zip(res[1], res[0])]
    print('block k=%d %dx%d' % (k, h, w), ' '.join('%s %.2e' % ne for ne in zip(names, errs)))
    for n, e in zip(names, errs):
        tol = tol_data if n in ('output', 'dP') else tol_w
        assert e <= tol, '%s (k=%d, %dx%d): relative error %.3e > %.1e' % (n, k, h, w, e, tol)


def block_bits_case(dev, k, hw):
    """On the device, with the tuner on: the frame-rows form takes the K split, the weight-gradient kernel and the pixel split of the
    full strips it is cut from (whose decisions exist once the full-strip form has run), and the rows it no longer computes only ever
    added zeros -- so the block's output and every gradient are the full-strip form's bit for bit.  That holds for the split-bf16 and
    nine-taps weight-gradient kernels, whose k-steps keep their place on the full strip's grid (the generic and tap-major kernels tile
    the pixels of dY linearly): the full strips' weight gradients are pinned to them, as the shipped decisions of the training
    resolutions are (nine-taps for k = 3, split-bf16 for k = 5), and the row windows must follow the pins."""
    from packnet_sfm.hip import tune
    from packnet_sfm.networks.layers.packnet.layers01 import PackLayerConv3d
    h, w = hw
    r = k // 2
    dec = tune.WgradDecision(3, 2, WCI=2) if k == 3 else tune.WgradDecision(2, 2)
    pins = [(tune.key(tune.WGRAD, 4, 512, 16, 2 * r, ww, k), dec) for ww in (w, h)]
    torch.manual_seed(20 * k + h)
    blk = PackLayerConv3d(16, k, d=8).to(dev)
    blk.collapse = True
    P0 = torch.randn(2, 64, h, w)
    g0 = torch.randn(2, 16, h, w)
    res = []
    with tune.pinned(*pins):
        for rows in (False, True):
            blk.strip_frame_rows = rows
            blk.zero_grad()
            x = P0.to(dev).requires_grad_(True)
            y = blk._conv_collapsed(x)
            y.backward(g0.to(dev))
            base = blk.conv.conv_base
            res.append((y.detach(), x.grad, base.weight.grad.clone(), base.bias.grad.clone(), blk.conv3d.weight.grad.clone(),
                        blk.conv3d.bias.grad.clone()))
    for n, a, b in zip(('output', 'dP', 'dW2', 'db2', 'dW3', 'db3'), res[1], res[0]):
        assert torch.equal(a, b), '%s (k=%d, %dx%d): frame rows differ from the full strips by %.3e' % (n, k, h, w, P.err(a, b))
