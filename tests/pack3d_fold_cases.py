"""Cases of the folded launch sequences of the packing / unpacking blocks (csrc/pack3d.hip, csrc/elementwise.hip), shared by the
emulated CPU tests (tests/test_pack3d_fold_emulated.py) and the GPU tests (tests/test_gpu_pack3d_fold.py):

  forward     pnsfm_conv3d_forward_d2s        conv3d_fwd_x4_d2s_kernel: the Conv3d stencil stores the depth-to-space layout
  rows        pnsfm_conv3d_forward_rows / _backward_data_rows / _backward_weight_rows: the border strips' Conv3d on the 2r rows
              strip_select keeps (a row window in conv3d_fwd_x4_kernel and the gradient kernels)
  bias        pnsfm_pack_bias_eff_forward     pack_bias_ssum_kernel on a (d, C) grid + pack_bias_eff_tail_kernel

A fold moves no arithmetic: per output the folded kernels run the unfolded kernels' operations in their order.  So the reference
is the unfolded launch sequence of the same build (pnsfm_set_pack3d_fold(0)) and the comparison is torch.equal, no tolerance; the
unfolded sequence itself is pinned against float64 by tests/pack3d_cases.py.  Layout as there: every launch goes through the C ABI
into a NaN-filled slot inside a larger NaN-filled tensor (wgrad_cases._slot), inputs sit in such slots too (a case can put a tensor
1 - 3 floats off a 16-byte boundary, and a load that strays reads NaN); asserted in this order: return code 0, guards still NaN,
every element written, equality; for the gradients also that a second launch into a fresh slot is bit-identical.

Each forward case states whether the folded kernel or the fallback is meant to run (`fwd`: True = folded); check_table() restates
the launcher's conditions, and the runner compares the statement with pnsfm_conv3d_d2s_folded.

The stencil gradients reading the incoming gradient through the space-to-depth map were measured and left out, and
the reference-form pack4 / pack5 folds are not built; there are no cases for them."""
import torch
import torch.nn.functional as F

from wgrad_cases import _slot, _check_slot

NFS = (8, 4)


def _sid(shape):
    return 'x'.join(str(s) for s in shape)


# ------------------------------------------------------------------------------------------------ the table
# (B, D, H, W) of the Conv3d volume p; y is [B, NF*D/4, 2H, 2W].
VOLUME_SHAPES = [
    (1, 4, 1, 4), (2, 4, 3, 8), (1, 8, 5, 12), (3, 12, 2, 36),
    (1, 4, 2, 64),                                    # a row of 16 threads
    (1, 8, 16, 124),                                  # 4 x 16 x 31 = 1984 thread items: 8 blocks, ragged last
    (1, 8, 13, 252),                                  # 3276 items: 13 blocks
    (1, 8, 24, 260),                                  # 6240 items: 25 blocks
    (1, 4, 2, 62), (1, 4, 2, 63), (1, 4, 3, 6),       # W % 4 != 0: the two-kernel path
    (2, 6, 2, 8), (1, 5, 3, 4),                       # D % 4 != 0: the two-kernel path
]
GRIDS_WANTED = {1, 8, 13, 25}


def _vol_case(shape, nf, p_off=0, y_off=0):
    B, D, H, W = shape
    name = 'vol-%s-nf%d%s%s' % (_sid(shape), nf, '-p+%d' % p_off if p_off else '', '-y+%d' % y_off if y_off else '')
    return dict(id=name, shape=shape, nf=nf, p_off=p_off, y_off=y_off,
                fwd=(W % 4 == 0 and D % 4 == 0 and p_off % 4 == 0 and y_off % 4 == 0))       # slots are 16-byte aligned at offset 0


def _vol_cases():
    out = []
    for nf in NFS:
        out += [_vol_case(s, nf) for s in VOLUME_SHAPES]
        # a tensor 1 - 3 floats off a 16-byte boundary: the two-kernel path (the folded kernel stores float4)
        out.append(_vol_case((2, 4, 3, 8), nf, p_off=1))
        out.append(_vol_case((2, 4, 3, 8), nf, y_off=2))
        out.append(_vol_case((1, 8, 5, 12), nf, p_off=3, y_off=3))
    return out


FWD_CASES = _vol_cases()

# border strips [2B, D, S = 2r + 1, w]: the two halves of the batch keep different rows (0 .. 2r-1 / 1 .. 2r).  wt: the column strips'
# form, the Conv3d weights with their (y, x) taps transposed (W3.transpose(3, 4))
ROWS_CASES = [dict(id='rows-r%d-w%d-B%d-D%d-nf%d%s' % (r, w, B, D, nf, '-wt' if wt else ''), r=r, w=w, B=B, D=D, nf=nf, wt=wt)
              for nf in NFS for r in (1, 2) for w in (4, 8, 36, 64) for B, D, wt in ((1, 5, False), (2, 8, True))]

# (C, d, blk) of pnsfm_pack_bias_eff_forward: W2 is [C, d * blk]
BIAS_CASES = [dict(id='bias-%d-%d-%d%s' % (C, d, blk, '' if b2 else '-nob2'), C=C, d=d, blk=blk, b2=b2)
              for C, d, blk, b2 in ((3, 8, 7, True), (5, 4, 257, True), (64, 8, 800, True), (5, 4, 257, False))]

# whole blocks (GroupNorm(16) wants 16 channels): x [2, 16, 12, 16]
BLOCK_CASES = ['pack-collapsed-k3', 'pack-collapsed-k5', 'pack-reference-k3', 'unpack-k3']

assert len({c['id'] for c in FWD_CASES}) == len(FWD_CASES)


def ids(cases):
    return [c if isinstance(c, str) else c['id'] for c in cases]


def select(cases, **want):
    got = [c for c in cases if all(c[k] == v for k, v in want.items())]
    assert got, want
    return got


# ------------------------------------------------------------------------------------------------ the launchers' conditions, restated
def _ceil_div(a, b):
    return -(-a // b)


def fwd_grid(shape):
    B, D, H, W = shape
    return _ceil_div((D // 2) * H * (W // 4), 256)


def check_table():
    """What the table promises without running a kernel."""
    for c in FWD_CASES:
        B, D, H, W = c['shape']
        assert D * H * W <= 50000, c['id']
    for nf in NFS:
        cs = [c for c in FWD_CASES if c['nf'] == nf]
        assert {c['shape'] for c in cs} == set(VOLUME_SHAPES)
        assert {(1, 4, 1, 4), (2, 4, 3, 8), (1, 8, 5, 12), (3, 12, 2, 36)} <= {c['shape'] for c in cs if c['fwd']}
        # both outcomes of every condition of the fold
        assert any(not c['fwd'] and c['shape'][3] % 4 for c in cs) and any(not c['fwd'] and c['shape'][1] % 4 for c in cs)
        assert {1, 2, 3} <= {c['p_off'] % 4 for c in cs} | {c['y_off'] % 4 for c in cs}
        assert GRIDS_WANTED <= {fwd_grid(c['shape']) for c in cs if c['fwd']}
        assert any((c['shape'][1] // 2) * c['shape'][2] * (c['shape'][3] // 4) % 256 for c in cs if c['fwd'] and fwd_grid(c['shape']) > 1)
    assert {(c['r'], c['w'], c['B']) for c in ROWS_CASES} == {(r, w, B) for r in (1, 2) for w in (4, 8, 36, 64) for B in (1, 2)}
    assert any(c['wt'] for c in ROWS_CASES)
    assert {(c['C'], c['d'], c['blk']) for c in BIAS_CASES} == {(3, 8, 7), (5, 4, 257), (64, 8, 800)} and any(not c['b2'] for c in BIAS_CASES)


# ------------------------------------------------------------------------------------------------ the runners
def _lib_ops():
    from packnet_sfm.hip import _lib, ops
    return _lib.get(), ops


def _place(t, device, offset=0):
    _, s = _slot(t.shape, device, t.dtype, offset)
    s.copy_(t)
    return s


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


class _Fold(object):
    """`with _Fold(lib, 0):` -- the unfolded launch sequences; the previous setting comes back on exit."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, on

    def __enter__(self):
        self.prev = self.lib.pnsfm_set_pack3d_fold(self.on)

    def __exit__(self, *exc):
        self.lib.pnsfm_set_pack3d_fold(self.prev)


def _inputs(case):
    B, D, H, W = case['shape']
    nf = case['nf']
    g = torch.Generator().manual_seed(16 * sum(case['shape']) + 97 * W + nf)
    p = torch.randn(B, D, H, W, generator=g)
    w3 = 0.3 * torch.randn(nf, 1, 3, 3, 3, generator=g)
    b3 = torch.randn(nf, generator=g)
    return p, w3, b3


def run_forward(device, case):
    """pnsfm_conv3d_forward_d2s folded (or its fallback, as the case says) against the unfolded sequence of the same build, and that
    against torch's pixel_shuffle of pnsfm_conv3d_forward."""
    lib, ops = _lib_ops()
    B, D, H, W = case['shape']
    nf = case['nf']
    pc, w3c, b3c = _inputs(case)
    p, w3, b3 = _place(pc, device, case['p_off']), _place(w3c, device), _place(b3c, device)
    yshape = (B, nf * D // 4, 2 * H, 2 * W)

    def launch(with_tmp):
        whole, y = _slot(yshape, device, offset=case['y_off'])
        wt, tmp = _slot((B, nf * D, H, W), device) if with_tmp else (None, None)
        rc = lib.pnsfm_conv3d_forward_d2s(ops._ptr(p), ops._ptr(w3), ops._ptr(b3), ops._ptr(tmp), ops._ptr(y), B, D, H, W, nf, ops._stream(y))
        _sync(device)
        assert rc == 0, (rc, lib.pnsfm_last_error())
        _check_slot(whole, y, case['id'])
        return y, tmp, wt

    with _Fold(lib, 0):
        assert lib.pnsfm_conv3d_d2s_folded(ops._ptr(p), ops._ptr(_slot(yshape, device, offset=case['y_off'])[1]), D, W) == 0
        ref, tmp, wt = launch(True)
        _check_slot(wt, tmp, case['id'] + ' tmp')
        assert torch.equal(ref.cpu(), F.pixel_shuffle(tmp.cpu(), 2)), case['id']
    with _Fold(lib, 1):
        assert lib.pnsfm_conv3d_d2s_folded(ops._ptr(p), ops._ptr(_slot(yshape, device, offset=case['y_off'])[1]), D, W) == int(case['fwd'])
        got, tmp, wt = launch(not case['fwd'])
    assert torch.equal(got, ref), '%s: %d of %d elements differ from the unfolded sequence' % (case['id'], int((got != ref).sum()), got.numel())


def run_rows(device, case):
    """The three *_rows entry points against the full-frame sequence: pnsfm_conv3d_forward and the row selection; the zero-filled
    gradient, pnsfm_conv3d_backward_data (all S rows of dp, the un-kept row's included) and pnsfm_conv3d_backward_weight."""
    lib, ops = _lib_ops()
    r, w, B, D, nf = case['r'], case['w'], case['B'], case['D'], case['nf']
    S, n2, B2 = 2 * r + 1, 2 * r, 2 * B
    g = torch.Generator().manual_seed(1000 * r + 10 * w + B + nf)
    w3c = 0.3 * torch.randn(nf, 1, 3, 3, 3, generator=g)
    if case['wt']:
        w3c = w3c.transpose(3, 4).contiguous()
    p, w3, b3 = _place(torch.randn(B2, D, S, w, generator=g), device), _place(w3c, device), _place(torch.randn(nf, generator=g), device)
    gout = _place(torch.randn(B2, nf * D, n2, w, generator=g), device)
    st = ops._stream(p)
    ws = torch.empty((8 * 28,), dtype=torch.float64, device=device)
    # the full-frame sequence
    wz, z = _slot((B2, nf * D, S, w), device)
    assert lib.pnsfm_conv3d_forward(ops._ptr(p), ops._ptr(w3), ops._ptr(b3), ops._ptr(z), B2, D, S, w, nf, st) == 0
    _sync(device)
    _check_slot(wz, z, case['id'] + ' z')
    ref_out = torch.cat((z[:B, :, :n2], z[B:, :, 1:]), 0)
    dz = _place(torch.zeros(B2, nf * D, S, w), device)
    dz[:B, :, :n2] = gout[:B]
    dz[B:, :, 1:] = gout[B:]
    wdp, ref_dp = _slot((B2, D, S, w), device)
    wdw, ref_dw = _slot((nf, 1, 3, 3, 3), device)
    wdb, ref_db = _slot((nf,), device)
    assert lib.pnsfm_conv3d_backward_data(ops._ptr(dz), ops._ptr(w3), ops._ptr(ref_dp), B2, D, S, w, nf, st) == 0
    assert lib.pnsfm_conv3d_backward_weight(ops._ptr(p), ops._ptr(dz), ops._ptr(ref_dw), ops._ptr(ref_db), ops._ptr(ws), B2, D, S, w, nf, st) == 0
    _sync(device)
    for whole, t in ((wdp, ref_dp), (wdw, ref_dw), (wdb, ref_db)):
        _check_slot(whole, t, case['id'] + ' reference')

    def launch():
        wo, out = _slot((B2, nf * D, n2, w), device)
        wdp, dp = _slot((B2, D, S, w), device)
        wdw, dw = _slot((nf, 1, 3, 3, 3), device)
        wdb, db = _slot((nf,), device)
        assert lib.pnsfm_conv3d_rows_folded(ops._ptr(p), ops._ptr(out), w) == 1
        rc = lib.pnsfm_conv3d_forward_rows(ops._ptr(p), ops._ptr(w3), ops._ptr(b3), ops._ptr(out), B2, D, S, w, nf, B, st)
        assert rc == 0, (rc, lib.pnsfm_last_error())
        rc = lib.pnsfm_conv3d_backward_data_rows(ops._ptr(gout), ops._ptr(w3), ops._ptr(dp), B2, D, S, w, nf, B, st)
        assert rc == 0, (rc, lib.pnsfm_last_error())
        rc = lib.pnsfm_conv3d_backward_weight_rows(ops._ptr(p), ops._ptr(gout), ops._ptr(dw), ops._ptr(db), B2, D, S, w, nf, B, st)
        _sync(device)
        assert rc == 0, (rc, lib.pnsfm_last_error())
        for whole, t, what in ((wo, out, ' out'), (wdp, dp, ' dp'), (wdw, dw, ' dw3'), (wdb, db, ' db3')):
            _check_slot(whole, t, case['id'] + what)
        return out, dp, dw, db

    with _Fold(lib, 0):
        assert lib.pnsfm_conv3d_rows_folded(ops._ptr(p), ops._ptr(p), w) == 0
    with _Fold(lib, 1):
        outs = [launch() for _ in range(2)]
    for i, (what, ref) in enumerate((('out', ref_out), ('dp', ref_dp), ('dw3', ref_dw), ('db3', ref_db))):
        assert torch.equal(outs[0][i], ref), '%s %s: %d of %d elements differ from the full-frame sequence' % (
            case['id'], what, int((outs[0][i] != ref).sum()), ref.numel())
        assert torch.equal(outs[0][i], outs[1][i]), '%s %s: two launches differ' % (case['id'], what)


def run_bias(device, case):
    """pnsfm_pack_bias_eff_forward on the (d, C) grid against the one-workgroup-per-row kernel: Ssum and bias_eff bit for bit."""
    lib, ops = _lib_ops()
    C, d, blk = case['C'], case['d'], case['blk']
    g = torch.Generator().manual_seed(C + 3 * d + 7 * blk)
    W2 = _place(torch.randn(C, d * blk, generator=g), device)
    b2 = _place(torch.randn(C, generator=g), device) if case['b2'] else None
    b3 = _place(torch.randn(d, generator=g), device)

    def launch():
        ws, Ssum = _slot((C, d), device)
        wb, bias = _slot((C,), device)
        rc = lib.pnsfm_pack_bias_eff_forward(ops._ptr(W2), ops._ptr(b2), ops._ptr(b3), ops._ptr(Ssum), ops._ptr(bias), C, d, blk, ops._stream(W2))
        _sync(device)
        assert rc == 0, (rc, lib.pnsfm_last_error())
        _check_slot(ws, Ssum, case['id'] + ' Ssum')
        _check_slot(wb, bias, case['id'] + ' bias_eff')
        return Ssum, bias

    with _Fold(lib, 0):
        ref = launch()
    with _Fold(lib, 1):
        got = launch()
    want = W2.cpu().double().view(C, d, blk).sum(2)
    assert float((ref[0].cpu().double() - want).abs().max()) <= 1e-5 * float(W2.abs().cpu().double().view(C, d, blk).sum(2).max())
    assert torch.equal(got[0], ref[0]), case['id'] + ' Ssum'
    assert torch.equal(got[1], ref[1]), case['id'] + ' bias_eff'


def run_block(device, name):
    """One whole block, forward and backward, under both switch settings: output, input gradient and every parameter gradient equal."""
    from packnet_sfm.networks.layers.packnet.layers01 import PackLayerConv3d, UnpackLayerConv3d
    lib, _ = _lib_ops()
    torch.manual_seed(11)
    if name.startswith('pack'):
        m = PackLayerConv3d(16, int(name[-1]))
        m.collapse = 'collapsed' in name
    else:
        m = UnpackLayerConv3d(16, 32, 3)
    m = m.to(device).train()
    g = torch.Generator().manual_seed(12)
    xc = torch.randn(2, 16, 12, 16, generator=g)

    def run(on):
        with _Fold(lib, on):
            m.zero_grad(set_to_none=True)
            x = xc.clone().to(device).requires_grad_(True)
            y = m(x)
            dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(13)).to(device)
            y.backward(dy)
            _sync(device)
            return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    ref, got = run(0), run(1)
    names = ['y', 'dx'] + ['d' + n for n, _ in m.named_parameters()]
    assert len(ref) == len(got) == len(names)
    for n, a, b in zip(names, got, ref):
        assert not bool(torch.isnan(b).any()), n
        assert torch.equal(a, b), '%s %s: %d of %d elements differ between the switch settings' % (name, n, int((a != b).sum()), a.numel())
