"""Cases of the collapsed packing block's weight path without ATen copies and adds (PNSFM_PACK_WPATH; csrc/pack3d.hip, conv2d_bx3.h,
conv2d_wgrad3.hip, elementwise.hip, hip/functional.py: _PackGrads), shared by the emulated CPU tests (tests/test_pack_wpath_emulated.py)
and the GPU tests (tests/test_gpu_pack_wpath.py):

  packer    pnsfm_conv2d_pack_weights_t / pnsfm_conv2d_pack_item_fill_t: the packed images of W with the tap-transpose flag against
            the packed images of W.transpose(2, 3).contiguous() without it, both directions, per-layer call and table
  conv3d    forward / data gradient / weight gradient with the flag against the same calls on W3.transpose(3, 4).contiguous(); dW3 with
            the swap undone against the transposed result; whole volumes and the border strips' row window
  ring      the kernel composition and its Conv3d weight gradient on W2 itself (pnsfm_conv3d_backward_data_ring / _weight_ring) against
            the same kernels on F.pad(W2, (1, 1, 1, 1)); the composition node (ComposePackParamsFn) under both switch settings
  add-into  the four points where gradients meet inside a kernel -- the second stage of the split-bf16 weight gradients (a single
            pixel split, a split launch, a masked build), conv3d_wgrad_finish_kernel, pack_bias_eff_backward: the destination
            preloaded with a random g1 equals torch.add(g1, the kernel's plain output); a second launch gives the same bits
  block     PackLayerConv3d collapsed under both switch settings: output, input gradient and the four parameter gradients, with and
            without registered gradient slots, with a hook on W2 (the owner stands back), over two backward passes into an existing
            .grad

Nothing here may change a rounding, so every comparison is torch.equal.  Layout as in tests/pack3d_fold_cases.py: C-ABI launches go
into NaN-filled slots inside larger NaN-filled tensors (wgrad_cases._slot); asserted in this order: return code 0, guards still NaN,
every element written, equality."""
import torch
import torch.nn.functional as F

from wgrad_cases import _slot, _check_slot

EPI_ADD, EPI_TAPT = 1, 2


def ids(cases):
    return [c['id'] for c in cases]


# ------------------------------------------------------------------------------------------------ the table
# packer: (Cin, Cout, ks) -- ragged against the 16-channel chunk and the 32-row m-block, and exact
PACK_CASES = [dict(id='pack-%d-%d-k%d' % (ci, co, ks), Cin=ci, Cout=co, ks=ks) for ks in (3, 5) for ci, co in ((40, 24), (32, 32))]

# conv3d: whole volumes (B, D, H, W) -- one 4-wide group wide, several blocks -- and strip windows (r, w, B, D)
C3D_VOLUMES = [(1, 4, 3, 4), (2, 8, 5, 12), (1, 8, 16, 124)]
C3D_CASES = ([dict(id='vol-%s-nf%d' % ('x'.join(map(str, v)), nf), kind='vol', shape=v, nf=nf) for nf in (8, 4) for v in C3D_VOLUMES] +
             [dict(id='rows-r%d-w%d-B%d-D%d-nf%d' % (r, w, B, D, nf), kind='rows', r=r, w=w, B=B, D=D, nf=nf)
              for nf in (8, 4) for r, w, B, D in ((1, 4, 1, 5), (2, 36, 2, 8))])

# ring: W2 [C, d * D, k, k], D = 4 * C packed channels; len: the data gradient's run length (None: the launcher's choice)
RING_CASES = [dict(id='ring-k%d-d%d-len%s' % (k, d, ln), k=k, d=d, C=16, len=ln)
              for k in (3, 5) for d in (8, 4) for ln in ((None, 8, 3) if (k, d) == (3, 8) else (None,))]
COMPOSE_CASES = [dict(id='compose-k%d-d%d' % (k, d), k=k, d=d, C=16) for k in (3, 5) for d in (8, 4)]

# add-into, Conv2d weight gradient of the border strips: (B2, Cin, Cout, r, W) and the pinned decision (kernel, pixel split);
# kernel 2 = split-bf16 (one kernel row per workgroup), 3 = nine taps, 0 = generic f32 (the epilogue as a pass of its own)
ADD2_CASES = [
    dict(id='add2-k3-one-split', B2=2, Cin=32, Cout=32, r=1, W=16, kernel=2, split=1),
    dict(id='add2-k3-reduced', B2=4, Cin=40, Cout=24, r=1, W=32, kernel=2, split=3),
    dict(id='add2-k3-masked', B2=2, Cin=32, Cout=32, r=1, W=12, kernel=2, split=2),          # W % 8 != 0: the masked build
    dict(id='add2-k5-one-split', B2=2, Cin=32, Cout=16, r=2, W=16, kernel=2, split=1),
    dict(id='add2-k5-reduced', B2=2, Cin=32, Cout=16, r=2, W=24, kernel=2, split=2),
    dict(id='add2-nine-taps-one-split', B2=2, Cin=32, Cout=32, r=1, W=16, kernel=3, split=1),
    dict(id='add2-nine-taps-reduced', B2=4, Cin=32, Cout=32, r=1, W=24, kernel=3, split=2),
    dict(id='add2-generic', B2=2, Cin=32, Cout=32, r=1, W=16, kernel=0, split=1),
]
ADD3_CASES = [dict(id='add3-nf%d-%s' % (nf, kind), nf=nf, kind=kind) for nf in (8, 4) for kind in ('rows', 'ring', 'vol')]
ADDB_CASES = [dict(id='addb-%d-%d-%d-k%d%s' % (C, d, D, k, '' if b2 else '-nob2'), C=C, d=d, D=D, k=k, b2=b2)
              for C, d, D, k, b2 in ((3, 8, 5, 3, True), (70, 4, 12, 5, True), (16, 8, 64, 3, False))]

# whole blocks (GroupNorm(16) wants 16 channels): x [2, 16, 12, 16] -- its packed map is 6 x 8, the column strips are 6 wide and take
# the Conv3d's full-frame fallback, so the block keeps the former strip path and only the composition changes -- and x [2, 16, 16, 24],
# packed 8 x 12: both strip directions on the row-window kernels, the gradient owner in charge (`owner`: what the case expects)
BLOCK_CASES = [dict(id='block-%dx%d-k%d-d%d-%s-%s' % (hw[0], hw[1], k, d, 'lrt' if t else 'lr', mode), hw=hw, k=k, d=d, lr_t=t, mode=mode,
                    owner=(t and hw == (16, 24) and mode in ('plain', 'slots')))
               for hw in ((12, 16), (16, 24)) for k in (3, 5) for d in (8, 4) for t in (True, False)
               for mode in ('plain', 'slots', 'hook', 'twice') if (t and hw == (16, 24)) or mode == 'plain']


def check_table():
    assert {(c['Cin'], c['Cout'], c['ks']) for c in PACK_CASES} == {(40, 24, 3), (32, 32, 3), (40, 24, 5), (32, 32, 5)}
    assert any(c['kind'] == 'vol' and c['shape'][3] == 4 for c in C3D_CASES) and {c['nf'] for c in C3D_CASES} == {4, 8}
    assert {(c['k'], c['d']) for c in RING_CASES} == {(3, 8), (3, 4), (5, 8), (5, 4)} and all(c['C'] == 16 for c in RING_CASES)
    assert any(c['split'] == 1 for c in ADD2_CASES) and any(c['split'] > 1 for c in ADD2_CASES) and any(c['W'] % 8 for c in ADD2_CASES)
    for hw in ((12, 16), (16, 24)):
        assert {(c['k'], c['d'], c['lr_t']) for c in BLOCK_CASES if c['hw'] == hw} == {(k, d, t) for k in (3, 5) for d in (8, 4) for t in (True, False)}
    assert {c['mode'] for c in BLOCK_CASES if c['lr_t'] and c['hw'] == (16, 24)} == {'plain', 'slots', 'hook', 'twice'}
    assert any(c['owner'] for c in BLOCK_CASES) and all((c['hw'][0] // 2) % 4 == 0 and (c['hw'][1] // 2) % 4 == 0 for c in BLOCK_CASES if c['owner'])
    for cases in (PACK_CASES, C3D_CASES, RING_CASES, COMPOSE_CASES, ADD2_CASES, ADD3_CASES, ADDB_CASES, BLOCK_CASES):
        assert len(set(ids(cases))) == len(cases)


# ------------------------------------------------------------------------------------------------ helpers
def _lib_ops():
    from packnet_sfm.hip import _lib, ops
    return _lib.get(), ops


def _place(t, device):
    _, s = _slot(t.shape, device, t.dtype)
    s.copy_(t)
    return s


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def _eq(a, b, what):
    assert torch.equal(a, b), '%s: %d of %d elements differ' % (what, int((a != b).sum()), a.numel())


def _ok(rc, lib):
    assert rc == 0, (rc, lib.pnsfm_last_error())


# ------------------------------------------------------------------------------------------------ packer
def run_packer(device, case):
    lib, ops = _lib_ops()
    Cin, Cout, ks = case['Cin'], case['Cout'], case['ks']
    assert ops.conv2d_pack_tapT_supported(Cin, Cout, ks)
    g = torch.Generator().manual_seed(100 * Cin + Cout + ks)
    W = _place(torch.randn(Cout, Cin, ks, ks, generator=g), device)
    Wt = _place(W.transpose(2, 3).contiguous(), device)
    nf, nb = ops.conv2d_packed_sizes(Cin, Cout, ks)

    def per_layer(w, tapT):
        wf, pf = _slot((nf,), device)
        wb, pb = _slot((nb,), device)
        st = ops._stream(w)
        if tapT:
            rc = lib.pnsfm_conv2d_pack_weights_t(ops._ptr(w), ops._ptr(pf), ops._ptr(pb), Cin, Cout, ks, 1, st)
        else:
            rc = lib.pnsfm_conv2d_pack_weights(ops._ptr(w), ops._ptr(pf), ops._ptr(pb), Cin, Cout, ks, st)
        _sync(device)
        _ok(rc, lib)
        return (wf, pf), (wb, pb)

    def table(w, tapT):
        wf, pf = _slot((nf,), device)
        wb, pb = _slot((nb,), device)
        # a second, plain item in the same table: the flag belongs to its item alone
        wf2, pf2 = _slot((nf,), device)
        wb2, pb2 = _slot((nb,), device)
        tab, n, blocks, covered = ops.conv2d_pack_table_build([(w, pf, pb, tapT), (Wt, pf2, pb2)], torch.device(device))
        assert n == 2 and covered == [0, 1]
        ops.conv2d_pack_table_run(tab, n, blocks)
        _sync(device)
        return (wf, pf), (wb, pb), (wf2, pf2), (wb2, pb2)

    ref = per_layer(Wt, False)
    got = per_layer(W, True)
    tab = table(W, True)
    # (the packed images have padding the packer writes as zero splits: every byte is written)
    for (wr, r), (wg, gt), (wt, t), (w2, t2), what in zip(ref, got, tab[:2], tab[2:], ('forward image', 'backward-data image')):
        for whole, x in ((wr, r), (wg, gt), (wt, t), (w2, t2)):
            lo = (x.data_ptr() - whole.data_ptr()) // 4
            assert bool(torch.isnan(whole[:lo]).all()) and bool(torch.isnan(whole[lo + x.numel():]).all()), case['id'] + ': store outside the slot'
        bits = lambda x: x.view(torch.int32)
        _eq(bits(gt), bits(r), case['id'] + ' per-layer ' + what)
        _eq(bits(t), bits(r), case['id'] + ' table ' + what)
        _eq(bits(t2), bits(r), case['id'] + ' table, plain item ' + what)


# ------------------------------------------------------------------------------------------------ conv3d taps
def run_conv3d(device, case):
    lib, ops = _lib_ops()
    nf = case['nf']
    rows = case['kind'] == 'rows'
    if rows:
        r, w, B, D = case['r'], case['w'], case['B'], case['D']
        S, B2 = 2 * r + 1, 2 * B
        pshape, oshape = (B2, D, S, w), (B2, nf * D, 2 * r, w)
    else:
        B2, D, H, w = case['shape']
        pshape, oshape = (B2, D, H, w), (B2, nf * D, H, w)
    g = torch.Generator().manual_seed(7 * sum(pshape) + nf)
    w3c = 0.3 * torch.randn(nf, 1, 3, 3, 3, generator=g)
    W3, W3t = _place(w3c, device), _place(w3c.transpose(3, 4).contiguous(), device)
    b3 = _place(torch.randn(nf, generator=g), device)
    p = _place(torch.randn(pshape, generator=g), device)
    gout = _place(torch.randn(oshape, generator=g), device)
    st = ops._stream(p)
    ws = torch.empty((8 * 28,), dtype=torch.float64, device=device)
    P = ops._ptr

    def launch(flag):
        """(out, dp, dw3, db3) -- flag: with the tap flag on W3; else the plain calls on the materialised transpose."""
        wo, out = _slot(oshape, device)
        wdp, dp = _slot(pshape, device)
        wdw, dw = _slot((nf, 1, 3, 3, 3), device)
        wdb, db = _slot((nf,), device)
        if rows and flag:
            _ok(lib.pnsfm_conv3d_forward_rows_t(P(p), P(W3), P(b3), P(out), B2, D, S, w, nf, B, 1, st), lib)
            _ok(lib.pnsfm_conv3d_backward_data_rows_t(P(gout), P(W3), P(dp), B2, D, S, w, nf, B, 1, st), lib)
            _ok(lib.pnsfm_conv3d_backward_weight_rows_epi(P(p), P(gout), P(dw), P(db), B2, D, S, w, nf, B, EPI_TAPT, st), lib)
        elif rows:
            _ok(lib.pnsfm_conv3d_forward_rows(P(p), P(W3t), P(b3), P(out), B2, D, S, w, nf, B, st), lib)
            _ok(lib.pnsfm_conv3d_backward_data_rows(P(gout), P(W3t), P(dp), B2, D, S, w, nf, B, st), lib)
            _ok(lib.pnsfm_conv3d_backward_weight_rows(P(p), P(gout), P(dw), P(db), B2, D, S, w, nf, B, st), lib)
        elif flag:
            _ok(lib.pnsfm_conv3d_forward_t(P(p), P(W3), P(b3), P(out), B2, D, H, w, nf, 1, st), lib)
            _ok(lib.pnsfm_conv3d_backward_data_t(P(gout), P(W3), P(dp), B2, D, H, w, nf, 1, st), lib)
            _ok(lib.pnsfm_conv3d_backward_weight_epi(P(p), P(gout), P(dw), P(db), B2, D, H, w, nf, EPI_TAPT, st), lib)
        else:
            _ok(lib.pnsfm_conv3d_forward(P(p), P(W3t), P(b3), P(out), B2, D, H, w, nf, st), lib)
            _ok(lib.pnsfm_conv3d_backward_data(P(gout), P(W3t), P(dp), B2, D, H, w, nf, st), lib)
            _ok(lib.pnsfm_conv3d_backward_weight(P(p), P(gout), P(dw), P(db), P(ws), B2, D, H, w, nf, st), lib)
        _sync(device)
        for whole, t, what in ((wo, out, ' out'), (wdp, dp, ' dp'), (wdw, dw, ' dw3'), (wdb, db, ' db3')):
            _check_slot(whole, t, case['id'] + what)
        return out, dp, dw, db

    ref = launch(False)
    got = launch(True)
    _eq(got[0], ref[0], case['id'] + ' forward')
    _eq(got[1], ref[1], case['id'] + ' data gradient')
    _eq(got[2], ref[2].transpose(3, 4).contiguous(), case['id'] + ' weight gradient, swap undone')
    _eq(got[3], ref[3], case['id'] + ' bias gradient')
    # the flag is not a no-op on these weights
    assert not torch.equal(W3, W3t)


# ------------------------------------------------------------------------------------------------ implicit ring
def _ring_inputs(case, device):
    k, d, C = case['k'], case['d'], case['C']
    D = 4 * C
    g = torch.Generator().manual_seed(31 * k + d)
    W2 = _place(torch.randn(C, d * D, k, k, generator=g) / (d * D) ** 0.5, device)
    W3 = _place(0.3 * torch.randn(d, 1, 3, 3, 3, generator=g), device)
    gW = _place(torch.randn(C, D, k + 2, k + 2, generator=g), device)
    return k, d, C, D, W2, W3, gW


def run_ring(device, case):
    """The two stencil kernels on W2 inside the implicit ring against themselves on the zero-padded copy."""
    lib, ops = _lib_ops()
    k, d, C, D, W2, W3, gW = _ring_inputs(case, device)
    W2pad = _place(F.pad(W2, (1, 1, 1, 1)), device)
    st = ops._stream(W2)
    ws = torch.empty((8 * 28,), dtype=torch.float64, device=device)
    P = ops._ptr

    def launch(ring):
        we, Weff = _slot((C, D, k + 2, k + 2), device)
        wdw, dw = _slot((d, 1, 3, 3, 3), device)
        wdb, db = _slot((d,), device)
        if ring:
            _ok(lib.pnsfm_conv3d_backward_data_ring(P(W2), P(W3), P(Weff), C, D, k, k, d, st), lib)
            _ok(lib.pnsfm_conv3d_backward_weight_ring(P(gW), P(W2), P(dw), P(db), C, D, k, k, d, 0, st), lib)
        else:
            _ok(lib.pnsfm_conv3d_backward_data(P(W2pad), P(W3), P(Weff), C, D, k + 2, k + 2, d, st), lib)
            _ok(lib.pnsfm_conv3d_backward_weight(P(gW), P(W2pad), P(dw), P(db), P(ws), C, D, k + 2, k + 2, d, st), lib)
        _sync(device)
        for whole, t, what in ((we, Weff, ' W_eff'), (wdw, dw, ' dW3'), (wdb, db, ' db3')):
            _check_slot(whole, t, case['id'] + what)
        return Weff, dw, db

    ref = launch(False)
    got = [launch(True) for _ in range(2)]
    for i, what in enumerate(('composition', 'dW3', 'bias sums')):
        _eq(got[0][i], ref[i], case['id'] + ' ' + what)
        _eq(got[1][i], got[0][i], case['id'] + ' ' + what + ', second launch')
    # a null bias destination is skipped
    wdw, dw = _slot((d, 1, 3, 3, 3), device)
    _ok(lib.pnsfm_conv3d_backward_weight_ring(P(gW), P(W2), P(dw), None, C, D, k, k, d, 0, st), lib)
    _sync(device)
    _check_slot(wdw, dw, case['id'] + ' dW3, no bias')
    _eq(dw, ref[1], case['id'] + ' dW3, no bias')


def run_compose(device, case):
    """ComposePackParamsFn forward and both gradients with the switch on (W2 itself) and off (F.pad(W2))."""
    from packnet_sfm.hip import functional as HF
    k, d, C, D, W2c, W3c, gWc = _ring_inputs(case, device)
    g = torch.Generator().manual_seed(5)
    b2c, b3c, gbc = torch.randn(C, generator=g).to(device), torch.randn(d, generator=g).to(device), torch.randn(C, generator=g).to(device)

    def run(on):
        prev = HF.set_pack_wpath(on)
        try:
            leaves = [t.clone().requires_grad_(True) for t in (W2c, b2c, W3c, b3c)]
            Weff, beff = HF.compose_pack_params(*leaves)
            torch.autograd.backward([Weff, beff], [gWc.clone(), gbc.clone()])
            _sync(device)
            return [Weff.detach(), beff.detach()] + [t.grad for t in leaves]
        finally:
            HF.set_pack_wpath(prev)

    ref, got = run(False), run(True)
    for n, a, b in zip(('W_eff', 'bias_eff', 'dW2', 'db2', 'dW3', 'db3'), got, ref):
        assert not bool(torch.isnan(b).any()), n
        _eq(a, b, case['id'] + ' ' + n)


# ------------------------------------------------------------------------------------------------ add-into
def run_add2(device, case):
    """pnsfm_conv2d_backward_weight_epi on a border-strip row window under a pinned decision: ADD, TAPT and both against the plain
    launch of the same decision."""
    lib, ops = _lib_ops()
    B2, Cin, Cout, r, W = case['B2'], case['Cin'], case['Cout'], case['r'], case['W']
    ks = 2 * r + 1
    g = torch.Generator().manual_seed(B2 + 3 * Cin + 5 * Cout + 7 * W + ks)
    x = _place(torch.randn(B2, Cin, 2 * r, W, generator=g), device)
    dy = _place(torch.randn(B2, Cout, r, W, generator=g), device)
    g1w, g1b = torch.randn(Cout, Cin, ks, ks, generator=g).to(device), torch.randn(Cout, generator=g).to(device)
    st = ops._stream(x)
    P = ops._ptr
    from packnet_sfm.hip import tune
    want_code = {2: 103, 3: 104, 0: 100}[case['kernel']]
    with tune.pinned((tune.key_rows(tune.WGRAD, B2, Cin, Cout, r, 2 * r, W, ks), tune.WgradDecision(kernel=case['kernel'], split=case['split']))):
        def launch(epi, preload):
            wdw, dw = _slot((Cout, Cin, ks, ks), device)
            wdb, db = _slot((Cout,), device)
            if preload:
                dw.copy_(g1w)
                db.copy_(g1b)
            if epi:
                rc = lib.pnsfm_conv2d_backward_weight_epi(P(x), P(dy), P(dw), P(db), B2, Cin, Cout, r, 2 * r, W, ks, r, B2 // 2, epi, st)
            else:
                rc = lib.pnsfm_conv2d_backward_weight_rows(P(x), P(dy), P(dw), P(db), B2, Cin, Cout, r, 2 * r, W, ks, r, B2 // 2, st)
            _sync(device)
            _ok(rc, lib)
            cfg = tune.last_config()
            assert cfg['variant'] == want_code and (cfg['split'] > 1) == (case['split'] > 1), (case['id'], cfg)
            if want_code == 103:
                assert cfg['masked'] == int(W % 8 != 0), (case['id'], cfg)
            _check_slot(wdw, dw, case['id'] + ' dw')
            _check_slot(wdb, db, case['id'] + ' db')
            return dw, db

        pw, pb = launch(0, False)
        for epi, want_w, want_b in ((EPI_ADD, torch.add(g1w, pw), torch.add(g1b, pb)),
                                    (EPI_TAPT, pw.transpose(2, 3).contiguous(), pb),
                                    (EPI_ADD | EPI_TAPT, torch.add(g1w, pw.transpose(2, 3).contiguous()), torch.add(g1b, pb))):
            a = launch(epi, bool(epi & EPI_ADD))
            b = launch(epi, bool(epi & EPI_ADD))
            _eq(a[0], want_w, '%s epi %d dw' % (case['id'], epi))
            _eq(a[1], want_b, '%s epi %d db' % (case['id'], epi))
            _eq(b[0], a[0], '%s epi %d dw, second launch' % (case['id'], epi))
            _eq(b[1], a[1], '%s epi %d db, second launch' % (case['id'], epi))


def run_add3(device, case):
    """conv3d_wgrad_finish_kernel adding into dW3 / db3: the row window, the ring and a whole volume."""
    lib, ops = _lib_ops()
    nf, kind = case['nf'], case['kind']
    g = torch.Generator().manual_seed(nf + len(kind))
    P = ops._ptr
    if kind == 'rows':
        B, D, r, w = 2, 8, 1, 36
        p = _place(torch.randn(2 * B, D, 2 * r + 1, w, generator=g), device)
        dout = _place(torch.randn(2 * B, nf * D, 2 * r, w, generator=g), device)
        call = lambda dw, db, epi: lib.pnsfm_conv3d_backward_weight_rows_epi(P(p), P(dout), P(dw), P(db), 2 * B, D, 2 * r + 1, w, nf, B, epi,
                                                                             ops._stream(p))
    elif kind == 'ring':
        C, D, k = 16, 64, 3
        p = _place(torch.randn(C, D, k + 2, k + 2, generator=g), device)
        dout = _place(torch.randn(C, nf * D, k, k, generator=g), device)
        call = lambda dw, db, epi: lib.pnsfm_conv3d_backward_weight_ring(P(p), P(dout), P(dw), P(db), C, D, k, k, nf, epi, ops._stream(p))
    else:
        B, D, H, w = 2, 8, 5, 12
        p = _place(torch.randn(B, D, H, w, generator=g), device)
        dout = _place(torch.randn(B, nf * D, H, w, generator=g), device)
        call = lambda dw, db, epi: lib.pnsfm_conv3d_backward_weight_epi(P(p), P(dout), P(dw), P(db), B, D, H, w, nf, epi, ops._stream(p))
    g1w, g1b = torch.randn(nf, 1, 3, 3, 3, generator=g).to(device), torch.randn(nf, generator=g).to(device)

    def launch(epi):
        wdw, dw = _slot((nf, 1, 3, 3, 3), device)
        wdb, db = _slot((nf,), device)
        if epi & EPI_ADD:
            dw.copy_(g1w)
            db.copy_(g1b)
        rc = call(dw, db, epi)
        _sync(device)
        _ok(rc, lib)
        _check_slot(wdw, dw, case['id'] + ' dw3')
        _check_slot(wdb, db, case['id'] + ' db3')
        return dw, db

    pw, pb = launch(0)
    for epi, want_w, want_b in ((EPI_ADD, torch.add(g1w, pw), torch.add(g1b, pb)),
                                (EPI_ADD | EPI_TAPT, torch.add(g1w, pw.transpose(3, 4).contiguous()), torch.add(g1b, pb))):
        a, b = launch(epi), launch(epi)
        _eq(a[0], want_w, '%s epi %d dw3' % (case['id'], epi))
        _eq(a[1], want_b, '%s epi %d db3' % (case['id'], epi))
        _eq(b[0], a[0], '%s epi %d dw3, second launch' % (case['id'], epi))
        _eq(b[1], a[1], '%s epi %d db3, second launch' % (case['id'], epi))


def run_addb(device, case):
    """pnsfm_pack_bias_eff_backward_add: db3, dW2 and db2 preloaded against torch.add of the plain outputs (db2's plain output is g)."""
    lib, ops = _lib_ops()
    C, d, D, k = case['C'], case['d'], case['D'], case['k']
    g = torch.Generator().manual_seed(C + d + D + k)
    gb = _place(torch.randn(C, generator=g), device)
    Ssum = _place(torch.randn(C, d, generator=g), device)
    b3 = _place(torch.randn(d, generator=g), device)
    full = _place(torch.randn(C, d * D, k + 2, k + 2, generator=g), device)
    g1 = [torch.randn(s, generator=g).to(device) for s in ((d,), (C, d * D, k, k), (C,))]
    st = ops._stream(gb)
    P = ops._ptr

    def launch(add):
        slots = [_slot(s, device) for s in ((d,), (C, d * D, k, k), (C,))]
        (w3_, db3), (w2_, dW2), (wb_, db2) = slots
        if add:
            for (_, t), v in zip(slots, g1):
                t.copy_(v)
            rc = lib.pnsfm_pack_bias_eff_backward_add(P(gb), P(Ssum), P(b3), P(full), P(db3), P(dW2), P(db2) if case['b2'] else None, C, d, D, k, st)
        else:
            rc = lib.pnsfm_pack_bias_eff_backward(P(gb), P(Ssum), P(b3), P(full), P(db3), P(dW2), C, d, D, k, st)
        _sync(device)
        _ok(rc, lib)
        _check_slot(w3_, db3, case['id'] + ' db3')
        _check_slot(w2_, dW2, case['id'] + ' dW2')
        if add:
            _check_slot(wb_, db2, case['id'] + ' db2')
        return db3, dW2, db2

    plain = launch(False)
    a, b = launch(True), launch(True)
    _eq(a[0], torch.add(g1[0], plain[0]), case['id'] + ' db3')
    _eq(a[1], torch.add(g1[1], plain[1]), case['id'] + ' dW2')
    _eq(a[2], torch.add(g1[2], gb) if case['b2'] else g1[2], case['id'] + ' db2')
    for i, n in enumerate(('db3', 'dW2', 'db2')):
        _eq(b[i], a[i], case['id'] + ' ' + n + ', second launch')


# ------------------------------------------------------------------------------------------------ whole blocks
def run_block(device, case):
    """PackLayerConv3d collapsed, forward and backward, under both switch settings."""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.networks.layers.packnet.layers01 import PackLayerConv3d
    k, d, mode = case['k'], case['d'], case['mode']
    torch.manual_seed(11)
    m = PackLayerConv3d(16, k, d=d)
    m.collapse = True
    m.lr_transposed = case['lr_t']
    m = m.to(device).train()
    xc = torch.randn(2, 16, case['hw'][0], case['hw'][1], generator=torch.Generator().manual_seed(12))
    params = [p for _, p in m.named_parameters()]
    block4 = [m.conv.conv_base.weight, m.conv.conv_base.bias, m.conv3d.weight, m.conv3d.bias]

    def run(on):
        prev = HF.set_pack_wpath(on)
        handle = hook = None
        hooked = []
        try:
            m.zero_grad(set_to_none=True)
            arena = None
            if mode == 'slots':
                # what FlatAdam registers: views of one flat gradient arena (NaN-filled here: every element must be written)
                arena = torch.full((sum(p.numel() for p in params),), float('nan'), device=device)
                views, o = [], 0
                for p in params:
                    views.append(arena[o:o + p.numel()].view_as(p))
                    o += p.numel()
                handle = HF.register_grad_slots(zip(params, views))
            if mode == 'hook':
                hook = m.conv.conv_base.weight.register_hook(lambda gr: hooked.append(gr.detach().clone()) or None)
            outs = []
            passes0 = HF._PackGrads.passes
            for it in range(2 if mode == 'twice' else 1):
                x = xc.clone().to(device).requires_grad_(True)
                y = m(x)
                dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(13 + it)).to(device)
                y.backward(dy)
                _sync(device)
                outs += [y.detach().clone(), x.grad.clone()]
            grads = [p.grad.clone() for p in params]
            # the owner was in charge exactly where the case says: never with the switch off, behind a hook or into an existing .grad
            # (the second pass of 'twice'; its first pass finds no .grad and is the owner's)
            want = (1 if (on and (case['owner'] or (mode == 'twice' and case['lr_t'] and case['hw'] == (16, 24)))) else 0)
            assert HF._PackGrads.passes - passes0 == want, (case['id'], on, HF._PackGrads.passes - passes0)
            if mode == 'slots' and on:
                # the owner's four gradients were written where the optimizer reads them: no gather copy left to do
                ptrs = {v.data_ptr() for v in views}
                assert all(p.grad.data_ptr() in ptrs for p in block4), 'a gradient of the block did not land in its slot'
            return outs + grads + hooked
        finally:
            HF.set_pack_wpath(prev)
            if handle is not None:
                handle.remove()
            if hook is not None:
                hook.remove()
            m.zero_grad(set_to_none=True)

    ref, got = run(False), run(True)
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert not bool(torch.isnan(b).any()), i
        _eq(a, b, '%s tensor %d' % (case['id'], i))
