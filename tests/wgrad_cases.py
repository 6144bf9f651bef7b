"""Weight-gradient cases shared by the emulated CPU tests (tests/test_kernels_emulated.py) and the GPU tests
(tests/test_gpu_wgrad_ladder.py): one small case or more for EVERY kernel build a weight-gradient decision can launch --

  conv2d_wgrad3_kernel<KS, NT, WM, TC, MASKED, OCC>   58 reachable builds   (csrc/conv2d_wgrad3.hip: enqueue_wgrad3)
  conv2d_wgrad4_kernel<WCI, TG, TR, MASKED>           16 builds             (csrc/conv2d_wgrad4.hip: enqueue_wgrad4)
  conv2d_wgrad_kernel<MT> at stride 2                 2 builds x 2 tile modes (csrc/conv2d.hip: enqueue_wgrad_generic)

-- pinned (packnet_sfm.hip.tune) and checked against a float64 unfold + matmul on the CPU.  A case states the build it must launch;
run_case() reads the build that DID launch back through tune.last_config (a pin that the library re-routes or drops fails
there, before any number is compared), so the table's coverage of the ladders is proven by the library, not by a copy of its dispatch.

Bounds (tests/test_gpu_round3.py: the project's own measure at the training step's reduction lengths):
  max |dW - dW64| / sum |dY||X| <= 16 * 2^-24      max |db - db64| / sum |dY| <= 1.5e-7
A kernel that drops one of the six bf16 piece products is off by ~2^-16 of |dy||x| on the elements it hits: 250 x the bound."""
import torch
import torch.nn.functional as F

from packnet_sfm.hip import tune

DW_BOUND = 16 * 2.0 ** -24
DB_BOUND = 1.5e-7
GUARD = 260          # floats of NaN either side of a gradient slot: 1040 bytes -- the slot starts 16-byte, not 64-byte, aligned


def wgrad_fp64(x, dy, ks, stride=1):
    """dW[co][ci][ky][kx] = sum_{b,y,x} dY * X(shifted) in float64, and the same sum over |dY| |X| (the quantity rounding errors
    scale with), by unfold + matmul per image (rocBLAS dgemm: an implementation that shares nothing with the kernels under test)."""
    B, Cin, H, W = x.shape
    Cout, HWo = dy.shape[1], dy.shape[2] * dy.shape[3]
    dw = torch.zeros(Cout, Cin * ks * ks, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(dw)
    cstep = max(1, (1 << 28) // (H * W * ks * ks))              # <= 2 GiB of unfolded fp64 columns at a time
    for b in range(B):
        dyb = dy[b].double().reshape(Cout, HWo)
        for c0 in range(0, Cin, cstep):
            c1 = min(Cin, c0 + cstep)
            cols = F.unfold(x[b:b + 1, c0:c1].double(), ks, padding=ks // 2, stride=stride)[0]        # [(c1-c0)*k*k, Ho*Wo]
            dw[:, c0 * ks * ks:c1 * ks * ks] += dyb @ cols.t()
            mag[:, c0 * ks * ks:c1 * ks * ks] += dyb.abs() @ cols.abs().t()
            del cols
    return dw.view(Cout, Cin, ks, ks), mag.view(Cout, Cin, ks, ks)


# ------------------------------------------------------------------------------------------------ the read-back
def launched_tiles(cfg, B, H, W, ks):
    """Pixel tiles of the launch `cfg` (the eight ints of pnsfm_conv2d_last_config: tune.last_config().raw) describes (the unit the pixel split divides), from the tile shape it reports.  H, W: the map of
    dY; a 1x1 layer's map is handed to wgrad3 as 32-wide rows of the flattened image when that is exact."""
    code = cfg[0]
    if code == 103:
        if ks == 1 and (H * W) % 32 == 0:
            H, W = H * W // 32, 32
        return B * -(-W // cfg[3]) * -(-H // 4)
    if code == 104:
        return B * -(-W // (8 * cfg[2])) * -(-H // cfg[3])
    if code == 100:
        PT, mode = cfg[3], cfg[5]
        if ks == 1 and cfg[1] == 1:
            H, W = -(-H * W // 32), 32
        return B * ((W // 32) * -(-H // (PT // 32)) if mode == 0 else -(-H * W // PT))
    if code == 105:
        return B * -(-H // 4) * -(-W // 64)
    raise AssertionError('no tile rule for launch %r' % (cfg,))


def clamped_split(tiles, split):
    """What the kernels' split clamp makes of a requested pixel split: whole tiles per share, no empty share."""
    split = max(1, min(split, tiles))
    return -(-tiles // -(-tiles // split))


# ------------------------------------------------------------------------------------------------ the table
# A case: id, shape (B, Cin, Cout, H, W, ks) with H, W the map of x, srcs (channel counts of a multi-source launch, or None), stride,
# dec = the tune.WgradDecision to pin (`kernel`: one without its pixel split), build = what tune.last_config().build must return.
def _case(name, shape, kernel, split, build, srcs=None, stride=1):
    return dict(id=name, shape=shape, srcs=srcs, stride=stride, dec=kernel._replace(split=split), build=build)


def _w3(NT, wm):
    return tune.WgradDecision(2, NT=NT, wm=wm)


def _w4(WCI, TG, TR):
    return tune.WgradDecision(3, WCI=WCI, TG=TG, TR=TR)


# wgrad3.  Cout 24 / 40 / 100 fills 1 / 2 / 4 co tiles per workgroup (all ragged against the 32-row tile); Cin 48 = two 32-channel
# tiles, the second half empty (NT = 1), Cin 80 = two 64-channel tiles, the second ragged (NT = 2); W 32 -> 32-column tiles, W 48 ->
# 16-column tiles (48 < 64 columns per row), W 20 -> the masked build (W % 8 == 4).  1x1: a map with H*W % 32 == 0 is flattened to
# 32-wide rows, so the 16-column and masked builds need H*W % 32 != 0 (5 x 48, 5 x 20).  Every (B, H, W, split) below leaves a tile
# count that is NO multiple of the tiles per share: the last share is short (and split = 1 is launched next to it, run_case).
_W3_COUT = {1: 24, 2: 40, 4: 100}
_W3_CIN = {1: 48, 2: 80}
# (TC, masked) -> ks -> (B, H, W, split); tiles = B * ceil(W / TC) * ceil(H / 4) (1x1, 9 x 32: the flattened map is the same 9 x 32)
_W3_MAP = {
    (32, 0): {1: (3, 9, 32, 2), 3: (3, 9, 32, 2), 5: (5, 6, 32, 3), 7: (3, 9, 32, 2)},       # 9 = 5 + 4 | 10 = 4 + 4 + 2
    (16, 0): {1: (3, 5, 48, 4), 3: (3, 6, 48, 4), 5: (2, 9, 48, 4), 7: (3, 6, 48, 4)},       # 18 = 5 + 5 + 5 + 3
    (16, 1): {1: (5, 5, 20, 3), 3: (3, 9, 20, 4), 5: (3, 9, 20, 4), 7: (3, 9, 20, 4)},       # 20 = 7 + 7 + 6 | 18 = 5 + 5 + 5 + 3
}


def _wgrad3_cases():
    out = []
    for ks in (1, 3, 5, 7):
        for NT in ((1, 2) if ks <= 3 else (1,)):
            for WM in (1, 2, 4):
                for (TC, masked), maps in sorted(_W3_MAP.items(), reverse=True):
                    if (ks, NT, WM, TC) == (3, 2, 4, 32):
                        continue            # no such build: the request runs <3, 1, 4, 32> (enqueue_wgrad3, "tight")
                    B, H, W, split = maps[ks]
                    out.append(_case('w3-k%d-nt%d-wm%d-tc%d%s' % (ks, NT, WM, TC, 'm' if masked else ''),
                                     (B, _W3_CIN[NT], _W3_COUT[WM], H, W, ks), _w3(NT, 0), split, (103, ks, NT, WM, TC, masked, 2)))
    # the three-workgroups-per-CU builds: wm | 8 on a 3x3 layer, NT = 1, not masked; <3, 1, 4, 32, OCC 3> does not exist
    for WM, TC in ((1, 32), (2, 32), (1, 16), (2, 16), (4, 16)):
        B, H, W, split = _W3_MAP[(TC, 0)][3]
        out.append(_case('w3-k3-nt1-wm%d-tc%d-occ3' % (WM, TC), (B, 48, _W3_COUT[WM], H, W, 3), _w3(1, 8), split, (103, 3, 1, WM, TC, 0, 3)))
    # WM below the layer's maximum: the same builds as a small Cout, but several co groups and WK = 4 / WM pixel shares per workgroup
    # summed through LDS (one row per kernel size and tile form, both NT, one OCC = 3)
    for ks, NT, wm, key, occ in ((1, 1, 1, (32, 0), 0), (1, 2, 2, (16, 1), 0), (3, 1, 1, (16, 0), 0), (3, 1, 2, (32, 0), 0),
                                 (3, 2, 1, (32, 0), 0), (3, 2, 2, (16, 1), 0), (3, 1, 2, (16, 0), 8), (3, 1, 1, (32, 0), 8),
                                 (5, 1, 1, (16, 1), 0), (5, 1, 2, (32, 0), 0), (7, 1, 2, (16, 0), 0), (7, 1, 1, (32, 0), 0)):
        B, H, W, split = _W3_MAP[key][ks]
        out.append(_case('w3-k%d-nt%d-wm%d-tc%d%s%s-cout100' % (ks, NT, wm, key[0], 'm' if key[1] else '', '-occ3' if occ else ''),
                         (B, _W3_CIN[NT], 100, H, W, ks), _w3(NT, wm | occ), split, (103, ks, NT, wm, key[0], key[1], 3 if occ else 2)))
    return out


def _wgrad4_cases():
    # (TG, TR, masked) -> per WCI (B, H, W, split): W 24 / 20 = 3-group tiles plain / masked; W 64 (TG 4) and 80 (TG 5) whole tiles,
    # W 80 with TG 4 a ragged last tile, W 44 the masked 4- and 5-group builds; 6-row tiles (18 groups: the fifth k-step half empty) on
    # H = 9 and 6.  Cin 40 = three 16-channel tiles, the last half empty; Cout 40 / 100 against 64- (WCI 2) and 128-row (WCI 1) groups
    maps = {
        (3, 4, 0): {1: (3, 9, 24, 2), 2: (5, 6, 24, 3)},      # 9 = 5 + 4 | 10 = 4 + 4 + 2
        (3, 4, 1): {1: (3, 9, 20, 2), 2: (5, 6, 20, 3)},      # 10 = 4 + 4 + 2
        (3, 6, 0): {1: (5, 9, 24, 3), 2: (5, 6, 24, 2)},      # 10 = 4 + 4 + 2 | 5 = 3 + 2
        (3, 6, 1): {1: (5, 6, 20, 2), 2: (5, 9, 20, 3)},
        (4, 4, 0): {1: (2, 6, 64, 3), 2: (3, 9, 80, 2)},      # 8 = 3 + 3 + 2 | 27 = 14 + 13 (ragged last tile of a row)
        (4, 4, 1): {1: (2, 6, 44, 3), 2: (3, 9, 44, 4)},      # 8 | 18 = 5 + 5 + 5 + 3
        (5, 4, 0): {1: (2, 6, 80, 3), 2: (3, 9, 80, 4)},      # 8 | 18 = 5 + 5 + 5 + 3
        (5, 4, 1): {1: (2, 6, 44, 3), 2: (3, 9, 44, 4)},
    }
    out = []
    for (TG, TR, masked), per in sorted(maps.items()):
        for WCI in (1, 2):
            B, H, W, split = per[WCI]
            Cout = 100 if (WCI + TG + masked) % 2 else 40
            pinTG = 0 if W <= 24 else TG      # narrow images have one legal width (3 groups); the tile rows are always pinned
            out.append(_case('w4-wci%d-tg%d-tr%d%s' % (WCI, TG, TR, 'm' if masked else ''), (B, 40, Cout, H, W, 3),
                             _w4(WCI, pinTG, TR), split, (104, WCI, TG, TR, masked)))
    return out


def _cat_cases():
    # several input tensors (key kind + 1000): 32 + 48 channels -- the second tensor starts inside the launch's second 32-channel tile
    # row of workgroups -- and 64 + 16 for the 64-channel tiles of NT = 2
    return [
        _case('cat-w3-k3-nt2-wm2-tc16', (3, 80, 40, 6, 48, 3), _w3(2, 0), 4, (103, 3, 2, 2, 16, 0, 2), srcs=(64, 16)),
        _case('cat-w3-k3-nt1-wm2-tc32-occ3', (3, 80, 40, 9, 32, 3), _w3(1, 8), 2, (103, 3, 1, 2, 32, 0, 3), srcs=(32, 48)),
        _case('cat-w3-k5-nt1-wm1-tc16m', (3, 80, 24, 9, 20, 5), _w3(1, 0), 4, (103, 5, 1, 1, 16, 1, 2), srcs=(32, 48)),
        _case('cat-w4-wci2-tg4-tr4m', (3, 80, 40, 9, 44, 3), _w4(2, 4, 4), 4, (104, 2, 4, 4, 1), srcs=(32, 48)),
    ]


def _generic_cases():
    # the generic f32 kernel at stride 2 (kind 22) with a pinned split: Cout 24 and 72 run the 32-row build (MT 1: one and three co
    # tiles), Cout 40 the 64-row build (MT 2); tile mode 0 / 1 = output width 32 / 20.  shape: the map of x is twice the map of dY.
    out = []
    for ks, Cout, Wo, B, Ho, split in ((3, 24, 32, 3, 9, 2), (3, 40, 20, 3, 13, 2), (5, 72, 32, 3, 9, 2), (5, 24, 20, 3, 13, 2),
                                       (7, 40, 32, 5, 6, 3), (7, 72, 20, 3, 13, 2), (3, 72, 32, 3, 9, 2), (5, 40, 32, 3, 9, 2)):
        MT, mode = (2 if Cout == 40 else 1), (0 if Wo % 32 == 0 else 1)
        out.append(_case('gen-s2-k%d-cout%d-mt%d-mode%d' % (ks, Cout, MT, mode), (B, 20, Cout, 2 * Ho, 2 * Wo, ks), tune.WgradDecision(0), split,
                         (100, 2, MT, mode), stride=2))
    return out


CASES = _wgrad3_cases() + _wgrad4_cases() + _cat_cases() + _generic_cases()
CASE_IDS = [c['id'] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def expected_builds():
    """Every build the two split-bf16 dispatch ladders can launch, listed from enqueue_wgrad3 (PNSFM_W3 / PNSFM_W3T and the OCC = 3 and
    <3, 2, 4> branches) and enqueue_wgrad4 (PNSFM_W4G / PNSFM_W4).  A build added to a ladder must be added here, and then needs a case."""
    w3 = set()
    for ks in (1, 3, 5, 7):
        for NT in ((1, 2) if ks <= 3 else (1,)):          # two ci tiles per wave: 1x1 and 3x3 only
            for WM in (1, 2, 4):
                for TC, masked in ((32, 0), (16, 0), (16, 1)):
                    w3.add((103, ks, NT, WM, TC, masked, 2))
    w3.remove((103, 3, 2, 4, 32, 0, 2))                   # "unreachable build": re-routed to NT = 1
    for WM, TC in ((1, 32), (2, 32), (1, 16), (2, 16), (4, 16)):
        w3.add((103, 3, 1, WM, TC, 0, 3))
    w4 = {(104, WCI, TG, TR, masked) for WCI in (1, 2) for TG, TR in ((3, 4), (3, 6), (4, 4), (5, 4)) for masked in (0, 1)}
    assert len(w3) == 58 and len(w4) == 16
    return w3 | w4


def check_table():
    """What the table promises without running a kernel: every build of the two ladders has a case, and every split-bf16 case asks
    for a pixel split whose last share is short (run_case launches split = 1 next to it)."""
    have = {c['build'] for c in CASES if c['build'][0] in (103, 104)}
    assert have == expected_builds(), (sorted(expected_builds() - have), sorted(have - expected_builds()))
    for c in CASES:
        assert c['dec'].split > 1, c['id']


# ------------------------------------------------------------------------------------------------ the checker
def _slot(shape, device, dtype=torch.float32, offset=0):
    """A NaN-filled slot inside a larger NaN-filled 1-D tensor, GUARD elements of NaN either side: (whole tensor, view of the slot).
    offset: elements by which the slot starts past the guard (tests/pack3d_cases.py: a float32 slot 1, 2 or 3 elements off a
    16-byte boundary)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((GUARD + offset + n + GUARD,), float('nan'), dtype=dtype, device=device)
    slot = whole[GUARD + offset:GUARD + offset + n].view(shape)
    assert whole.data_ptr() % 16 == 0 and slot.data_ptr() % 16 == (GUARD + offset) * whole.element_size() % 16 and slot.is_contiguous()
    return whole, slot


def _launch(ops, case, xs, dy):
    """One launch into fresh NaN slots; ((whole, dw), (whole, db), tune.last_config()) -- the caller checks guards and coverage."""
    B, Cin, Cout, H, W, ks = case['shape']
    dev = dy.device
    wdw, dw = _slot((Cout, Cin, ks, ks), dev)
    wdb, db = _slot((Cout,), dev)
    if case['srcs']:
        ops.conv2d_backward_weight_cat(xs, dy, ks, dw_out=dw, db_out=db)
    elif case['stride'] == 2:
        ops.conv2d_backward_weight_strided(xs[0], dy, ks, 2, dw_out=dw, db_out=db)
    else:
        ops.conv2d_backward_weight(xs[0], dy, ks, dw_out=dw, db_out=db)
    cfg = tune.last_config()
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return (wdw, dw), (wdb, db), cfg


def _check_slot(whole, slot, what):
    n = slot.numel()
    lo = (slot.data_ptr() - whole.data_ptr()) // whole.element_size()
    assert lo >= GUARD and whole.numel() - (lo + n) >= GUARD
    assert bool(torch.isnan(whole[:lo]).all()) and bool(torch.isnan(whole[lo + n:]).all()), '%s: store outside the slot' % what
    assert not bool(torch.isnan(slot).any()), '%s: %d elements never written' % (what, int(torch.isnan(slot).sum()))


def run_case(device, case, with_single_split=True, repeat=True):
    """Pin the case's decision, launch, and check -- in this order -- the build that ran, the pixel splits launched, the guards
    around the gradient slots, that every element was written, the error against float64, and that a second launch is bit-identical.
    with_single_split: also launch the same build un-split; both stay within the float64 bound and within their summed errors of
    each other.  (The emulated tier turns both extra launches off: its fibers run one at a time, in one order.)  Returns the measured (dW, db) errors of the pinned launch (in units of the bounds' quantities)."""
    from packnet_sfm.hip import _lib, ops, functional as HF
    lib = _lib.get()
    B, Cin, Cout, H, W, ks = case['shape']
    S = case['stride']
    Ho, Wo = H // S, W // S
    dec = case['dec']
    split, v1 = dec.encode()

    g = torch.Generator().manual_seed(1000 + sum(case['shape']) + 7 * split + (v1 & 1023))
    x = torch.randn(B, Cin, H, W, generator=g) * torch.exp(0.5 * torch.randn(B, Cin, 1, 1, generator=g))
    dy = torch.randn(B, Cout, Ho, Wo, generator=g) * torch.exp(0.5 * torch.randn(B, Cout, 1, 1, generator=g))
    dw64, mag = wgrad_fp64(x, dy, ks, S)
    db64, dbmag = dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
    assert float(mag.min()) > 0
    if case['srcs']:
        assert sum(case['srcs']) == Cin
        xs = [t.contiguous().to(device) for t in torch.split(x, list(case['srcs']), 1)]
    else:
        xs = [x.to(device)]
    dyd = dy.to(device)

    def errors(dw, db):
        return (float(((dw.double().cpu() - dw64).abs() / mag).max()), float(((db.double().cpu() - db64).abs() / dbmag).max()))

    prev_math = HF.set_conv_math('bx3')
    lib.pnsfm_set_autotune(0)
    try:
        key = tune.key(tune.WGRAD, B, Cin, Cout, Ho, Wo, ks, S, len(case['srcs'] or (0,)))      # under the arithmetic set above
        with tune.pinned((key, dec)):
            (wdw, dw), (wdb, db), last = _launch(ops, case, xs, dyd)
            cfg = last.raw
            assert last.build == case['build'], 'pinned %r launched %r (last_config %r)' % (case['build'], last.build, cfg)
            tiles = launched_tiles(cfg, B, Ho, Wo, ks)
            assert cfg[4] == clamped_split(tiles, split), 'splits launched %d, asked %d of %d tiles' % (cfg[4], split, tiles)
            assert cfg[4] > 1 and tiles % -(-tiles // split) != 0, 'the case has no short last share (%d tiles, %d ways)' % (tiles, split)
            _check_slot(wdw, dw, 'dW')
            _check_slot(wdb, db, 'db')
            e_dw, e_db = errors(dw, db)
            print('%s: last_config %r  |dW-dW64|/sum|dY||X| %.3e  |db-db64|/sum|dY| %.3e' % (case['id'], cfg, e_dw, e_db))
            assert e_dw <= DW_BOUND, (e_dw, DW_BOUND)
            assert e_db <= DB_BOUND, (e_db, DB_BOUND)
            if repeat:
                (wdw2, dw2), (wdb2, db2), last2 = _launch(ops, case, xs, dyd)
                assert last2.raw == cfg
                assert torch.equal(dw2, dw) and torch.equal(db2, db), 'two launches of one build differ: the summation order is not fixed'
        if with_single_split:
            with tune.pinned((key, dec._replace(split=1))):
                (wdw1, dw1), (wdb1, db1), last1 = _launch(ops, case, xs, dyd)
                cfg1 = last1.raw
                assert last1.build == case['build'] and cfg1[4] == 1, cfg1
                _check_slot(wdw1, dw1, 'dW (one split)')
                _check_slot(wdb1, db1, 'db (one split)')
            e1_dw, e1_db = errors(dw1, db1)
            print('%s: one split  %.3e  %.3e' % (case['id'], e1_dw, e1_db))
            assert e1_dw <= DW_BOUND and e1_db <= DB_BOUND, (e1_dw, e1_db)
            d_dw = float(((dw.double().cpu() - dw1.double().cpu()).abs() / mag).max())
            d_db = float(((db.double().cpu() - db1.double().cpu()).abs() / dbmag).max())
            slack = 1 + 1e-9      # float64 rounding of the three quotients
            assert d_dw <= (e_dw + e1_dw) * slack and d_db <= (e_db + e1_db) * slack, (d_dw, e_dw, e1_dw, d_db, e_db, e1_db)
        return e_dw, e_db
    finally:
        lib.pnsfm_set_autotune(1)
        HF.set_conv_math(prev_math)
