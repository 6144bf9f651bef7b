"""Cases that tie the tuning-key query (pnsfm_tune_key), the decision codec of csrc/conv2d.hip and its Python copy
(packnet_sfm/hip/tune.py) together; shared by the emulated CPU tests (tests/test_kernels_emulated.py) and tests/test_gpu_tune.py.

  codec      every data line of the shipped database survives decode -> encode, and the decoded fields of every forward /
             backward-data line are the ones the replay on the GPU recorded (tests/golden/tuned_configs.json): no library needed.
  key        tune.key, fed a database line's own shape, returns the line's key (the database was written by the launches).
  launches   one per key rule: pin a decision that differs from the un-tuned one in a field pnsfm_conv2d_last_config reports, read
             it back, compare with torch, and see the un-tuned configuration return after the `with tune.pinned` block."""
import json
import os

import torch
import torch.nn.functional as F

import parity_cases as P
from packnet_sfm.hip import tune

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tuned_configs.json')


# ------------------------------------------------------------------------------------------------ codec (no library)
def check_codec_round_trip():
    lines = tune.database_lines()
    assert len(lines) == 346
    bad = [text for text, v in lines if tuple(tune.decode(v[0], v[7], v[8]).encode()) != (v[7], v[8])]
    assert not bad, 'lines that do not survive decode -> encode: %r' % bad


def check_codec_against_recorded_configurations():
    """tuned_configs.json: line text -> the eight ints of pnsfm_conv2d_last_config of the line's launch on an MI355X
    ([0] variant, [1] NT, [4] K-split, [5] tile mode)."""
    with open(GOLDEN) as f:
        recorded = json.load(f)
    lines = {text: v for text, v in tune.database_lines() if v[0] % 10 != tune.WGRAD}
    assert len(recorded) == 229 and sorted(recorded) == sorted(lines)
    bad = []
    for text, v in lines.items():
        d, c = tune.ConvDecision.decode(v[7], v[8]), recorded[text]
        if (d.variant, d.NT, d.tile_mode, d.split) != (c[0], c[1], c[5], c[4]):
            bad.append((text, d, c))
    assert not bad, 'decoded decision against the launch recorded on the GPU: %r' % bad


# ------------------------------------------------------------------------------------------------ key (library: any build)
def check_key_reproduces_database_lines():
    """Under the split-bf16 arithmetic the database was tuned for.  Forward / backward-data: H, W as the line holds them (a re-tiled
    1x1 line holds 32-wide rows, which the launch leaves alone).  Weight gradient, ks > 1: the key holds H*W and W.  The 1x1
    weight-gradient lines are left out for a structural reason: their key holds H*W and the constant 32, not the map's width, so the
    map the launch saw cannot be recovered from the line."""
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_get_conv_math() == 1
    n_conv = n_wgrad = n_1x1 = 0
    bad = []
    for text, v in tune.database_lines():
        kind, B, K, M, h, w, ks = v[:7]
        direction, S, _bx3, several = tune.kind_fields(kind)
        if direction != tune.WGRAD:
            got = tune.key(direction, B, K, M, h, w, ks, S)
            n_conv += 1
        elif ks > 1:
            assert h % w == 0, text
            got = tune.key(tune.WGRAD, B, K, M, h // w, w, ks, S, 2 if several else 1)
            n_wgrad += 1
        else:
            n_1x1 += 1
            continue
        if list(got) != v[:7]:
            bad.append((text, got))
    assert (n_conv, n_wgrad, n_1x1) == (229, 100, 17), (n_conv, n_wgrad, n_1x1)
    assert not bad, 'tune.key of a line\'s own shape is not the line\'s key (line, key): %r' % bad


# ------------------------------------------------------------------------------------------------ launches, one per key rule
# id, what (fwd | bwd | wgrad), x shape (B, Cin, H, W), Cout, ks, stride, sources, decision, the key the library must report
# (kinds: + 10 * stride, + 100 split-bf16, + 1000 several sources)
def _c(name, what, x, Cout, ks, dec, key, stride=1, srcs=None):
    return dict(id=name, what=what, x=x, Cout=Cout, ks=ks, stride=stride, srcs=srcs, dec=dec, key=key)


LAUNCH_CASES = [
    _c('a-3x3-fwd', 'fwd', (1, 48, 9, 32), 64, 3, tune.ConvDecision(2, 3, split=2), (110, 1, 48, 64, 9, 32, 3)),
    _c('a-3x3-bwd', 'bwd', (1, 48, 9, 32), 64, 3, tune.ConvDecision(2, 3, split=2), (111, 1, 64, 48, 9, 32, 3)),
    _c('b-1x1-4x40-retiled', 'fwd', (2, 80, 4, 40), 64, 1, tune.ConvDecision(2, 8, split=2), (110, 2, 80, 64, 5, 32, 1)),
    _c('c-1x1-5x7-as-is', 'fwd', (2, 48, 5, 7), 64, 1, tune.ConvDecision(1, 8, split=3), (110, 2, 48, 64, 5, 7, 1)),
    _c('d-3x3-stride2-fwd', 'fwd', (2, 32, 9, 48), 64, 3, tune.ConvDecision(1, 3, split=2), (120, 2, 32, 64, 5, 24, 3), stride=2),
    _c('e-3x3-wgrad-bx3', 'wgrad', (3, 48, 9, 32), 24, 3, tune.WgradDecision(2, 2, NT=1), (112, 3, 48, 24, 288, 32, 3)),
    _c('f-1x1-wgrad', 'wgrad', (3, 48, 9, 32), 24, 1, tune.WgradDecision(2, 2, NT=1), (112, 3, 48, 24, 288, 32, 1)),
    _c('g-stem-wgrad', 'wgrad', (2, 3, 6, 40), 64, 5, tune.WgradDecision(0, 2), (12, 2, 3, 64, 240, 40, 5)),      # 2 x 2 x 1 tiles of 4 x 64 pixels
    _c('h-two-sources-wgrad', 'wgrad', (3, 80, 6, 48), 40, 3, tune.WgradDecision(2, 4, NT=2), (1112, 3, 80, 40, 288, 48, 3), srcs=(64, 16)),
    _c('i-stride2-wgrad', 'wgrad', (3, 20, 9, 48), 24, 3, tune.WgradDecision(0, 2), (22, 3, 20, 24, 120, 24, 3), stride=2),
]
LAUNCH_IDS = [c['id'] for c in LAUNCH_CASES]


def run_launch_case(device, case, tol_conv, tol_wgrad):
    """tol_*: the tolerance of the neighbouring tests of these kernels on `device` (P.check: max error relative to the reference's
    maximum)."""
    from packnet_sfm.hip import _lib, ops, functional as HF
    lib = _lib.get()
    B, Cin, H, W = case['x']
    Cout, ks, S, what, dec = case['Cout'], case['ks'], case['stride'], case['what'], case['dec']
    g = torch.Generator().manual_seed(sum(case['x']) + Cout + ks)
    x = torch.randn(B, Cin, H, W, generator=g)
    wr = (torch.randn(Cout, Cin, ks, ks, generator=g) * 0.1).requires_grad_(True)
    br = torch.randn(Cout, generator=g).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, stride=S, padding=ks // 2)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy)
    Ho, Wo = yr.shape[2:]
    xd, dyd, wd, bd = x.to(device), dy.to(device), wr.detach().to(device), br.detach().to(device)

    def launch():
        """-> (results, references, tolerance, what tune.last_config reports)"""
        if what == 'wgrad':
            if case['srcs']:
                dw, db = ops.conv2d_backward_weight_cat([t.contiguous() for t in torch.split(xd, list(case['srcs']), 1)], dyd, ks)
            elif S == 2:
                dw, db = ops.conv2d_backward_weight_strided(xd, dyd, ks, 2)
            else:
                dw, db = ops.conv2d_backward_weight(xd, dyd, ks)
            return (dw, db), (wr.grad, br.grad), tol_wgrad, tune.last_config()
        wf, wb = ops.conv2d_pack(wd)
        if what == 'bwd':
            return (ops.conv2d_backward_data(dyd, wb, Cin, ks),), (xr.grad,), tol_conv, tune.last_config()
        y = ops.conv2d_forward_strided(xd, wf, bd, Cout, ks, 2) if S == 2 else ops.conv2d_forward(xd, wf, bd, Cout, ks)
        return (y,), (yr.detach(),), tol_conv, tune.last_config()

    prev_math = HF.set_conv_math('bx3')
    lib.pnsfm_set_autotune(0)
    try:
        tune.unpin()
        K, M = (Cout, Cin) if what == 'bwd' else (Cin, Cout)
        key = tune.key({'fwd': tune.FORWARD, 'bwd': tune.BACKWARD_DATA, 'wgrad': tune.WGRAD}[what], B, K, M, Ho, Wo, ks, S, len(case['srcs'] or (0,)))
        assert key == case['key'], key
        _, _, _, untuned = launch()
        with tune.pinned((key, dec)):
            got, ref, tol, ran = launch()
        print('%s: un-tuned %r  pinned %r' % (case['id'], untuned.raw, ran.raw))
        if what == 'wgrad':
            assert ran['split'] == dec.split and ran['split'] != untuned['split'], (ran, untuned)
            assert ran['variant'] == {0: 105 if Cin == 3 else 100, 2: 103}[dec.kernel] and (dec.kernel != 2 or ran['NT'] == dec.NT), ran
        else:
            assert (ran['variant'], ran['NT'], ran['split']) == (dec.variant, dec.NT, dec.split), ran
            assert (ran['NT'], ran['split']) != (untuned['NT'], untuned['split']), (ran, untuned)
        for a, b in zip(got, ref):
            P.check(a, b, tol, case['id'])
        _, _, _, after = launch()
        assert after.raw == untuned.raw, 'the un-tuned configuration did not return after the block: %r, was %r' % (after.raw, untuned.raw)
    finally:
        lib.pnsfm_set_autotune(1)
        HF.set_conv_math(prev_math)
