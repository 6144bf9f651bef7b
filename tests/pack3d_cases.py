"""Cases of csrc/pack3d.hip shared by the emulated CPU tests (tests/test_kernels_emulated.py, tests/test_half_emulated.py) and the
GPU tests (tests/test_gpu_pack3d.py): the two shuffles (per-element and 16-byte forms, fp32 and fp16), the 3x3x3 Conv3d(1 -> NF)
forward (per-voxel and four-voxels-per-thread forms, fp32 and fp16), its data gradient (column kernel at runs of 8 / 4 / 2 planes,
sliding kernel) and its weight / bias gradient (both builds), at the shapes where their lane, chunk and row arithmetic has edges.

Every launch goes through the C ABI into a NaN-filled slot inside a larger NaN-filled flat tensor (wgrad_cases._slot: 260 elements
of guard either side); the inputs sit in such tensors too, so that a case can put a tensor 1, 2 or 3 elements off a 16-byte
boundary and a load that strays outside a tensor reads NaN.  Asserted in this order: return code 0, guards still NaN, no NaN left
in the slot, the error bound; for the gradients also that a second launch into a fresh slot is bit-identical.

Reference: torch.nn.functional.conv3d in float64 on the CPU and its float64 autograd.  The magnitudes the rounding errors scale with
are the same computation on absolute values.  Per-element bounds, worst cases by derivation (u = 2^-24), not tuned:
  forward y        32 u (|b3| + sum |w3||p|)       27 FMAs chained from the bias
  data gradient    (27 NF + 8) u sum |w3||dy|      27 NF FMAs into one accumulator
  dw3              40 u sum |dy||p|                <= 12 fp32 products per thread (check_table), conv3d_wgrad_block_reduce's 16 serial
  db3              40 u sum |dy|                    + 4 shuffle adds, one fp64 -> fp32 cast; the rest is fp64
  fp16 forward     one fp16 ulp + 2^-18 sum |w3||p|   (half_cases.assert_close16)
No volume exceeds 50 000 voxels per image, so one dropped voxel is ~1 / 50 000 of sum |dy||p|: about 8 x the dw3 bound.
The shuffles move data: bit-exact against F.pixel_unshuffle / F.pixel_shuffle.

There is no read-back of the kernel these launches chose (no C ABI symbol for it).  In its place a case states the path it is meant
to take and check_table() restates the launcher's conditions (pnsfm_space_to_depth, pnsfm_depth_to_space, pnsfm_conv3d_forward,
pnsfm_conv3d_backward_data, pnsfm_conv3d_backward_weight) on the case's own shape and on the alignment of slots built as the run
builds them."""
import functools
import os

import torch
import torch.nn.functional as F

import half_cases as HC
from wgrad_cases import _slot, _check_slot

U = 2.0 ** -24
FWD_BOUND = 32.0
DW_BOUND = 40.0
DB_BOUND = 40.0
MAX_VOXELS = 50000
NFS = (8, 4)


def dgrad_bound(nf):
    return 27.0 * nf + 8.0


def _sid(shape):
    return 'x'.join(str(s) for s in shape)


# ------------------------------------------------------------------------------------------------ the table
# Shapes are (B, D, H, W).  In every list the shapes the emulated tests ran before this table come first, in their order.
FWD_X4_SHAPES = [(1, 5, 4, 8), (2, 13, 3, 4), (1, 9, 5, 12), (1, 1, 2, 4), (1, 6, 2, 64),
                 (2, 7, 9, 36)]                   # 7 * 9 * 9 = 567 thread items: three blocks, ragged last
FWD_VOXEL_SHAPES = [(1, 5, 4, 6), (2, 13, 3, 5), (1, 40, 2, 3), (2, 5, 4, 6), (1, 3, 5, 7), (1, 1, 1, 1), (1, 4, 1, 1), (1, 5, 3, 63),
                    (1, 5, 7, 37)]                # 1295 voxels: six blocks, ragged last
FWD_SHAPES = [(1, 5, 4, 6), (2, 13, 3, 5), (1, 40, 2, 3), (1, 5, 4, 8), (2, 13, 3, 4), (1, 9, 5, 12)]      # test_conv3d_raw's, in its order
FWD_SHAPES += [s for s in FWD_X4_SHAPES + FWD_VOXEL_SHAPES if s not in FWD_SHAPES]


def _fwd_case(path, shape, nf, bias=True, p_off=0, out_off=0):
    name = '%s-%s-nf%d%s%s%s' % (path, _sid(shape), nf, '' if bias else '-nobias', '-p+%d' % p_off if p_off else '',
                                 '-out+%d' % out_off if out_off else '')
    return dict(id=name, shape=shape, nf=nf, bias=bias, p_off=p_off, out_off=out_off, path=path)


def _fwd_cases():
    out = []
    for nf in NFS:
        out += [_fwd_case('x4', s, nf) for s in FWD_X4_SHAPES]
        out += [_fwd_case('voxel', s, nf) for s in FWD_VOXEL_SHAPES]
        out.append(_fwd_case('x4', (2, 13, 3, 4), nf, bias=False))
        out.append(_fwd_case('voxel', (2, 13, 3, 5), nf, bias=False))
        # W % 4 == 0, but a pointer off the 16-byte boundary: the launcher's test is ((p | out) & 15) == 0
        out.append(_fwd_case('voxel', (1, 9, 5, 12), nf, p_off=1))
        out.append(_fwd_case('voxel', (1, 9, 5, 12), nf, out_off=2))
    return out


FWD_CASES = _fwd_cases()
FWD16_SHAPES = [(2, 5, 4, 6)] + [s for s in FWD_VOXEL_SHAPES if s != (2, 5, 4, 6)]      # test_conv3d_h16's shape first
FWD16_CASES = [dict(id='h16-%s-nf%d' % (_sid(s), nf), shape=s, nf=nf) for nf in NFS for s in FWD16_SHAPES]

# data gradient.  run: PNSFM_CONV3D_LEN (None = the launcher's choice); 8 / 4 / 2 run conv3d_dgrad_col_kernel, 3 / 1 conv3d_dgrad_kernel
DGRAD_SHAPES = [(1, 19, 3, 5), (2, 8, 2, 70), (1, 33, 4, 6), (1, 3, 5, 7),
                (1, 4, 1, 1),                     # W = 1: no neighbour on either side
                (1, 9, 1, 62), (1, 9, 2, 62),     # a row is exactly a wave's 62 outputs
                (1, 5, 3, 63), (1, 6, 2, 64),     # rows one and two past it
                (1, 10, 5, 124),                  # run 2: 5 chunks x 620 pixels = 50 waves = 13 blocks (13 % 8 != 0, ragged last block)
                (3, 12, 2, 62)]                   # three images; run 8: a ragged second chunk
DGRAD_RUNS = [8, 4, 2, None, 3, 1]
DGRAD_CASES = [dict(id='dgrad-%s-run%s-nf%d' % (_sid(s), r, nf), shape=s, run=r, nf=nf) for nf in NFS for r in DGRAD_RUNS for s in DGRAD_SHAPES]

# weight / bias gradient.  variant: PNSFM_CONV3D_WGRAD_RING ('34' = conv3d_wgrad_ring_kernel<3, 4>, '0' = conv3d_wgrad_kernel)
WGRAD_SHAPES = [(1, 40, 2, 3), (2, 13, 3, 70), (1, 5, 4, 6), (1, 1, 1, 1), (1, 2, 1, 62), (3, 12, 2, 62), (1, 14, 5, 124)]
WGRAD_VARIANTS = ['0', '34']
WGRAD_CASES = [dict(id='wgrad-%s-ring%s-nf%d' % (_sid(s), v, nf), shape=s, variant=v, nf=nf)
               for nf in NFS for v in WGRAD_VARIANTS for s in WGRAD_SHAPES]

# shuffles.  base (B, C, H, W): the x of space_to_depth.  Per base: space_to_depth of x; depth_to_space of its output (input width
# W / 2); depth_to_space of a [B, 4C, H, W] tensor (input width W); space_to_depth of the channel slices [lo, lo + C) of a C + 3
# channel tensor (B = 2: batch stride > C H W), which are 16-byte aligned whenever W % 8 == 0.  The three paths stated per base:
# space_to_depth, depth_to_space at W / 2, depth_to_space at W.
_SHUFFLE_BASES = [
    ((2, 3, 4, 16), 'v4', 'v4', 'v4'),
    ((1, 5, 6, 8), 'v4', 'v4', 'v4'),
    ((2, 4, 2, 24), 'v4', 'v4', 'v4'),
    ((1, 2, 4, 12), 'scalar-width', 'scalar-width', 'v4'),
    ((3, 1, 2, 4), 'scalar-width', 'scalar-width', 'v4'),
    ((1, 3, 2, 2), 'scalar-width', 'scalar-width', 'scalar-width'),        # the smallest shape
    ((2, 2, 6, 10), 'scalar-width', 'scalar-width', 'scalar-width'),      # neither 16-byte form applies
    ((2, 5, 18, 40), 'v4', 'v4', 'v4'),                                   # 450 thread items: two blocks, ragged
]
SHUFFLE_SHAPES = [b[0] for b in _SHUFFLE_BASES]


def _shuffle_case(base, op, shape, path, dtype='f32', x_off=0, y_off=0, lo=None):
    name = '%s-%s-%s%s%s%s%s' % (op, _sid(shape), path, '' if dtype == 'f32' else '-' + dtype, '-slice%d' % lo if lo is not None else '',
                                 '-x+%d' % x_off if x_off else '', '-y+%d' % y_off if y_off else '')
    return dict(id=name, base=base, op=op, shape=shape, path=path, dtype=dtype, x_off=x_off, y_off=y_off, lo=lo)


def _shuffle_cases():
    out = []
    for base, p_s2d, p_half, p_full in _SHUFFLE_BASES:
        B, C, H, W = base
        out.append(_shuffle_case(base, 's2d', base, p_s2d))
        out.append(_shuffle_case(base, 'd2s', (B, C, H // 2, W // 2), p_half))
        out.append(_shuffle_case(base, 'd2s', base, p_full))
        for lo in (1, 2):
            out.append(_shuffle_case(base, 's2d', base, p_s2d, lo=lo))
        out.append(_shuffle_case(base, 's2d', base, 'h16', dtype='f16'))
        out.append(_shuffle_case(base, 'd2s', base, 'h16', dtype='f16'))
    # shapes of the 16-byte forms with x or y 1 / 3 elements off a 16-byte boundary: the per-element kernels
    for base in ((2, 3, 4, 16), (2, 5, 18, 40)):
        for op in ('s2d', 'd2s'):
            for x_off, y_off in ((1, 0), (3, 0), (0, 1), (0, 3)):
                out.append(_shuffle_case(base, op, base, 'scalar-misaligned', x_off=x_off, y_off=y_off))
    return out


SHUFFLE_CASES = _shuffle_cases()

for _cases in (FWD_CASES, FWD16_CASES, DGRAD_CASES, WGRAD_CASES, SHUFFLE_CASES):
    assert len({c['id'] for c in _cases}) == len(_cases)


def ids(cases):
    return [c['id'] for c in cases]


def select(cases, **want):
    """The cases whose fields equal `want` (the emulated tests keep their parametrisation by shape and pick their cases here)."""
    got = [c for c in cases if all(c[k] == v for k, v in want.items())]
    assert got, want
    return got


# ------------------------------------------------------------------------------------------------ the launcher's conditions, restated
def _ceil_div(a, b):
    return -(-a // b)


def forward_path(W, p_ptr, out_ptr):
    return 'x4' if W % 4 == 0 and (p_ptr | out_ptr) % 16 == 0 else 'voxel'


def shuffle_path(op, W, x_ptr, y_ptr, x_batch_stride):
    """W: the width of the kernel's input.  pnsfm_space_to_depth: W % 8 == 0, both pointers and the batch stride 16-byte; pnsfm_depth_to_space: W % 4 == 0."""
    width_ok = W % (8 if op == 's2d' else 4) == 0
    aligned = (x_ptr | y_ptr) % 16 == 0 and (op == 'd2s' or x_batch_stride % 4 == 0)
    return 'v4' if width_ok and aligned else ('scalar-misaligned' if width_ok else 'scalar-width')


def dgrad_run(shape, run):
    """Planes per thread of pnsfm_conv3d_backward_data (run: PNSFM_CONV3D_LEN or None)."""
    B, D, H, W = shape
    n = min(D, 8)
    while n > 2 and B * _ceil_div(D, n) * H * W < 2 * 256 * 256:
        n = _ceil_div(n, 2)
    return run if run is not None else n


def dgrad_grid(shape, run):
    B, D, H, W = shape
    return _ceil_div(_ceil_div(_ceil_div(D, dgrad_run(shape, run)) * H * W, 62), 4)


def wgrad_run(shape, nf):
    """Planes per thread of pnsfm_conv3d_backward_weight before it is rounded up to whole trips of three."""
    B, D, H, W = shape
    n = D
    while n > 12 and B * (nf // 4) * _ceil_div(D, n) * H * W < 4 * 256 * 256:
        n = _ceil_div(n, 2)
    return n


def _shuffle_buffers(case, device):
    """x and y of a shuffle case: ((whole, slot) of y, the kernel's x, the x torch sees, the batch stride)."""
    B, C, H, W = case['shape']
    dtype = torch.float32 if case['dtype'] == 'f32' else torch.float16
    g = torch.Generator().manual_seed(sum(case['shape']) + (case['lo'] or 0))
    if case['op'] == 's2d':
        Cw = C + 3 if case['lo'] is not None else C
        xin = torch.randn((B, Cw, H, W), generator=g).to(dtype)
        yshape = (B, 4 * C, H // 2, W // 2)
    else:
        xin = torch.randn((B, 4 * C, H, W), generator=g).to(dtype)
        yshape = (B, C, 2 * H, 2 * W)
    _, xs = _slot(xin.shape, device, dtype, case['x_off'])
    xs.copy_(xin)
    stride = C * H * W
    if case['lo'] is not None:
        xs, xin = xs[:, case['lo']:case['lo'] + C], xin[:, case['lo']:case['lo'] + C]
        stride = xs.stride(0) if B > 1 else C * H * W
    return _slot(yshape, device, dtype, case['y_off']), xs, xin, stride


def check_table():
    """What the table promises without running a kernel."""
    shapes = set(FWD_SHAPES + FWD16_SHAPES + DGRAD_SHAPES + WGRAD_SHAPES)
    for B, D, H, W in shapes:
        assert D * H * W <= MAX_VOXELS, (B, D, H, W)
    # forward: the case's width and the alignment of its slots select the form it names; both forms with and without a bias
    for c in FWD_CASES:
        B, D, H, W = c['shape']
        _, p = _slot(c['shape'], 'cpu', offset=c['p_off'])
        _, out = _slot((B, c['nf'] * D, H, W), 'cpu', offset=c['out_off'])
        assert forward_path(W, p.data_ptr(), out.data_ptr()) == c['path'], c['id']
    for nf in NFS:
        assert {(c['path'], c['bias']) for c in FWD_CASES if c['nf'] == nf} == {(p, b) for p in ('x4', 'voxel') for b in (True, False)}
        assert {c['shape'] for c in FWD_CASES if c['nf'] == nf} == set(FWD_SHAPES)
        assert any(c['p_off'] % 4 and c['shape'][3] % 4 == 0 for c in FWD_CASES if c['nf'] == nf)
        assert any(c['out_off'] % 4 and c['shape'][3] % 4 == 0 for c in FWD_CASES if c['nf'] == nf)
    # data gradient: runs on both kernels, and grids that meet every branch of pnsfm_xcd_logical_block
    assert {8, 4, 2} < set(DGRAD_RUNS) and {3, 1, None} < set(DGRAD_RUNS)
    grids = {dgrad_grid(s, r) for s in DGRAD_SHAPES for r in DGRAD_RUNS}
    assert min(grids) < 8 and grids & {8, 16} and {1, 5} <= {g % 8 for g in grids if g > 8}, sorted(grids)
    assert dgrad_grid((1, 10, 5, 124), 2) == 13
    assert any(s[1] < 8 for s in DGRAD_SHAPES) and any(s[1] % r for s in DGRAD_SHAPES for r in (8, 4, 2))      # D < run; ragged last run
    # weight gradient: at most 12 planes per thread (the dw3 bound counts 12 fp32 products), both builds, both feature counts
    for s in set(WGRAD_SHAPES + FWD_SHAPES):
        for nf in NFS:
            assert wgrad_run(s, nf) <= 12, (s, nf)
    assert {(c['variant'], c['nf']) for c in WGRAD_CASES} == {(v, nf) for v in ('0', '34') for nf in NFS}
    # shuffles: the stated path follows from the width and the pointers; every path in both directions
    for c in SHUFFLE_CASES:
        if c['dtype'] != 'f32':
            assert c['path'] == 'h16', c['id']
            continue
        (_, y), xs, _, stride = _shuffle_buffers(c, 'cpu')
        assert shuffle_path(c['op'], c['shape'][3], xs.data_ptr(), y.data_ptr(), stride) == c['path'], c['id']
        if c['lo'] is not None and c['shape'][0] > 1:
            assert stride > c['shape'][1] * c['shape'][2] * c['shape'][3]
    for op in ('s2d', 'd2s'):
        assert {c['path'] for c in SHUFFLE_CASES if c['op'] == op} == {'v4', 'scalar-width', 'scalar-misaligned', 'h16'}, op


# ------------------------------------------------------------------------------------------------ the float64 reference
class _Ref(object):
    pass


@functools.lru_cache(maxsize=None)
def reference(shape, nf):
    """Inputs (finite randn, w3 scaled by 0.3) and the float64 forward and gradients of one (shape, NF), computed once per process
    and never written to.  y_nb / y_nb_mag: without the bias."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(16 * sum(shape) + 97 * W + nf)
    r = _Ref()
    r.p = torch.randn(B, D, H, W, generator=g)
    r.w3 = 0.3 * torch.randn(nf, 1, 3, 3, 3, generator=g)
    r.b3 = torch.randn(nf, generator=g)
    r.dy = torch.randn(B, nf * D, H, W, generator=g)

    def run(p, w3, b3, dy):
        p, w3, b3 = (t.double().requires_grad_(True) for t in (p, w3, b3))
        y_nb = F.conv3d(p.unsqueeze(1), w3, None, padding=1)
        y = (y_nb + b3.view(1, nf, 1, 1, 1)).reshape(B, nf * D, H, W)
        dp, dw, db = torch.autograd.grad(y, (p, w3, b3), dy.double())
        return y.detach(), y_nb.detach().reshape(B, nf * D, H, W), dp, dw, db

    r.y, r.y_nb, r.dp, r.dw, r.db = run(r.p, r.w3, r.b3, r.dy)
    r.y_mag, r.y_nb_mag, r.dp_mag, r.dw_mag, r.db_mag = run(r.p.abs(), r.w3.abs(), r.b3.abs(), r.dy.abs())
    return r


@functools.lru_cache(maxsize=None)
def reference16(shape, nf):
    """fp16 inputs and the float64 forward on those fp16 values (half_cases.conv3d_case's recipe)."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(16 * sum(shape) + 97 * W + nf + 1)
    r = _Ref()
    r.p = HC._rand16((B, D, H, W), g)
    r.w3 = (torch.randn((nf, 1, 3, 3, 3), generator=g) * 0.3).half()
    r.b3 = (torch.randn(nf, generator=g) * 0.1).half()
    r.y = F.conv3d(r.p.double().unsqueeze(1), r.w3.double(), r.b3.double(), padding=1).reshape(B, nf * D, H, W)
    r.y_mag = F.conv3d(r.p.double().abs().unsqueeze(1), r.w3.double().abs(), None, padding=1).reshape(B, nf * D, H, W)
    return r


# ------------------------------------------------------------------------------------------------ the checkers
def _place(t, device, offset=0):
    """t copied into a NaN-guarded flat tensor on `device`, `offset` elements past the guard."""
    _, s = _slot(t.shape, device, t.dtype, offset)
    s.copy_(t)
    return s


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def _ratio(got, want, mag, bound, what):
    """max |got - want| / (u mag) over the elements with mag > 0; asserts |got - want| <= bound u mag on every element (an element
    whose magnitude is 0 -- a tap with no voxel under it -- must be exactly 0)."""
    err = (got.double().cpu() - want).abs()
    tol = bound * U * mag
    bad = err > tol
    pos = mag > 0
    worst = float((err[pos] / (U * mag[pos])).max()) if bool(pos.any()) else 0.0
    assert not bool(bad.any()), '%s: %d of %d elements past %g u mag (worst %.3g u mag)' % (what, int(bad.sum()), err.numel(), bound, worst)
    return worst


def _lib_ops():
    from packnet_sfm.hip import _lib, ops
    return _lib.get(), ops


def run_forward(device, case):
    """One forward case; returns max |y - y64| / (u mag)."""
    lib, ops = _lib_ops()
    B, D, H, W = case['shape']
    nf = case['nf']
    r = reference(case['shape'], nf)
    p, w3 = _place(r.p, device, case['p_off']), _place(r.w3, device)
    b3 = _place(r.b3, device) if case['bias'] else None
    whole, out = _slot((B, nf * D, H, W), device, offset=case['out_off'])
    assert forward_path(W, p.data_ptr(), out.data_ptr()) == case['path']
    rc = lib.pnsfm_conv3d_forward(ops._ptr(p), ops._ptr(w3), ops._ptr(b3), ops._ptr(out), B, D, H, W, nf, ops._stream(out))
    _sync(device)
    assert rc == 0, rc
    _check_slot(whole, out, case['id'])
    e = _ratio(out, r.y if case['bias'] else r.y_nb, r.y_mag if case['bias'] else r.y_nb_mag, FWD_BOUND, case['id'])
    print('%s: |y - y64| <= %.3g u mag' % (case['id'], e))
    return e


def run_forward16(device, case):
    """One fp16 forward case; returns the worst error in units of its tolerance (one fp16 ulp + 2^-18 mag)."""
    lib, ops = _lib_ops()
    B, D, H, W = case['shape']
    nf = case['nf']
    r = reference16(case['shape'], nf)
    p, w3, b3 = _place(r.p, device), _place(r.w3, device), _place(r.b3, device)
    whole, out = _slot((B, nf * D, H, W), device, torch.float16)
    rc = lib.pnsfm_conv3d_forward_h16(ops._ptr(p), ops._ptr(w3), ops._ptr(b3), ops._ptr(out), B, D, H, W, nf, ops._stream(out))
    _sync(device)
    assert rc == 0, rc
    _check_slot(whole, out, case['id'])
    extra = 2.0 ** -18 * r.y_mag
    e = float(((out.double().cpu() - r.y).abs() / (HC.ulp16(r.y) + extra)).max())
    print('%s: |y - y64| <= %.3g (fp16 ulp + 2^-18 mag)' % (case['id'], e))
    HC.assert_close16(out, r.y, extra=extra, what=case['id'])
    return e


def run_dgrad(device, case):
    """One data-gradient case (the caller has set or cleared PNSFM_CONV3D_LEN as the case says); returns max |dp - dp64| / (u mag)."""
    lib, ops = _lib_ops()
    assert os.environ.get('PNSFM_CONV3D_LEN') == (None if case['run'] is None else str(case['run']))
    B, D, H, W = case['shape']
    nf = case['nf']
    r = reference(case['shape'], nf)
    dy, w3 = _place(r.dy, device), _place(r.w3, device)
    outs = []
    for _ in range(2):
        whole, dp = _slot((B, D, H, W), device)
        rc = lib.pnsfm_conv3d_backward_data(ops._ptr(dy), ops._ptr(w3), ops._ptr(dp), B, D, H, W, nf, ops._stream(dp))
        _sync(device)
        assert rc == 0, rc
        _check_slot(whole, dp, case['id'])
        outs.append(dp)
    e = _ratio(outs[0], r.dp, r.dp_mag, dgrad_bound(nf), case['id'])
    print('%s: grid %d  |dp - dp64| <= %.3g u mag' % (case['id'], dgrad_grid(case['shape'], case['run']), e))
    assert torch.equal(outs[0], outs[1]), '%s: two launches differ' % case['id']
    return e


def run_wgrad(device, case):
    """One weight / bias gradient case (the caller has set PNSFM_CONV3D_WGRAD_RING); returns the (dw3, db3) errors in u mag."""
    lib, ops = _lib_ops()
    assert os.environ.get('PNSFM_CONV3D_WGRAD_RING') == case['variant']
    B, D, H, W = case['shape']
    nf = case['nf']
    r = reference(case['shape'], nf)
    p, dy = _place(r.p, device), _place(r.dy, device)
    ws = torch.empty((8 * 28,), dtype=torch.float64, device=device)
    outs = []
    for _ in range(2):
        wdw, dw = _slot((nf, 1, 3, 3, 3), device)
        wdb, db = _slot((nf,), device)
        rc = lib.pnsfm_conv3d_backward_weight(ops._ptr(p), ops._ptr(dy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), B, D, H, W, nf,
                                              ops._stream(dw))
        _sync(device)
        assert rc == 0, rc
        _check_slot(wdw, dw, case['id'] + ' dw3')
        _check_slot(wdb, db, case['id'] + ' db3')
        outs.append((dw, db))
    e_dw = _ratio(outs[0][0], r.dw, r.dw_mag, DW_BOUND, case['id'] + ' dw3')
    e_db = _ratio(outs[0][1], r.db, r.db_mag, DB_BOUND, case['id'] + ' db3')
    print('%s: |dw3 - dw64| <= %.3g u mag  |db3 - db64| <= %.3g u mag' % (case['id'], e_dw, e_db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), '%s: two launches differ' % case['id']
    return e_dw, e_db


def run_shuffle(device, case):
    """One shuffle case: bit-exact against torch, guards intact."""
    lib, ops = _lib_ops()
    B, C, H, W = case['shape']
    (whole, y), xs, xin, stride = _shuffle_buffers(case, device)
    if case['dtype'] == 'f32':
        assert shuffle_path(case['op'], W, xs.data_ptr(), y.data_ptr(), stride) == case['path']
        if case['op'] == 's2d':
            rc = lib.pnsfm_space_to_depth(ops._ptr(xs), ops._ptr(y), B, C, H, W, stride, ops._stream(y))
        else:
            rc = lib.pnsfm_depth_to_space(ops._ptr(xs), ops._ptr(y), B, C, H, W, ops._stream(y))
    elif case['op'] == 's2d':
        rc = lib.pnsfm_space_to_depth_h16(ops._ptr(xs), ops._ptr(y), B, C, H, W, ops._stream(y))
    else:
        rc = lib.pnsfm_depth_to_space_h16(ops._ptr(xs), ops._ptr(y), B, C, H, W, ops._stream(y))
    _sync(device)
    assert rc == 0, rc
    _check_slot(whole, y, case['id'])
    want = F.pixel_unshuffle(xin, 2) if case['op'] == 's2d' else F.pixel_shuffle(xin, 2)
    assert torch.equal(y.cpu(), want), case['id']


def run_rejects(device):
    """The error returns before any launch: -1, nothing written.  (Every buffer is sized for NF = 8, whatever NF is passed.)"""
    lib, ops = _lib_ops()
    for H, W in ((3, 4), (2, 3)):
        x = _place(torch.randn(1, 2, H, W), device)
        whole, y = _slot((8 * H * W,), device)
        assert lib.pnsfm_space_to_depth(ops._ptr(x), ops._ptr(y), 1, 2, H, W, 2 * H * W, ops._stream(y)) == -1
        xh = _place(torch.randn(1, 2, H, W).half(), device)
        wholeh, yh = _slot((8 * H * W,), device, torch.float16)
        assert lib.pnsfm_space_to_depth_h16(ops._ptr(xh), ops._ptr(yh), 1, 2, H, W, ops._stream(yh)) == -1
        _sync(device)
        assert bool(torch.isnan(whole).all()) and bool(torch.isnan(wholeh).all())
    B, D, H, W = 1, 3, 2, 4
    g = torch.Generator().manual_seed(5)
    p, w3, b3 = _place(torch.randn(B, D, H, W, generator=g), device), _place(torch.randn(8, 27, generator=g), device), _place(torch.randn(8, generator=g), device)
    dy = _place(torch.randn(B, 8 * D, H, W, generator=g), device)
    ws = torch.empty((8 * 28,), dtype=torch.float64, device=device)
    for nf in (3, 16, 0):
        wy, y = _slot((B, 8 * D, H, W), device)
        assert lib.pnsfm_conv3d_forward(ops._ptr(p), ops._ptr(w3), ops._ptr(b3), ops._ptr(y), B, D, H, W, nf, ops._stream(y)) == -1
        wyh, yh = _slot((B, 8 * D, H, W), device, torch.float16)
        ph, wh, bh = _place(p.cpu().half(), device), _place(w3.cpu().half(), device), _place(b3.cpu().half(), device)
        assert lib.pnsfm_conv3d_forward_h16(ops._ptr(ph), ops._ptr(wh), ops._ptr(bh), ops._ptr(yh), B, D, H, W, nf, ops._stream(yh)) == -1
        wdp, dp = _slot((B, D, H, W), device)
        assert lib.pnsfm_conv3d_backward_data(ops._ptr(dy), ops._ptr(w3), ops._ptr(dp), B, D, H, W, nf, ops._stream(dp)) == -1
        wdw, dw = _slot((8, 27), device)
        wdb, db = _slot((8,), device)
        assert lib.pnsfm_conv3d_backward_weight(ops._ptr(p), ops._ptr(dy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), B, D, H, W, nf,
                                                ops._stream(dw)) == -1
        _sync(device)
        for whole in (wy, wyh, wdp, wdw, wdb):
            assert bool(torch.isnan(whole).all()), nf


def run_autograd(device, shape, nf):
    """The product's autograd node (functional.conv3d_1to8: forward, data gradient at the launcher's run, weight gradient on the
    default build) against the same float64 reference and bounds; returns the four errors in u mag."""
    from packnet_sfm.hip import functional as HF
    r = reference(shape, nf)
    p, w3, b3 = (t.clone().to(device).requires_grad_(True) for t in (r.p, r.w3, r.b3))
    y = HF.conv3d_1to8(p, w3, b3)
    y.backward(r.dy.to(device))
    what = 'conv3d_1to8 %s nf %d ' % (_sid(shape), nf)
    e = (_ratio(y.detach(), r.y, r.y_mag, FWD_BOUND, what + 'y'), _ratio(p.grad, r.dp, r.dp_mag, dgrad_bound(nf), what + 'dp'),
         _ratio(w3.grad, r.dw, r.dw_mag, DW_BOUND, what + 'dw3'), _ratio(b3.grad, r.db, r.db_mag, DB_BOUND, what + 'db3'))
    print('%sy %.3g  dp %.3g  dw3 %.3g  db3 %.3g (u mag)' % ((what,) + e))
    return e
