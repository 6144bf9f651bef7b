"""Cases of csrc/supervised.hip, csrc/invdepth.hip and the invdepth_act / pose_vec2mat kernels of csrc/elementwise.hip, shared by the
emulated CPU tests (tests/test_sup_head_pose_emulated.py) and the GPU tests (tests/test_gpu_sup_head_pose.py).  Every kernel is called
through its packnet_sfm.hip.ops entry point and compared PER ELEMENT with the functions of oracle/packnet_oracle.py run on float64
tensors (supervised_loss with num_scales = 1, inv_depth_head, pose_vec2mat44; gradients from autograd on them; the head's backward
against float64 conv2d autograd).  Every input is a float32 tensor converted exactly, so kernel and oracle see the same numbers.  No
comparison has an outlier allowance.  The layout is that of tests/loss_cases.py.

Supervised loss (five methods, sparse and dense, upstream gradient 1 and 0.37).  Flat sizes 1; 255, 256, 257 (a block, its edge, a
one-pixel second block); 65 537 (257 blocks: the partial-max loop of sup_block_max_of_partials wraps, thread 0 reads slots 0 and 256);
262 145 (1024 blocks after the cap, block 0 alone strides once more); 599 379 (every thread strides, some three times).  256 has no
odd factorisation; every other size has a 4-D shape with odd sides.  Edge kinds: a wholly invalid block (BerHu partial -inf), the
BerHu maximum in the last block only (at 65 537 that is slot 256), every d < 0 (c < 0: all pixels quadratic), nothing valid (NaN like
torch.mean of an empty tensor where the oracle returns one -- its BerHu raises on the empty max, so that loss is not asserted --
and d_pred exactly 0).  Compared: the loss, relative, over ALL pixels; d_pred per element -- of the tensor's maximum for l1, mse and
berhu, of |ref| + the median magnitude of the valid pixels for abs_rel and silog (their gradients carry 1 / pred and span two decades;
under a max-normalised measure the small-pred pixels are free); d_pred exactly 0 on gt <= 0 under sparse.
Routing masks, from the float64 oracle ALONE, the share asserted before anything is compared: a pixel is left out of the d_pred
comparison when |d| <= 8 eps32 max(|pred|, |gt|) (the sign of an L1 term), under BerHu also when ||d| - c| <= 1e-5 |c|.  Cap: 0.1 % of
the valid pixels; nothing below 100 valid pixels.  A BerHu case must keep its float64 loss within the scalar tolerance when its
masked pixels change branch (one such pixel moves the loss by ~0.5 / n, so in practice: none near c); SUP_SEEDS holds the seeds,
chosen on the CPU from the oracle alone, at which that holds.
GPU only: the sizes 262 145 and 599 379 (a 1024-block launch takes 8-18 s on the emulator) and, of the 65 537-pixel cases (2-5 s
each there), all but two -- the BerHu maximum in slot 256 and sparse l1 (SUP_EMU_LARGE).

InvDepth head.  Backward: ops.invdepth_conv_backward(x, w, dz) against float64 conv2d autograd with PNSFM_INVDEPTH_BWD_PPT forcing 1,
2 and 16 pixel slices per thread at (2,5,7,9), (1,19,4,70), (1,9,3,171) (HW = 513: at 2 slices the second block's second slice is
wholly inactive and its first holds one live lane) and (3,8,16,16) (HW = 256: every later slice is inactive), and at one slice
(1,64,3,5), which completes the shapes of test_kernels_emulated.test_invdepth_conv_raw: this table is its GPU twin; GPU only and with the
variable unset, (4,128,50,75) and (4,256,100,124), where the launcher's own rule gives 2 and 16 slices (16 partial blocks per channel
group) -- bwd_ppt() restates the rule and the expected value is asserted, so a retuned rule fails here and does not move the cases
back to one slice -- with a bit-identical second launch.  dx and dw of the tensor's maximum, db of sum |dz|.  Forward:
ops.invdepth_conv_forward at the small shapes on the 64-pixel kernel and both strip kernels (PNSFM_INVDEPTH_STRIP = 0, 4, 8), and a
case whose weights are scaled until the logits reach +-30 on both sides, at min_depth 0.5 and 0.1; the error is absolute, in units
of the bound 1 / min_depth.
invdepth_act: n of 1, 257, 70 001, logits in [-30, 30] with the ends and 0 present.  The backward is compared with float64
sigmoid'(x) / min_depth computed from x, NOT from the rounded y the kernel is handed, absolutely against the tensor's maximum: in the
saturated tail 1 - y * min_depth has no relative accuracy in float32 under any implementation (y * min_depth rounds to 1 from
x = 17 on), so a relative measure would test the format and not the kernel.

pose_vec2mat: N of 1, 64, 65, 200 (a block, a second one, a tail); angles uniform in [-pi, pi], and where N allows fifteen rows that
hold 0, +-pi/2, +-pi (the nearest float32) in one angle slot each with the other two random: entries vanish and gradient terms cancel
there.  Forward: absolute per entry (entries are bounded by 1); the translation column and the bottom row bit-exact.  Backward: a
dense random d_mat (bottom row and (i, 3) included); d_vec of the row's maximum, its translation part the exact copy of d_mat[:, i, 3].

Tolerances.  Per family and quantity: the SAME oracle functions run in float32 torch on the same inputs, here on the CPU, their largest
error against float64 over the compared elements (`python tests/sup_head_pose_cases.py` prints them), times four -- the factor covers
another summation order, FMA contraction and the device's expf, logf, sinf, cosf and division.  Constants are split where one family
holds cases of different conditioning (the five supervised methods, small and automatic head shapes, plain and saturated logits),
which is never looser: silog's baseline is thirty times the other methods', the automatic shapes' dw sums 49 600 products.  Never
taken from the kernels; exact-zero and exact-copy assertions stay exact."""
import functools
import math

import torch
import torch.nn.functional as F

from loss_cases import EPS32, SMALL, O, _Ref, _key, _sid, _sync, _to, ids  # noqa: F401

# The measured float32-torch baselines (one thread); the tolerance of a comparison is 4 x its baseline (tol()).
# Supervised loss, per method (l1, mse, abs_rel, berhu, silog): one constant for all would be silog's, whose mean l^2 - 0.85 mean(l)^2
# cancels (at n = 1 it is 0.15 l^2 of a float32 l = log pred - log gt) and whose gradient at a small pred is 1 / pred times the
# rounding of a logarithm.
SUP_LOSS_BASE = dict(l1=1.23e-7, mse=8.66e-8, abs_rel=1.09e-7, berhu=1.37e-7, silog=3.47e-6)       # relative
SUP_DPRED_BASE = dict(l1=5.91e-8, mse=1e-7, berhu=1.29e-7,                                         # of the tensor's max
                      abs_rel=3.87e-7, silog=1.8e-5)                                               # of |ref| + median |ref|
IDC_DX_BASE, IDC_DW_BASE, IDC_DB_BASE = 1.45e-7, 6.85e-7, 1.07e-8              # forced slices, small shapes: of max, of max, of sum |dz|
IDC_DX_AUTO_BASE, IDC_DW_AUTO_BASE, IDC_DB_AUTO_BASE = 1.41e-7, 7.5e-6, 1.95e-8  # the two automatic shapes
IDC_FWD_BASE, IDC_FWD_SAT_BASE = 2.49e-7, 7.94e-7                                # absolute x min_depth
ACT_FWD_BASE, ACT_BWD_BASE = 1.46e-7, 3.02e-7                                    # absolute, of the tensor's max
POSE_FWD_BASE = 1.02e-7            # absolute
POSE_DVEC_BASE = 2.26e-7           # of the row's max
_BASE = dict(idc_dx=IDC_DX_BASE, idc_dw=IDC_DW_BASE, idc_db=IDC_DB_BASE,
             idc_dx_auto=IDC_DX_AUTO_BASE, idc_dw_auto=IDC_DW_AUTO_BASE, idc_db_auto=IDC_DB_AUTO_BASE,
             idc_fwd=IDC_FWD_BASE, idc_fwd_sat=IDC_FWD_SAT_BASE, act_fwd=ACT_FWD_BASE, act_bwd=ACT_BWD_BASE,
             pose_fwd=POSE_FWD_BASE, pose_dvec=POSE_DVEC_BASE)
_BASE.update({'sup_loss_' + m: v for m, v in SUP_LOSS_BASE.items()})
_BASE.update({'sup_dpred_' + m: v for m, v in SUP_DPRED_BASE.items()})


def tol(name):
    return 4.0 * _BASE[name]


# ------------------------------------------------------------------------------------------------ the tables
SUP_METHODS = ('l1', 'mse', 'abs_rel', 'berhu', 'silog')
SUP_MAX_NORMALISED = ('l1', 'mse', 'berhu')
SUP_GOUTS = (1.0, 0.37)
SUP_CAP = 0.001
SUP_SHAPES = [(1, 1, 1, 1), (1, 1, 15, 17), (1, 1, 16, 16), (1, 1, 1, 257), (1, 1, 1, 65537), (1, 1, 185, 1417), (3, 1, 443, 451)]
SUP_EMU_SLOW = 65537               # from this size on a case takes 2-18 s on the emulator, which runs only these two of them
SUP_EMU_LARGE = ('sup-maxlast-65537-berhu-sparse-g1', 'sup-65537-l1-sparse-g1')
# seeds chosen on the CPU, from the oracle alone, so that every case meets its caps (check_sup_case): (shape, sparse, kind) -> seed
SUP_SEEDS = {((1, 1, 185, 1417), True, 'rand'): 3, ((1, 1, 185, 1417), False, 'rand'): 11, ((3, 1, 443, 451), True, 'rand'): 4,
             ((3, 1, 443, 451), False, 'rand'): 68, ((4, 1, 16, 16), True, 'blockinvalid'): 1, ((1, 1, 25, 41), True, 'allneg'): 1}


def _n(shape):
    return int(math.prod(shape))


def _sup_case(shape, method, sparse, gout, kind='rand'):
    return dict(id='sup-%s%d-%s-%s-g%g' % ('' if kind == 'rand' else kind + '-', _n(shape), method, 'sparse' if sparse else 'dense', gout),
                shape=shape, method=method, sparse=sparse, gout=gout, kind=kind)


SUP_CASES = [_sup_case(s, m, sp, g) for s in SUP_SHAPES for m in SUP_METHODS for sp in (True, False) for g in SUP_GOUTS]
SUP_CASES += [_sup_case((4, 1, 16, 16), m, True, 1.0, 'blockinvalid') for m in SUP_METHODS]
SUP_CASES += [_sup_case(s, 'berhu', True, g, 'maxlast') for s, g in (((1, 1, 25, 41), 0.37), ((1, 1, 1, 65537), 1.0))]
SUP_CASES += [_sup_case((1, 1, 25, 41), 'berhu', sp, 0.37, 'allneg') for sp in (True, False)]
SUP_CASES += [_sup_case((1, 1, 1, 257), m, True, 0.37, 'novalid') for m in SUP_METHODS]
SUP_CASES_EMU = [c for c in SUP_CASES if _n(c['shape']) < SUP_EMU_SLOW or c['id'] in SUP_EMU_LARGE]
assert all(any(c['id'] == i for c in SUP_CASES) for i in SUP_EMU_LARGE)

IDC_SHAPES = [(2, 5, 7, 9),        # ragged channel quarters and groups, one block
              (1, 19, 4, 70),      # three channel groups, the last of three channels; a block and a 24-pixel tail
              (1, 9, 3, 171),      # HW = 513
              (3, 8, 16, 16)]      # HW = 256 exactly, one full channel group, three images
IDC_PPTS = (1, 2, 16)
IDC_AUTO = [((4, 128, 50, 75), 2), ((4, 256, 100, 124), 16)]          # (shape, the slices the launcher's rule gives)
IDC_DEEP = (1, 64, 3, 5)           # eight full channel groups on 15 pixels: the third shape of test_invdepth_conv_raw
IDC_BWD_CASES = [dict(id='idc-bwd-%s-ppt%d' % (_sid(s), p), shape=s, ppt=p) for s in IDC_SHAPES for p in IDC_PPTS]
IDC_BWD_CASES += [dict(id='idc-bwd-%s-ppt1' % _sid(IDC_DEEP), shape=IDC_DEEP, ppt=1)]
IDC_BWD_AUTO_CASES = [dict(id='idc-bwd-%s-auto%d' % (_sid(s), p), shape=s, ppt=None, expect=p) for s, p in IDC_AUTO]
IDC_STRIPS = (0, 4, 8)
IDC_MIN_DEPTHS = (0.5, 0.1)
IDC_FWD_CASES = [dict(id='idc-fwd-%s-strip%d' % (_sid(s), r), shape=s, strip=r, min_depth=0.5, sat=False) for s in IDC_SHAPES for r in IDC_STRIPS]
IDC_FWD_CASES += [dict(id='idc-fwd-%s-strip0' % _sid(IDC_DEEP), shape=IDC_DEEP, strip=0, min_depth=0.5, sat=False)]
IDC_FWD_CASES += [dict(id='idc-fwd-sat-%s-strip%d-md%g' % (_sid(s), r, md), shape=s, strip=r, min_depth=md, sat=True)
                  for s, r in (((1, 19, 4, 70), 0), ((1, 9, 3, 171), 4)) for md in IDC_MIN_DEPTHS]
ACT_CASES = [dict(id='act-%d-md%g' % (n, md), n=n, min_depth=md) for n in (1, 257, 70001) for md in IDC_MIN_DEPTHS]

HALF_PI, PI = float(torch.tensor(math.pi / 2, dtype=torch.float32)), float(torch.tensor(math.pi, dtype=torch.float32))
POSE_SPECIAL = (0.0, HALF_PI, -HALF_PI, PI, -PI)
POSE_CASES = [dict(id='pose-%d-%s' % (n, k), N=n, kind=k) for n, k in ((1, 'rand'), (1, 'zero'), (64, 'special'), (65, 'special'), (200, 'special'))]

for _cases in (SUP_CASES, IDC_BWD_CASES, IDC_BWD_AUTO_CASES, IDC_FWD_CASES, ACT_CASES, POSE_CASES):
    assert len({c['id'] for c in _cases}) == len(_cases)


def bwd_ppt(B, C, H, W):
    """The pixel slices per thread pnsfm_invdepth_conv_backward chooses: a copy of the rule in csrc/invdepth.hip (start at 16, halve
    while the grid has fewer than 512 blocks)."""
    ppt = 16
    while ppt > 1 and -(-H * W // (256 * ppt)) * -(-C // 8) * B < 512:
        ppt >>= 1
    return ppt


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ supervised loss
@functools.lru_cache(maxsize=4)
def sup_inputs(shape, sparse, kind):
    """float32 pred in [0.02, 2] and gt = pred * lognormal noise (sigma 0.35); sparse: about 55 % of gt set to 0."""
    n = _n(shape)
    g = torch.Generator().manual_seed(_key(shape, int(sparse), ('rand', 'blockinvalid', 'maxlast', 'allneg', 'novalid').index(kind),
                                           SUP_SEEDS.get((shape, sparse, kind), 0)))
    pred = 0.02 + 1.98 * torch.rand(n, generator=g, dtype=torch.float64)
    z = torch.randn(n, generator=g, dtype=torch.float64)
    if kind == 'allneg':
        gt = pred * torch.exp(0.35 * z.abs() + 0.01)
    else:
        gt = pred * torch.exp(0.35 * z)
    if kind == 'maxlast':           # d <= 0.7 everywhere but on the last pixel, where it is 1.98
        gt = torch.maximum(gt, pred - 0.7)
        pred[-1], gt[-1] = 2.0, 0.02
    pred, gt = pred.float(), gt.float()
    if sparse:
        drop = torch.rand(n, generator=g) < 0.55
        if kind == 'maxlast' or n == 1:
            drop[-1] = False
        if kind == 'blockinvalid':
            drop[256:512] = True
        if kind == 'novalid':
            drop[:] = True
        gt[drop] = 0.0
    return pred.view(shape).contiguous(), gt.view(shape).contiguous()


def _sup_name(method, sparse):
    return ('sparse-' if sparse else 'dense-') + method


def _sup_loss_and_grad(pred, gt, method, sparse, gout):
    pred = pred.clone().requires_grad_(True)
    loss = O.supervised_loss([pred], gt, _sup_name(method, sparse), num_scales=1)
    loss.backward(torch.tensor(gout, dtype=pred.dtype))
    return loss.detach(), pred.grad


def _berhu(d, c, above):
    """BerHuLoss over the differences d with the quadratic branch on `above` (float64)"""
    return float((d.abs().sum() + (d[above] ** 2).sum()) / (d.numel() + int(above.sum())))


@functools.lru_cache(maxsize=4)
def sup_reference(shape, method, sparse, kind):
    """The fp64 oracle of one case at upstream gradient 1: loss, d_pred, the valid pixels and the routing mask."""
    r = _Ref()
    r.inputs = sup_inputs(shape, sparse, kind)
    pred, gt = (t.double() for t in r.inputs)
    r.valid = (gt > 0) if sparse else torch.ones_like(gt, dtype=torch.bool)
    r.nvalid = int(r.valid.sum())
    d = pred - gt
    r.excluded = r.valid & (d.abs() <= 8.0 * EPS32 * torch.maximum(pred.abs(), gt.abs()))
    r.flip = None
    if r.nvalid == 0:
        r.dpred = torch.zeros_like(pred)
        try:
            r.loss = O.supervised_loss([pred], gt, _sup_name(method, sparse), num_scales=1)
        except (RuntimeError, IndexError):        # BerHu: the max of an empty tensor
            r.loss = None
        return r
    r.loss, r.dpred = _sup_loss_and_grad(pred, gt, method, sparse, 1.0)
    if method == 'berhu':
        dv = d[r.valid]
        r.c = 0.2 * float(dv.max())
        nearc = (dv.abs() - r.c).abs() <= 1e-5 * abs(r.c)
        above = dv.abs() > r.c
        assert abs(_berhu(dv, r.c, above) - float(r.loss)) <= 1e-14 * float(r.loss)
        r.flip = abs(_berhu(dv, r.c, above ^ nearc) - _berhu(dv, r.c, above)) / float(r.loss)
        r.quadratic = float(above.double().mean())
        near = torch.zeros_like(r.valid)
        near[r.valid] = nearc
        r.excluded = r.excluded | near
    return r


def check_sup_case(case):
    """What a case promises, from the oracle alone: the cap on the excluded share and what makes it an edge case."""
    shape, method, sparse, kind = case['shape'], case['method'], case['sparse'], case['kind']
    r = sup_reference(shape, method, sparse, kind)
    pred, gt = (t.double() for t in r.inputs)
    n = pred.numel()
    assert float(pred.min()) >= 0.02 and float(pred.max()) <= 2.0
    if kind == 'novalid':
        assert r.nvalid == 0
        return 0.0
    assert r.nvalid >= 1
    if sparse and n >= SMALL and kind == 'rand':
        assert 0.35 <= r.nvalid / n <= 0.55, '%s: %.1f %% valid' % (case['id'], 100.0 * r.nvalid / n)
    if not sparse:
        assert bool((gt > 0).all())
    nex = int(r.excluded.sum())
    if r.nvalid < SMALL:
        assert nex == 0, '%s: %d excluded pixels of %d' % (case['id'], nex, r.nvalid)
    else:
        assert nex <= SUP_CAP * r.nvalid, '%s: the oracle alone excludes %d of %d valid pixels (cap 0.1 %%)' % (case['id'], nex, r.nvalid)
    if r.flip is not None:
        assert r.flip <= tol('sup_loss_berhu'), '%s: the masked pixels move the float64 loss by %.3g' % (case['id'], r.flip)
    flat_gt, d = gt.flatten(), (pred - gt).flatten()
    if kind == 'blockinvalid':
        assert bool((flat_gt[256:512] == 0).all()) and bool((flat_gt[:256] > 0).any()) and bool((flat_gt[512:] > 0).any())
    if kind == 'maxlast':
        last = (n - 1) // 256 * 256
        v = r.valid.flatten()
        assert float(d[:last][v[:last]].max()) <= 0.5 * float(d[last:][v[last:]].max()) and n - last == 1
    if kind == 'allneg':
        assert bool((d[r.valid.flatten()] < 0).all()) and r.c < 0 and r.quadratic == 1.0
    elif method == 'berhu' and r.nvalid >= SMALL:
        assert 0.1 <= r.quadratic <= 0.9, '%s: %.1f %% of the pixels are quadratic' % (case['id'], 100 * r.quadratic)
    return nex / r.nvalid


def _sup_errors(loss, dpred, r, method, goutv):
    """(loss error, relative; d_pred error in the method's measure; the mask of elements past `limit` = tol x scale)"""
    ref = r.dpred * goutv
    keep = r.valid & ~r.excluded
    err = (dpred - ref).abs()
    if method in SUP_MAX_NORMALISED:
        scale = ref.abs().max().expand_as(ref)
    else:
        scale = ref.abs() + ref[r.valid].abs().median()
    e_l = abs(float(loss) - float(r.loss)) / abs(float(r.loss))
    return e_l, float((err / scale)[keep].max()) if bool(keep.any()) else 0.0, err, scale, keep


def run_sup(device, case, baseline=False):
    """One supervised-loss case, forward and backward.  baseline: the oracle in float32 torch in place of the kernels."""
    from packnet_sfm.hip import ops
    shape, method, sparse, kind, gout = case['shape'], case['method'], case['sparse'], case['kind'], case['gout']
    check_sup_case(case)
    r = sup_reference(shape, method, sparse, kind)
    pred, gt = r.inputs
    goutv = _f32(gout)
    name, lname = 'sup_dpred_' + method, 'sup_loss_' + method
    if baseline:
        if r.nvalid == 0:
            return 0.0, 0.0
        loss, dpred = _sup_loss_and_grad(pred, gt, method, sparse, gout)
    else:
        dp, dg = _to(device, pred, gt)
        loss, ws = ops.supervised_loss_forward(dp, dg, ops.SUP_METHODS[method], sparse)
        dpred = ops.supervised_loss_backward(dp, dg, ws, torch.full((1,), gout, dtype=torch.float32, device=device),
                                             ops.SUP_METHODS[method], sparse)
        _sync(device)
        assert tuple(loss.shape) == (1,) and dpred.shape == pred.shape
    loss, dpred = loss.detach().double().cpu().reshape(()), dpred.detach().double().cpu()
    if sparse:
        assert bool((dpred[~r.valid] == 0).all()), case['id'] + ': d_pred not exactly 0 where gt <= 0'
    if r.nvalid == 0:
        print('%s: nothing valid, loss %s (oracle %s)' % (case['id'], float(loss), 'raises' if r.loss is None else float(r.loss)))
        if r.loss is not None:
            assert math.isnan(float(r.loss)) and math.isnan(float(loss)), case['id']
        return 0.0, 0.0
    e_l, e_d, err, scale, keep = _sup_errors(loss, dpred, r, method, goutv)
    print('%s%s: valid %d  excluded %d  loss %.3g  d_pred %.3g (%s)' % (case['id'], ' [float32 torch]' if baseline else '', r.nvalid,
                                                                     int(r.excluded.sum()), e_l, e_d, 'of max' if method in SUP_MAX_NORMALISED else 'of |ref| + median'))
    if baseline:
        return e_l, e_d
    assert bool(torch.isfinite(dpred).all()), case['id']
    assert e_l <= tol(lname), '%s: loss %.9g vs %.9g (%.3g past %.3g)' % (case['id'], float(loss), float(r.loss), e_l, tol(lname))
    bad = (err > tol(name) * scale) & keep
    assert not bool(bad.any()), '%s: %d d_pred values past %.3g (worst %.3g), first %s' % (
        case['id'], int(bad.sum()), tol(name), e_d, bad.nonzero()[0].tolist())
    return e_l, e_d


# ------------------------------------------------------------------------------------------------ InvDepth head
@functools.lru_cache(maxsize=4)
def idc_inputs(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(_key(shape, 7))
    x = torch.randn(B, C, H, W, generator=g)
    w = 0.2 * torch.randn(1, C, 3, 3, generator=g)
    b = torch.randn(1, generator=g)
    dz = torch.randn(B, 1, H, W, generator=g)
    return x, w, b, dz


def _conv_grads(x, w, b, dz):
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    (F.conv2d(x, w, b, padding=1) * dz).sum().backward()
    return x.grad, w.grad, b.grad


@functools.lru_cache(maxsize=2)
def idc_bwd_reference(shape):
    r = _Ref()
    r.inputs = idc_inputs(shape)
    r.dx, r.dw, r.db = _conv_grads(*(t.double() for t in r.inputs))
    r.sum_abs_dz = float(r.inputs[3].double().abs().sum())
    return r


def _idc_bwd_errors(dx, dw, db, r):
    dx, dw, db = (t.detach().double().cpu() for t in (dx, dw, db))
    return ((dx - r.dx).abs() / r.dx.abs().max(), (dw - r.dw).abs() / r.dw.abs().max(), (db - r.db).abs() / r.sum_abs_dz)


def run_idc_bwd(device, case, setenv, delenv, baseline=False):
    """One backward case of the head: dx and dw per element (of the tensor's max), db (of sum |dz|).  setenv / delenv: the caller's
    monkeypatch; ppt None = the launcher's own rule, with the expected value asserted and a bit-identical second launch."""
    from packnet_sfm.hip import ops
    shape, ppt = case['shape'], case['ppt']
    B, C, H, W = shape
    auto = ppt is None
    if auto:
        assert bwd_ppt(*shape) == case['expect'], '%s: the rule gives %d slices per thread' % (case['id'], bwd_ppt(*shape))
        if case['expect'] == 16:
            assert -(-H * W // 4096) * B == 16
    else:
        assert bwd_ppt(*shape) == 1          # what these shapes get without the override
    r = idc_bwd_reference(shape)
    x, w, b, dz = r.inputs
    names = ['idc_%s%s' % (q, '_auto' if auto else '') for q in ('dx', 'dw', 'db')]
    if baseline:
        got = _conv_grads(x, w, b, dz)
    else:
        if auto:
            delenv('PNSFM_INVDEPTH_BWD_PPT', raising=False)
        else:
            setenv('PNSFM_INVDEPTH_BWD_PPT', str(ppt))
        dx_, dw_, dz_ = _to(device, x, w, dz)
        got = ops.invdepth_conv_backward(dx_, dw_, dz_)
        _sync(device)
        if auto:
            again = ops.invdepth_conv_backward(dx_, dw_, dz_)
            _sync(device)
            assert all(torch.equal(a, b_) for a, b_ in zip(got, again)), case['id'] + ': a second launch differs'
        assert got[0].shape == x.shape and got[1].shape == w.shape and got[2].shape == b.shape
    errs = _idc_bwd_errors(*got, r)
    e = tuple(float(v.max()) for v in errs)
    print('%s%s: dx %.3g of max  dw %.3g of max  db %.3g of sum |dz|' % ((case['id'], ' [float32 torch]' if baseline else '') + e))
    if baseline:
        return e
    for v, name, q in zip(errs, names, ('dx', 'dw', 'db')):
        assert bool(torch.isfinite(v).all()), '%s: %s not finite' % (case['id'], q)
        bad = v > tol(name)
        assert not bool(bad.any()), '%s: %d %s values past %.3g (worst %.3g), first %s' % (
            case['id'], int(bad.sum()), q, tol(name), float(v.max()), bad.nonzero()[0].tolist())
    return e


@functools.lru_cache(maxsize=4)
def idc_fwd_reference(shape, sat, min_depth):
    r = _Ref()
    x, w, b, _ = idc_inputs(shape)
    if sat:     # the weights scaled (bias 0) so that the logits pass +30 and -30
        z = F.conv2d(x.double(), w.double(), None, padding=1)
        w = (w.double() * (30.5 / min(float(z.max()), -float(z.min())))).float()
        b = torch.zeros(1)
    r.inputs = (x, w, b)
    sd = {'h.conv1.weight': w.double(), 'h.conv1.bias': b.double()}
    r.y = O.inv_depth_head(x.double(), sd, 'h', min_depth)
    r.z = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    return r


def run_idc_fwd(device, case, setenv, baseline=False):
    """One forward case of the head, per pixel, absolute in units of the bound 1 / min_depth."""
    from packnet_sfm.hip import ops
    shape, strip, md, sat = case['shape'], case['strip'], case['min_depth'], case['sat']
    r = idc_fwd_reference(shape, sat, md)
    x, w, b = r.inputs
    if sat:
        assert float(r.z.max()) >= 30.0 and float(r.z.min()) <= -30.0
        assert float((r.z.abs() < 2).double().mean()) > 0.02          # and some pixels on the slope
    name = 'idc_fwd_sat' if sat else 'idc_fwd'
    if baseline:
        y = O.inv_depth_head(x, {'h.conv1.weight': w, 'h.conv1.bias': b}, 'h', md)
    else:
        setenv('PNSFM_INVDEPTH_STRIP', str(strip))
        y = ops.invdepth_conv_forward(*_to(device, x, w, b), md)
        _sync(device)
        assert y.shape == r.y.shape
    err = (y.detach().double().cpu() - r.y).abs() * md
    e = float(err.max())
    print('%s%s: |y - y64| x min_depth %.3g' % (case['id'], ' [float32 torch]' if baseline else '', e))
    if baseline:
        return e
    assert bool(torch.isfinite(err).all())
    bad = err > tol(name)
    assert not bool(bad.any()), '%s: %d values past %.3g (worst %.3g), first %s' % (case['id'], int(bad.sum()), tol(name), e, bad.nonzero()[0].tolist())
    return e


@functools.lru_cache(maxsize=None)
def act_reference(n, min_depth):
    r = _Ref()
    g = torch.Generator().manual_seed(_key(n, 11))
    x = 60.0 * torch.rand(n, generator=g) - 30.0
    if n > 1:
        x[0], x[1], x[-1] = -30.0, 0.0, 30.0
    else:
        x[0] = 0.75                 # a single element is its own maximum: not in the tail
    dy = torch.randn(n, generator=g)
    r.inputs = (x, dy)
    x64 = x.double()
    s = torch.sigmoid(x64)
    r.y = s / min_depth
    r.dx = dy.double() * s * (1.0 - s) / min_depth          # from x, not from the rounded y
    return r


def run_act(device, case, baseline=False):
    """invdepth_act forward and backward, absolute against the tensor's maximum (see the module docstring for why)."""
    from packnet_sfm.hip import ops
    n, md = case['n'], case['min_depth']
    r = act_reference(n, md)
    x, dy = r.inputs
    if baseline:
        xg = x.clone().requires_grad_(True)
        y = torch.sigmoid(xg) / md
        y.backward(dy)
        dx = xg.grad
    else:
        dxx, ddy = _to(device, x, dy)
        y = ops.invdepth_act_forward(dxx, md)
        dx = ops.invdepth_act_backward(ddy, y, md)
        _sync(device)
    y, dx = y.detach().double().cpu(), dx.detach().double().cpu()
    ef, eb = (y - r.y).abs() / r.y.abs().max(), (dx - r.dx).abs() / r.dx.abs().max()
    e = float(ef.max()), float(eb.max())
    print('%s%s: forward %.3g  backward %.3g of max' % ((case['id'], ' [float32 torch]' if baseline else '') + e))
    if baseline:
        return e
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    for v, name in ((ef, 'act_fwd'), (eb, 'act_bwd')):
        bad = v > tol(name)
        assert not bool(bad.any()), '%s: %d %s values past %.3g (worst %.3g), first %s' % (
            case['id'], int(bad.sum()), name, tol(name), float(v.max()), bad.nonzero()[0].tolist())
    return e


# ------------------------------------------------------------------------------------------------ pose
def _pose_grad(vec, dmat):
    vec = vec.clone().requires_grad_(True)
    mat = O.pose_vec2mat44(vec)
    mat.backward(dmat)
    return mat.detach(), vec.grad


@functools.lru_cache(maxsize=None)
def pose_reference(N, kind):
    r = _Ref()
    g = torch.Generator().manual_seed(_key(N, 13))
    vec = torch.randn(N, 6, generator=g)
    vec[:, 3:] = (2.0 * torch.rand(N, 3, generator=g) - 1.0) * math.pi
    if kind == 'zero':
        vec[:, 3:] = 0.0
    if kind == 'special':
        for slot in range(3):
            for k, v in enumerate(POSE_SPECIAL):
                vec[slot * len(POSE_SPECIAL) + k, 3 + slot] = v
    dmat = torch.randn(N, 4, 4, generator=g)
    r.inputs = (vec.contiguous(), dmat.contiguous())
    r.mat, r.dvec = _pose_grad(vec.double(), dmat.double())
    return r


def run_pose(device, case, baseline=False):
    """pose_vec2mat forward (absolute; translation column and bottom row exact) and backward (of the row's maximum; the translation
    gradient the exact copy of d_mat[:, i, 3])."""
    from packnet_sfm.hip import ops
    N, kind = case['N'], case['kind']
    r = pose_reference(N, kind)
    vec, dmat = r.inputs
    assert float(vec[:, 3:].abs().max()) <= PI and bool((dmat[:, 3] != 0).all()) and bool((dmat[:, :3, 3] != 0).all())
    if kind == 'special':
        assert all(bool((vec[:, 3 + s] == v).any()) for s in range(3) for v in POSE_SPECIAL)
    if baseline:
        mat, dvec = _pose_grad(vec, dmat)
    else:
        dv, dm = _to(device, vec, dmat)
        mat = ops.pose_vec2mat_forward(dv)
        dvec = ops.pose_vec2mat_backward(dv, dm)
        _sync(device)
        assert tuple(mat.shape) == (N, 4, 4) and tuple(dvec.shape) == (N, 6)
    mat, dvec = mat.detach().cpu(), dvec.detach().cpu()
    ef = (mat.double() - r.mat).abs()
    eb = (dvec.double() - r.dvec).abs() / r.dvec.abs().amax(1, keepdim=True)
    e = float(ef.max()), float(eb.max())
    print('%s%s: matrix %.3g absolute  d_vec %.3g of the row max' % ((case['id'], ' [float32 torch]' if baseline else '') + e))
    if baseline:
        return e
    assert torch.equal(mat[:, :3, 3], vec[:, :3]), case['id'] + ': the translation column is no copy'
    assert torch.equal(mat[:, 3], torch.tensor([0., 0., 0., 1.]).expand(N, 4)), case['id'] + ': bottom row'
    assert torch.equal(dvec[:, :3], dmat[:, :3, 3]), case['id'] + ': the translation gradient is no copy of d_mat[:, i, 3]'
    assert bool(torch.isfinite(mat).all()) and bool(torch.isfinite(dvec).all())
    bad = ef > tol('pose_fwd')
    assert not bool(bad.any()), '%s: %d matrix entries past %.3g (worst %.3g), first %s' % (
        case['id'], int(bad.sum()), tol('pose_fwd'), e[0], bad.nonzero()[0].tolist())
    bad = eb > tol('pose_dvec')
    assert not bool(bad.any()), '%s: %d d_vec values past %.3g of the row max (worst %.3g), first %s' % (
        case['id'], int(bad.sum()), tol('pose_dvec'), e[1], bad.nonzero()[0].tolist())
    return e


# ------------------------------------------------------------------------------------------------ the float32-torch baselines
def measure_baselines():
    """Largest error of the oracle functions in float32 torch against float64, per family and quantity, over the compared elements
    of all its cases: the numbers beside the tolerances above."""
    out = {}
    sup = [(c, run_sup('cpu', c, baseline=True)) for c in SUP_CASES]
    for m in SUP_METHODS:
        out['sup_loss_' + m] = max(e[0] for c, e in sup if c['method'] == m)
        out['sup_dpred_' + m] = max(e[1] for c, e in sup if c['method'] == m)
    for suffix, cases in (('', IDC_BWD_CASES), ('_auto', IDC_BWD_AUTO_CASES)):
        es = [run_idc_bwd('cpu', c, None, None, baseline=True) for c in cases]
        out.update({'idc_dx' + suffix: max(e[0] for e in es), 'idc_dw' + suffix: max(e[1] for e in es), 'idc_db' + suffix: max(e[2] for e in es)})
    out['idc_fwd'] = max(run_idc_fwd('cpu', c, None, baseline=True) for c in IDC_FWD_CASES if not c['sat'])
    out['idc_fwd_sat'] = max(run_idc_fwd('cpu', c, None, baseline=True) for c in IDC_FWD_CASES if c['sat'])
    act = [run_act('cpu', c, baseline=True) for c in ACT_CASES]
    out.update(act_fwd=max(e[0] for e in act), act_bwd=max(e[1] for e in act))
    pose = [run_pose('cpu', c, baseline=True) for c in POSE_CASES]
    out.update(pose_fwd=max(e[0] for e in pose), pose_dvec=max(e[1] for e in pose))
    for k, v in out.items():
        print('%-18s baseline %.3g   committed %.3g   tolerance %.3g' % (k, v, _BASE[k], tol(k)))
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    measure_baselines()
