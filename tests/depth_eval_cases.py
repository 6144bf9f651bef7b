"""Depth-evaluation cases (csrc/depth_eval.h: flip-and-fuse post-processing, fused depth metrics, utils.depth.evaluate_depth) shared by
the emulated CPU tests (tests/test_depth_eval_emulated.py) and the GPU tests (tests/test_gpu_depth_eval.py).

Inputs come from an integer hash (`uniform`), so they are the same numbers on every machine and need no storage; the reference's own
outputs on them are in tests/golden/eval.pt (written by tools/make_eval_golden.py, which imports the input builders below) and, for
case 1, in tests/golden/slim.pt['host']['metrics'].

Metric cases (each for use_gt_scale False / True):
  1  gt 3x1x40x60, pred 3x1x20x30, crop '' and 'garg', resize                     the slim.pt fixture
  2  gt = pred size 2x1x96x320, pred quantised to 0.25 (long runs of ties)          several blocks per image; even / odd valid counts
  3  gt 2x1x37x53, pred 2x1x19x27, resize, min_depth 1, max_depth 50               odd sizes, both clamp bounds active
  4  gt 2x1x40x60, pred 2x1x32x48, top-center, min_depth 1e-3, max_depth 80        paste; a strip of valid pixels outside the window
  5  case 3 in fp16 storage                                                        expected: the Python function on .float() inputs

Tolerances.  abs_rel .. rmse_log: 1e-5 relative (what tests/test_host_plumbing.py::test_depth_metrics grants compute_depth_metrics
against the reference).  a1..a3 are counts / n: they must agree to 1e-6 absolute PROVIDED no valid pixel's ratio max(g/p, p/g),
recomputed in float64, lies within 1e-4 relative of a threshold (a one-ulp difference in the scale ratio or in the resize may move
such a pixel either way); every case built here ASSERTS that proviso.  The inputs are built for it: `settle` invalidates (gt := 0) the
few ground-truth pixels whose ratio comes within 2e-4 of a threshold for any of the predictions and scale modes of the case.  Case 1's
data is fixed by the slim.pt fixture and does have such pixels (no seed to pick): there, and only there, a1..a3 are granted exactly
what those pixels can move them by -- (their number) / n per image, / B -- on top of the 1e-6.

Medians.  functional.depth_metrics(details=True) returns the two medians of every image from the head of the kernel workspace
(include/pnsfm.h) and `sampled`, a dump of the prediction the kernels saw at every ground-truth pixel.  For cases 2 and 3 both medians
must equal torch.median of the valid ground truth / of the valid `sampled` values bit for bit (case 2 has no resize: there `sampled`
must also equal the prediction itself bit for bit)."""
import functools
import types

import torch

import parity_cases as P
from packnet_sfm.hip import functional as HF
from packnet_sfm.utils import depth as D

THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)


def uniform(shape, seed):
    """float64 in [0, 1) from an integer hash of (element index, seed): exact integer arithmetic, identical on every machine."""
    n = 1
    for s in shape:
        n *= s
    h = (torch.arange(n, dtype=torch.int64) + 1 + 7919 * seed) * 2654435761 % (1 << 32)
    h = h ^ (h >> 15)
    h = h * 2246822519 % (1 << 32)
    h = h ^ (h >> 13)
    h = h * 3266489917 % (1 << 32)
    h = h ^ (h >> 16)
    return (h.double() / float(1 << 32)).reshape(shape)


def cfg(crop='', min_depth=0.0, max_depth=80.0, scale_output='resize'):
    return types.SimpleNamespace(crop=crop, min_depth=min_depth, max_depth=max_depth, scale_output=scale_output)


# ----------------------------------------------------------------------------------------------- float64 recomputation
def valid_mask(c, gt):
    """[B,H,W] bool: the validity rule of compute_depth_metrics."""
    B, _, H, W = gt.shape
    y1, y2, x1, x2 = D.crop_window(c.crop, H, W)
    inside = torch.zeros((H, W), dtype=torch.bool)
    inside[y1:y2, x1:x2] = True
    g = gt[:, 0].float()
    return inside & (g > c.min_depth) & (g < c.max_depth)


def ratios64(c, gt, pred, use_gt_scale):
    """Per image: (float64 ratios max(g/p, p/g) of the valid pixels, the fp32 medians (gt, pred) or None); CPU, fp32 inputs."""
    p_full = D._to_gt_resolution(pred, gt, c.scale_output)
    keep = valid_mask(c, gt)
    out = []
    for b in range(gt.shape[0]):
        g, p = gt[b, 0][keep[b]], p_full[b, 0][keep[b]]
        med = None
        g64, p64 = g.double(), p.double()
        if g.numel() and use_gt_scale:
            med = (g.median(), p.median())
            p64 = p64 * (med[0] / med[1]).double()
        p64 = p64.clamp(c.min_depth, c.max_depth)
        out.append((torch.maximum(g64 / p64, p64 / g64), med))
    return out


def near_threshold(r, margin):
    bad = torch.zeros_like(r, dtype=torch.bool)
    for t in THRESHOLDS:
        bad |= (r / t - 1).abs() <= margin
    return bad


def settle(c, gt, preds, parity=None):
    """gt with the pixels invalidated (:= 0) whose ratio lies within 2e-4 of a threshold for any prediction in `preds`, with or
    without median scaling (repeated until none is left: removing a pixel can move a median); parity: per image, the wanted
    valid count modulo 2 (one more pixel is dropped where it differs)."""
    gt = gt.clone()
    for _ in range(50):
        changed = False
        for pred in preds:
            for ugs in (False, True):
                keep = valid_mask(c, gt)
                for b, (r, _) in enumerate(ratios64(c, gt, pred, ugs)):
                    bad = near_threshold(r, 2e-4)
                    if bad.any():
                        gt[b, 0].view(-1)[keep[b].flatten().nonzero()[:, 0][bad]] = 0.0
                        changed = True
        keep = valid_mask(c, gt)
        if parity is not None:
            for b, want in enumerate(parity):
                if int(keep[b].sum()) % 2 != want:
                    gt[b, 0].view(-1)[keep[b].flatten().nonzero()[0, 0]] = 0.0
                    changed = True
        if not changed:
            return gt
    raise AssertionError('settle did not converge')


# ----------------------------------------------------------------------------------------------- inputs
def _sparse_gt(shape, seed, lo=10.0, hi=80.0):
    gt = (hi * uniform(shape, seed)).float()
    gt[gt < lo] = 0
    return gt


@functools.lru_cache(maxsize=None)
def metric_inputs(case):
    """(gt, pred, [configs]) on the CPU; case 5's tensors are fp16."""
    if case == 1:
        fx = P.golden('slim')['host']['metrics']
        return fx['gt'], fx['pred'], [cfg(''), cfg('garg')]
    if case == 2:
        c = cfg('', 1e-3, 80.0)
        pred = (torch.round((2 + 40 * uniform((2, 1, 96, 320), 21)) * 4) / 4).float()
        gt = (torch.round(_sparse_gt((2, 1, 96, 320), 22, lo=8.0, hi=60.0).double() * 8) / 8).float()
        return settle(c, gt, [pred], parity=(0, 1)), pred, [c]
    if case in (3, 5):
        c = cfg('', 1.0, 50.0)
        pred = (0.5 + 70 * uniform((2, 1, 19, 27), 31)).float()
        gt = _sparse_gt((2, 1, 37, 53), 32, lo=0.9, hi=60.0)
        if case == 5:
            pred, gt = pred.half().float(), gt.half().float()
        gt = settle(c, gt, [pred])
        return (gt.half(), pred.half(), [c]) if case == 5 else (gt, pred, [c])
    if case == 4:
        c = cfg('', 1e-3, 80.0, 'top-center')
        pred = (3 + 60 * uniform((2, 1, 32, 48), 41)).float()
        gt = _sparse_gt((2, 1, 40, 60), 42, lo=5.0, hi=90.0)
        gt[:, :, :8] = 0              # the pasted window is rows 8..39, columns 6..53 ...
        gt[:, :, :, :4] = 0           # ... columns 4, 5 stay: a strip of valid pixels where the pasted prediction is 0
        gt[:, :, :, 54:] = 0
        return settle(c, gt, [pred]), pred, [c]
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def evaluate_inputs():
    """(config, gt 2x1x37x53, inv_depth, inv_depth_flipped 2x1x19x27) for the evaluate_depth case."""
    c = cfg('', 1.0, 50.0)
    inv = (1.0 / (0.5 + 70 * uniform((2, 1, 19, 27), 51))).float()
    inv_f = (1.0 / (0.5 + 70 * uniform((2, 1, 19, 27), 52))).float()
    gt = _sparse_gt((2, 1, 37, 53), 53, lo=0.9, hi=60.0)
    return c, settle(c, gt, [D.inv2depth(inv), D.inv2depth(pp_formula(inv, inv_f, 'mean').float())]), inv, inv_f


def checksum(*tensors):
    """Sum of the bit patterns: exact, whatever the summation order."""
    return [int(t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).long().sum()) for t in tensors]


# ----------------------------------------------------------------------------------------------- checks
def rel_close(got, want, tol, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = (got - want).abs() / want.abs().clamp(min=1e-30)
    assert bool((err <= tol).all()), '%s: got %s, expected %s (relative error %s > %g)' % (what, got.tolist(), want.tolist(), err.tolist(), tol)


def metrics_close(got, want, what, slack=(0.0, 0.0, 0.0)):
    rel_close(got[:4], want[:4], 1e-5, what + ' abs_rel..rmse_log')
    d = (got[4:].double().cpu() - want[4:].double().cpu()).abs()
    assert bool((d <= 1e-6 + torch.tensor(slack, dtype=torch.float64)).all()), '%s a1..a3: got %s, expected %s' % (what, got[4:].tolist(), want[4:].tolist())


def assert_margin(c, gt, pred, use_gt_scale, what, fixed_data=False):
    """The proviso of the a1..a3 comparison; returns per image (n, [count below each threshold], [pixels within 1e-4 of each
    threshold]) from the float64 ratios.  The third entry is all zeros -- asserted -- except for fixed_data (case 1)."""
    counts = []
    for b, (r, _) in enumerate(ratios64(c, gt.float(), pred.float(), use_gt_scale)):
        near = [int(((r / t - 1).abs() <= 1e-4).sum()) for t in THRESHOLDS]
        assert fixed_data or near == [0, 0, 0], '%s: image %d has a pixel within 1e-4 of a threshold' % (what, b)
        counts.append((r.numel(), [int((r < t).sum()) for t in THRESHOLDS], near))
    return counts


def a_slack(counts):
    """What the pixels within 1e-4 of a threshold can move a1..a3 of the batch by: each of them 1 / n of its image, / B."""
    return tuple(sum(near[k] / max(n, 1) for n, _, near in counts) / len(counts) for k in range(3))


def reference_metrics(case, crop, use_gt_scale):
    if case == 1:
        return P.golden('slim')['host']['metrics']['values'][(crop, use_gt_scale)]
    fx = P.golden('eval')
    gt, pred, _ = metric_inputs(case)
    assert checksum(gt, pred) == fx['checksums'][case], 'inputs of case %d differ from those the fixture was recorded on' % case
    return fx['metrics'][(case, use_gt_scale)]


def metric_case(dev, case, use_gt_scale):
    gt, pred, configs = metric_inputs(case)
    for c in configs:
        what = 'case %d crop=%r use_gt_scale=%s' % (case, c.crop, use_gt_scale)
        counts = assert_margin(c, gt, pred, use_gt_scale, what, fixed_data=case == 1)
        slack = a_slack(counts)
        g, p = gt.to(dev), pred.to(dev)
        H, W = gt.shape[2:]
        m, rows, med, sampled = HF.depth_metrics(g, p, c.min_depth, c.max_depth, window=D.crop_window(c.crop, H, W),
                                                 scale_output=c.scale_output, use_gt_scale=use_gt_scale, details=True)
        assert m.dtype == torch.float32 and m.device == g.device and tuple(m.shape) == (7,) and tuple(rows.shape) == (gt.shape[0], 8)
        ref = reference_metrics(case, c.crop, use_gt_scale)
        assert bool(torch.isfinite(ref).all()), what
        metrics_close(m, ref, what + ' vs the reference', slack)
        ours = D.compute_depth_metrics(c, g.float(), p.float(), use_gt_scale)           # the Python function, same device
        metrics_close(m, ours, what + ' vs compute_depth_metrics', slack)
        # per-image rows: count, and a1..a3 * n against the integer counts of the float64 recomputation, exactly
        rows_c = rows.double().cpu()
        for b, (n, below, near) in enumerate(counts):
            assert rows_c[b, 7] == n, '%s image %d: %g valid pixels, expected %d' % (what, b, rows_c[b, 7], n)
            off = [abs(int(torch.round(rows_c[b, 4 + k] * n)) - below[k]) for k in range(3)]
            assert all(o <= nr for o, nr in zip(off, near)), (what, b, rows_c[b].tolist(), below, near)
        rel_close(m, rows_c[:, :7].sum(0) / gt.shape[0], 1e-6, what + ' metrics vs the sum of the rows / B')
        # the sampled prediction, then the medians
        want = D._to_gt_resolution(pred.float(), gt.float(), c.scale_output)
        if tuple(pred.shape) == tuple(gt.shape):
            assert torch.equal(sampled.cpu(), want), what + ': sampled prediction of an identical-size pair'
        else:
            P.check(sampled, want, 2e-6, what + ' sampled prediction')
        if use_gt_scale and case in (2, 3):
            keep = valid_mask(c, gt.float())
            for b in range(gt.shape[0]):
                mg, mp = gt[b, 0].float()[keep[b]].median(), sampled[b, 0].cpu()[keep[b]].median()
                assert torch.equal(med[b].cpu().view(torch.int32), torch.stack([mg, mp]).view(torch.int32)), \
                    '%s image %d: medians %s, torch.median %s' % (what, b, med[b].tolist(), [float(mg), float(mp)])
        if not use_gt_scale:
            assert med is None
        if case == 2:
            assert [cnt[0] % 2 for cnt in counts] == [0, 1], 'case 2 wants an even and an odd valid count'
    return m, rows


def empty_image_case(dev):
    """A batch whose middle image has no valid pixel: the sum over the other two, divided by 3; its row: count 0, metrics 0."""
    gt, pred, configs = metric_inputs(1)
    gt = gt.clone()
    gt[1] = 0
    c = configs[0]
    for ugs in (False, True):
        m, rows = HF.depth_metrics(gt.to(dev), pred.to(dev), c.min_depth, c.max_depth, use_gt_scale=ugs, details=True)[:2]
        assert bool((rows[1] == 0).all()), rows[1].tolist()
        assert bool((rows[0, 7] > 0) & (rows[2, 7] > 0))
        rel_close(m, (rows[0, :7].double() + rows[2, :7].double()) / 3, 1e-6, 'empty middle image: (row 0 + row 2) / 3')
        pair = torch.stack([gt[0], gt[2]]), torch.stack([pred[0], pred[2]])
        two = HF.depth_metrics(pair[0].to(dev), pair[1].to(dev), c.min_depth, c.max_depth, use_gt_scale=ugs)
        rel_close(m, two.double() * 2 / 3, 1e-6, 'empty middle image vs the two-image batch')
        want = D.compute_depth_metrics(c, gt, pred, ugs)
        assert bool(torch.isfinite(want).all())
        rel_close(m[:4], want[:4], 1e-5, 'empty middle image vs compute_depth_metrics')


def inverse_case(dev):
    """pred_is_inverse: every tap inverted BEFORE the resize == compute_depth_metrics on inv2depth(inv)."""
    c, gt, inv, _ = evaluate_inputs()
    for ugs in (False, True):
        assert_margin(c, gt, D.inv2depth(inv), ugs, 'inverse')
        m = HF.depth_metrics(gt.to(dev), inv.to(dev), c.min_depth, c.max_depth, use_gt_scale=ugs, pred_is_inverse=True)
        metrics_close(m, D.compute_depth_metrics(c, gt, D.inv2depth(inv), ugs), 'pred_is_inverse use_gt_scale=%s' % ugs)


# ----------------------------------------------------------------------------------------------- post-process
def pp_formula(inv, inv_flipped, method, dtype=None):
    """The formula of include/pnsfm.h in torch, in `dtype` (default: the inputs')."""
    a, ah = inv.to(dtype or inv.dtype), inv_flipped.to(dtype or inv.dtype).flip(3)
    W = a.shape[3]
    xs = torch.arange(W, dtype=a.dtype, device=a.device) / max(W - 1, 1)
    mask = 1.0 - torch.clamp(20. * (xs - 0.05), 0., 1.)
    mask_hat = mask.flip(0)
    fuse = {'mean': lambda: 0.5 * (a + ah), 'max': lambda: torch.max(a, ah), 'min': lambda: torch.min(a, ah)}[method]()
    return mask_hat * a + mask * ah + (1.0 - mask - mask_hat) * fuse


def pp_inputs(W=64, seed=61):
    return (0.02 + 0.5 * uniform((2, 1, 8, W), seed)).float(), (0.02 + 0.5 * uniform((2, 1, 8, W), seed + 1)).float()


def pp_reference_case(dev, method, fn):
    """fn(inv, inv_flipped, method) against the reference's recorded output: 1e-5 relative, fp32."""
    fx = P.golden('eval')['post_process']
    inv, inv_f = pp_inputs()
    assert torch.equal(inv, fx['inv_depth']) and torch.equal(inv_f, fx['inv_depth_flipped'])
    out = fn(inv.to(dev), inv_f.to(dev), method)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(inv.shape)
    rel_close(out, fx['out'][method], 1e-5, 'post_process_inv_depth %s' % method)


def pp_half_case(dev, method, W):
    """fp16 storage against the float64 formula on the same fp16 values: one fp16 rounding (2^-11 relative) + the fp32 tolerance."""
    inv, inv_f = (t.half() for t in pp_inputs(W, 63))
    out = HF.post_process_inv_depth(inv.to(dev), inv_f.to(dev), method)
    assert out.dtype == torch.float16
    want = pp_formula(inv, inv_f, method, torch.float64)
    err = (out.double().cpu() - want).abs()
    assert bool((err <= (2.0 ** -11 + 1e-5) * want.abs()).all()), 'post_process fp16 %s W=%d: worst %g' % (method, W, float((err / want.abs()).max()))
    mixed = HF.post_process_inv_depth(inv.float().to(dev), inv_f.to(dev), method)     # a dtype flag per tensor: fp32 map, fp16 flipped map
    assert mixed.dtype == torch.float32
    rel_close(mixed, want, 1e-5, 'post_process fp32 / fp16 %s' % method)


def pp_symmetry_case(dev, W):
    """Mirror symmetry, exact: post_process(a, b) is the mirror image of post_process(b, a) (the masks are one function of x and of
    W-1-x), so post_process(a, a) -- the pair (a, flip(a)) of the formula's own a / a^ -- equals its own mirror image."""
    a, b = pp_inputs(W, 65)
    a, b = a.to(dev), b.to(dev)
    for method in ('mean', 'max', 'min'):
        assert torch.equal(HF.post_process_inv_depth(a, b, method).flip(3), HF.post_process_inv_depth(b, a, method)), (method, W)
    out = HF.post_process_inv_depth(a, a, 'mean')
    assert torch.equal(out, out.flip(3)), W
    s = 0.5 * (a + a.flip(3))                  # a symmetric map and its flip
    out = HF.post_process_inv_depth(s, s.flip(3), 'mean')
    assert torch.equal(out, out.flip(3)), W


def pp_errors_case(dev):
    a, b = (t.to(dev) for t in pp_inputs())
    import pytest
    with pytest.raises(ValueError):
        HF.post_process_inv_depth(a, b, 'median')
    with pytest.raises(ValueError):
        D.post_process_inv_depth(a, b, 'median')
    with pytest.raises(ValueError):
        D.fuse_inv_depth(a, b, 'median')
    for dt in (torch.float32, torch.float16):          # forward only, both dtypes
        x = a.to(dt).requires_grad_(True)
        out = HF.post_process_inv_depth(x, b.to(dt), 'mean')
        with pytest.raises(NotImplementedError):
            out.float().sum().backward()
    with pytest.raises(RuntimeError):
        HF.post_process_inv_depth(a, b[:, :, :4], 'mean')
    with pytest.raises(RuntimeError):               # top-center with a prediction larger than the ground truth: the library's error code
        HF.depth_metrics(a, torch.cat([b, b], 2), 0.0, 80.0, scale_output='top-center')


# ----------------------------------------------------------------------------------------------- evaluate_depth
def evaluate_case(dev):
    c, gt, inv, inv_f = evaluate_inputs()
    depth, inv_pp = D.inv2depth(inv), pp_formula(inv, inv_f, 'mean')
    depth_pp = D.inv2depth(inv_pp)
    res = D.evaluate_depth(c, gt.to(dev), inv.to(dev), inv_f.to(dev))
    assert list(res['metrics']) == ['', '_pp', '_gt', '_pp_gt']
    assert torch.equal(res['inv_depth'], D.post_process_inv_depth(inv.to(dev), inv_f.to(dev), 'mean'))
    rel_close(res['inv_depth'], inv_pp, 1e-5, 'evaluate_depth inv_depth')
    for mode, m in res['metrics'].items():
        pred, ugs = (depth_pp if 'pp' in mode else depth), 'gt' in mode
        assert_margin(c, gt, pred, ugs, 'evaluate_depth %r' % mode)
        assert m.dtype == gt.dtype and m.device == res['inv_depth'].device
        metrics_close(m, D.compute_depth_metrics(c, gt, pred, use_gt_scale=ugs), 'evaluate_depth mode %r' % mode)
    plain = D.evaluate_depth(c, gt.to(dev), inv.to(dev), modes=('', '_gt'))
    assert plain['inv_depth'] is None and torch.equal(plain['metrics']['_gt'], res['metrics']['_gt'])
    import pytest
    with pytest.raises(ValueError):
        D.evaluate_depth(c, gt.to(dev), inv.to(dev))
