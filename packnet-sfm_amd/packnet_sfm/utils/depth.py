"""Depth-map helpers on the training path + the evaluation metrics (API subset of the reference's
packnet_sfm/utils/depth.py).  inv2depth on the loss path is fused into the view-synthesis kernel."""
import torch

from packnet_sfm.utils.image import flip_lr
from packnet_sfm.utils.types import is_seq


def inv2depth(inv_depth):
    if is_seq(inv_depth):
        return [inv2depth(item) for item in inv_depth]
    return 1. / inv_depth.clamp(min=1e-6)


def depth2inv(depth):
    if is_seq(depth):
        return [depth2inv(item) for item in depth]
    inv_depth = 1. / depth.clamp(min=1e-6)
    inv_depth[depth <= 0.] = 0.
    return inv_depth


def inv_depths_normalize(inv_depths):
    """Divide each map by its per-sample spatial mean (clamped at 1e-6)."""
    means = [d.mean(2, True).mean(3, True) for d in inv_depths]
    return [d / m.clamp(min=1e-6) for d, m in zip(inv_depths, means)]


# Evaluation crop of Garg et al. (fractions of the image height / width), used by the KITTI protocol when config.crop == 'garg'
_GARG_ROWS, _GARG_COLS = (0.40810811, 0.99189189), (0.03594771, 0.96405229)

# name -> f(gt, pred) on the 1-D vectors of valid pixels; order = the reference's metric vector
_DEPTH_METRICS = (
    ('abs_rel', lambda g, p: ((g - p).abs() / g).mean()),
    ('sqr_rel', lambda g, p: ((g - p) ** 2 / g).mean()),
    ('rmse', lambda g, p: ((g - p) ** 2).mean().sqrt()),
    ('rmse_log', lambda g, p: ((g.log() - p.log()) ** 2).mean().sqrt()),
    ('a1', lambda g, p: (torch.maximum(g / p, p / g) < 1.25).float().mean()),
    ('a2', lambda g, p: (torch.maximum(g / p, p / g) < 1.25 ** 2).float().mean()),
    ('a3', lambda g, p: (torch.maximum(g / p, p / g) < 1.25 ** 3).float().mean()),
)


def _to_gt_resolution(pred, gt, how):
    """'resize': bilinear (align_corners) to the ground-truth size; 'top-center': paste into a zero map, flush with the
    bottom edge and centred horizontally (predictions made on a top-cropped image)."""
    import torch.nn.functional as funct
    if how == 'resize':
        if tuple(pred.shape[-2:]) == tuple(gt.shape[-2:]):
            return pred
        return funct.interpolate(pred, size=gt.shape[-2:], mode='bilinear', align_corners=True)
    if how != 'top-center':
        raise NotImplementedError('Depth scale function {} not implemented.'.format(how))
    canvas = pred.new_zeros(gt.shape)
    dh, dw = gt.shape[2] - pred.shape[2], (gt.shape[3] - pred.shape[3]) // 2
    canvas[:, :, dh:dh + pred.shape[2], dw:dw + pred.shape[3]] = pred
    return canvas


def compute_depth_metrics(config, gt, pred, use_gt_scale=True):
    """[abs_rel, sqr_rel, rmse, rmse_log, a1, a2, a3], summed over the images that have valid pixels and divided by the
    batch size (the reference's convention, utils/depth.py:258-324).  config: .min_depth, .max_depth, .crop ('' | 'garg')
    and optionally .scale_output ('resize' | 'top-center'); gt, pred: [B,1,H,W] depth maps."""
    B, _, H, W = gt.shape
    pred = _to_gt_resolution(pred, gt, getattr(config, 'scale_output', 'resize'))
    inside = torch.ones((H, W), dtype=torch.bool, device=gt.device)
    if config.crop == 'garg':
        inside.zero_()
        inside[int(_GARG_ROWS[0] * H):int(_GARG_ROWS[1] * H), int(_GARG_COLS[0] * W):int(_GARG_COLS[1] * W)] = True
    totals = torch.zeros(len(_DEPTH_METRICS), dtype=torch.float64)
    for g_img, p_img in zip(gt[:, 0], pred[:, 0]):
        keep = inside & (g_img > config.min_depth) & (g_img < config.max_depth)
        if not bool(keep.any()):
            continue
        g, p = g_img[keep], p_img[keep]
        if use_gt_scale:                                  # median scaling of the (scale-ambiguous) prediction
            p = p * (g.median() / p.median())
        p = p.clamp(config.min_depth, config.max_depth)
        totals += torch.stack([fn(g, p) for _, fn in _DEPTH_METRICS]).double().cpu()
    return (totals / B).type_as(gt)


def crop_window(crop, H, W):
    """(y1, y2, x1, x2): the rows / columns of an H x W ground truth that config.crop keeps ('' | 'garg')."""
    if crop == 'garg':
        return (int(_GARG_ROWS[0] * H), int(_GARG_ROWS[1] * H), int(_GARG_COLS[0] * W), int(_GARG_COLS[1] * W))
    return (0, H, 0, W)


def fuse_inv_depth(inv_depth, inv_depth_hat, method='mean'):
    """Fuse an inverse-depth map and the (already flipped back) map of the mirrored image: 'mean' | 'max' | 'min'."""
    if method == 'mean':
        return 0.5 * (inv_depth + inv_depth_hat)
    if method == 'max':
        return torch.max(inv_depth, inv_depth_hat)
    if method == 'min':
        return torch.min(inv_depth, inv_depth_hat)
    raise ValueError('Unknown post-process method {}'.format(method))


def _on_kernels(*tensors):
    """Device tensors go to the HIP kernels (so do host tensors while the tests run the kernel sources on the emulator)."""
    from packnet_sfm.hip import _lib
    return all(t.is_cuda for t in tensors) or not _lib.REQUIRE_CUDA


def post_process_inv_depth(inv_depth, inv_depth_flipped, method='mean'):
    """Flip-and-fuse post-processing: the left 5 % of the width comes from the flipped prediction, the right 5 % from the plain
    one, linear ramps over the next 5 % on either side, fuse_inv_depth in between.  Device tensors: one kernel launch
    (hip.functional.post_process_inv_depth); CPU tensors: the same formula in torch."""
    if method not in ('mean', 'max', 'min'):
        raise ValueError('Unknown post-process method {}'.format(method))
    if _on_kernels(inv_depth, inv_depth_flipped):
        from packnet_sfm.hip import functional as HF
        return HF.post_process_inv_depth(inv_depth, inv_depth_flipped, method)
    W = inv_depth.shape[3]
    inv_depth_hat = flip_lr(inv_depth_flipped)
    xs = torch.arange(W, device=inv_depth.device, dtype=inv_depth.dtype) / max(W - 1, 1)
    mask = 1.0 - torch.clamp(20. * (xs - 0.05), 0., 1.)
    mask_hat = mask.flip(0)
    return mask_hat * inv_depth + mask * inv_depth_hat + (1.0 - mask - mask_hat) * fuse_inv_depth(inv_depth, inv_depth_hat, method)


def evaluate_depth(config, gt, inv_depth, inv_depth_flipped=None, modes=('', '_pp', '_gt', '_pp_gt'), method='mean'):
    """The reference's ModelWrapper.evaluate_depth after its two network forwards: inv_depth / inv_depth_flipped [B,1,h,w] are the
    predictions for the image and for its mirror image, gt [B,1,H,W] the ground truth.  Returns {'metrics': OrderedDict(mode -> [7]
    tensor like compute_depth_metrics, type_as(gt)), 'inv_depth': the post-processed map (None without inv_depth_flipped)}; a mode
    containing 'pp' scores the post-processed map, one containing 'gt' uses median scaling.
    Device tensors: one post-process launch and one hip.functional.depth_metrics call per mode on the INVERSE depth (inverted per
    tap, resized on the fly): no inv2depth pass, no host sync, the metrics stay on the device.  fp16 maps are scored in fp32
    arithmetic, i.e. as compute_depth_metrics scores their .float() copies.  CPU tensors: the Python functions of this module."""
    from collections import OrderedDict
    if any('pp' in m for m in modes) and inv_depth_flipped is None:
        raise ValueError('evaluate_depth: the post-processed modes need inv_depth_flipped')
    inv_depth_pp = None
    if inv_depth_flipped is not None:
        inv_depth_pp = post_process_inv_depth(inv_depth, inv_depth_flipped, method=method)
    metrics = OrderedDict()
    if _on_kernels(gt, inv_depth):
        from packnet_sfm.hip import functional as HF
        window = crop_window(config.crop, gt.shape[2], gt.shape[3])
        for mode in modes:
            metrics[mode] = HF.depth_metrics(gt, inv_depth_pp if 'pp' in mode else inv_depth, config.min_depth, config.max_depth,
                                             window=window, scale_output=getattr(config, 'scale_output', 'resize'),
                                             use_gt_scale='gt' in mode, pred_is_inverse=True).type_as(gt)
    else:
        depth = inv2depth(inv_depth)
        depth_pp = inv2depth(inv_depth_pp) if inv_depth_pp is not None else None
        for mode in modes:
            metrics[mode] = compute_depth_metrics(config, gt, depth_pp if 'pp' in mode else depth, use_gt_scale='gt' in mode)
    return {'metrics': metrics, 'inv_depth': inv_depth_pp}


# ---- depth output: the picture and the depth file's values (csrc/depth_output.h) ------------------------------------------------
_LUT8_CACHE = {}          # (colormap name, device) -> uint8 [N,3] tensor


def colormap_lut8(colormap, device):
    """uint8 [N,3] on `device`: rint(table * 255) of a matplotlib colormap name (resolved at call time to
    matplotlib.colormaps[name](arange(N))[:, :3]; the device table is cached per (name, device)) or of an [N,3] array / tensor of
    floats in [0, 1]."""
    import numpy as np
    device = torch.device(device)
    if isinstance(colormap, str):
        key = (colormap, device)
        if key not in _LUT8_CACHE:
            import matplotlib
            cmap = matplotlib.colormaps[colormap]
            _LUT8_CACHE[key] = colormap_lut8(cmap(np.arange(cmap.N))[:, :3], device)
        return _LUT8_CACHE[key]
    table = colormap.detach().cpu().numpy() if torch.is_tensor(colormap) else np.asarray(colormap)
    table = table.astype(np.float64)
    if table.ndim != 2 or table.shape[1] != 3 or not 1 <= table.shape[0] <= 256:
        raise ValueError('a colour table must be [N,3] with 1 <= N <= 256, got {}'.format(tuple(table.shape)))
    return torch.from_numpy(np.clip(np.rint(table * 255), 0, 255).astype(np.uint8)).to(device)


def _percentile_f32(values, percentile):
    """np.percentile(values, percentile) of a float32 vector, restated operation by operation in float32 (numpy 2.2, method
    'linear') -- the arithmetic csrc/depth_output.h runs; 0 for an empty vector (np.percentile raises there)."""
    import numpy as np
    f = np.float32
    n = values.size
    if n == 0:
        return f(0)
    s = np.sort(values)
    q = f(percentile) / f(100)
    v = f(n - 1) * q
    k = np.floor(v)
    gamma = v - k
    if v >= f(n - 1):
        lo = hi = s[n - 1]
    elif v < 0:
        lo = hi = s[0]
    else:
        lo, hi = s[int(k)], s[int(k) + 1]
    d = hi - lo
    return lo + d * gamma if gamma < f(0.5) else hi - d * (f(1) - gamma)


def _viz_inv_depth_host(inv, rgb, lut8, normalizer, percentile, filter_zeros, bgr):
    """viz_inv_depth_u8 for CPU tensors: the formula of include/pnsfm.h ("depth output") in numpy, float32 throughout."""
    import numpy as np
    f = np.float32
    x = inv.detach().float().numpy()[:, 0]
    lut = lut8.numpy()
    N = lut.shape[0]
    B, H, W = x.shape
    norms = np.zeros((B,), np.float32)
    index = np.zeros((B, H, W), np.uint8)
    with np.errstate(all='ignore'):
        for b in range(B):
            if normalizer is None:
                norms[b] = _percentile_f32(x[b][x[b] > 0] if filter_zeros else x[b].ravel(), percentile)
                divisor = norms[b] + f(1e-6)
            else:
                norms[b] = f(normalizer)
                divisor = f(float(normalizer) + 1e-6)
            xa = np.clip(x[b] / divisor, f(0), f(1)) * f(N)
            xa[xa == N] = N - 1
            index[b] = xa.astype(np.int64).astype(np.uint8)
    pic = lut[index.astype(np.int64)]
    if rgb is not None:
        frame = np.rint(rgb.detach().float().numpy() * f(255))
        frame = np.clip(frame, 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
        pic = np.concatenate([frame, pic], 1)
    if bgr:
        pic = pic[..., ::-1]
    return torch.from_numpy(np.ascontiguousarray(pic)), torch.from_numpy(index), torch.from_numpy(norms)


def viz_inv_depth_u8(inv_depth, rgb=None, normalizer=None, percentile=95, colormap='plasma', filter_zeros=False, bgr=False,
                     details=False):
    """The reference's viz_inv_depth(...) * 255 as bytes, for a batch: inv_depth [B,1,H,W] (fp32 or fp16) -> uint8 [B,H,W,3]; with
    rgb [B,3,H,W] -> [B,2H,W,3], the frame on top of the picture (what scripts/infer.py concatenates and writes); bgr=True gives the
    channel order cv2.imwrite wants.  normalizer None: each image is divided by its own `percentile` (np.percentile's float32
    result; of its values > 0 with filter_zeros -- an image without one gets 0).  colormap: a matplotlib name or an [N,3] table of
    floats in [0, 1], N <= 256.  The bytes are rint(value * 255), which is what cv2.imwrite stores for the reference's float image.
    Device tensors: hip.functional.viz_inv_depth_u8 (a fixed number of launches, no host sync, the result stays on the device);
    CPU tensors: the same formula in numpy.  details=True -> (out, index uint8 [B,H,W], normalisers fp32 [B])."""
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError('Percentiles must be in the range [0, 100]')
    if inv_depth.dim() != 4 or inv_depth.shape[1] != 1:
        raise ValueError('inv_depth must be [B,1,H,W], got {}'.format(tuple(inv_depth.shape)))
    if rgb is not None and tuple(rgb.shape) != (inv_depth.shape[0], 3) + tuple(inv_depth.shape[2:]):
        raise ValueError('rgb {} does not match inv_depth {}'.format(tuple(rgb.shape), tuple(inv_depth.shape)))
    lut8 = colormap_lut8(colormap, inv_depth.device)
    if _on_kernels(inv_depth) and (rgb is None or _on_kernels(rgb)):
        from packnet_sfm.hip import functional as HF
        res = HF.viz_inv_depth_u8(inv_depth, lut8, rgb=rgb, normalizer=normalizer, percentile=percentile, filter_zeros=filter_zeros,
                                  bgr=bgr, details=details)
    else:
        from packnet_sfm.hip import ops
        ops.viz_inv_depth_check(inv_depth.shape[0], inv_depth.shape[2], inv_depth.shape[3], lut8.shape[0], percentile)
        res = _viz_inv_depth_host(inv_depth, rgb, lut8, normalizer, percentile, filter_zeros, bgr)
        res = res if details else res[0]
    return res


def depth_png16(inv_depth):
    """uint16, inv_depth's shape: the values the reference's write_depth(filename.png, inv2depth(inv_depth)) stores --
    (depth * 256).int() -- saturated at 65535.  Device tensors: one kernel launch; CPU tensors: the same formula in torch."""
    if _on_kernels(inv_depth):
        from packnet_sfm.hip import functional as HF
        return HF.depth_png16(inv_depth)
    return (inv2depth(inv_depth.detach().float()) * 256).int().clamp(max=65535).to(torch.uint16)


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
