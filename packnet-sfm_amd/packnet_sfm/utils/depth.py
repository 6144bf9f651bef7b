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


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
