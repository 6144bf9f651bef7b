"""Training input pipeline on the device: resize (Lanczos) -> duplicate -> colour jitter -> ToTensor, for a BATCH of decoded
uint8 frames that already sit in HBM.

Drop-in for what `train_transforms` (reference packnet_sfm/datasets/transforms.py:11-41) does per sample on the host with
PIL / torchvision (datasets/augmentations.py: resize_sample :101-180, duplicate_sample :228-252, colorjitter_sample /
random_color_jitter_transform :254-337, to_tensor_sample :185-226): same keys in, same keys out ('rgb', 'rgb_context',
'rgb_original', 'rgb_context_original', 'intrinsics'), same random draws from Python's `random` in the same order (one
`random.random()` for the jitter probability, four `random.uniform` factors, one `random.shuffle` of the four operations per
sample), and BIT-IDENTICAL pixels: the kernels of csrc/augment.hip restate Pillow's integer arithmetic (tests pin them against
PIL itself).  The frames of a batch share one launch per stage; crop borders are index arithmetic on the uint8 tensor.

Depth maps ('depth', 'input_depth', 'depth_context': fp32 on the device) follow the images: the same crop window (crop_sample,
augmentations.py:402-505), then resize_depth_preserve (:56-98) as a gather kernel that is bit-identical to the reference's numpy
scatter (csrc/depth_input.h; tests pin it against the reference's own outputs), fp32 [B,1,H,W] out; all maps of one source size
share one launch and the crop is the kernel's window, not a copy.  'input_depth_context' is passed through untouched.

DeviceEvalTransform is the counterpart of `validation_transforms` / `test_transforms` (transforms.py:41-93) and
get_device_transforms of `get_transforms` (:95-132).  The 'test' mode resizes 'input_depth' with the nearest rule of
cv2.resize(..., INTER_NEAREST) as restated in include/pnsfm.h; OpenCV is not available where this package is tested, so that one
rule is NOT pinned against the real library.

Not covered (the reference's host path stays available through the merged package): 'input_depth_context', ragged batches
(frames of different sizes in one call), the optional 3x4 'color' matrix of `jittering[4]`, PIL images as input.
"""
import math
import random
import struct

import numpy as np
import torch

from packnet_sfm.hip import ops
from packnet_sfm.utils.misc import parse_crop_borders

_PRECISION_BITS = 32 - 8 - 2          # libImaging/Resample.c


def _lanczos(x):
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    if -3.0 <= x < 3.0:
        return sinc(x) * sinc(x / 3)
    return 0.0


_COEFF_CACHE = {}


def lanczos_coefficients(in_size, out_size):
    """(kk int32 [out, ksize], bounds int32 [out, 2]) exactly as Pillow's precompute_coeffs + normalize_coeffs_8bpc compute
    them for Image.resize(..., Image.LANCZOS) without a box (libImaging/Resample.c)."""
    key = (in_size, out_size)
    if key in _COEFF_CACHE:
        return _COEFF_CACHE[key]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << _PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << _PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    _COEFF_CACHE[key] = (kk, bounds)
    return kk, bounds


def resize_frames(frames, shape):
    """frames: uint8 [N, H, W, 3] on the device -> uint8 [N, shape[0], shape[1], 3]; == PIL's img.resize((W, H), LANCZOS) per
    frame (horizontal pass, then vertical pass)."""
    N, H, W, _ = frames.shape
    oH, oW = shape
    out = frames.contiguous()
    if W != oW:
        kk, bounds = lanczos_coefficients(W, oW)
        out = ops.resample8(out, torch.from_numpy(kk).to(out.device), torch.from_numpy(bounds).to(out.device), oW, axis=1)
    if H != oH:
        kk, bounds = lanczos_coefficients(H, oH)
        out = ops.resample8(out, torch.from_numpy(kk).to(out.device), torch.from_numpy(bounds).to(out.device), oH, axis=0)
    return out


def draw_jitter(parameters, prob=1.0):
    """One sample's colour-jitter decision, consuming Python's RNG exactly like colorjitter_sample +
    random_color_jitter_transform (augmentations.py:254-337) -> packed 56-byte record for the kernel (order, four factors, hue, enable flag, 3-entry colour scale: include/pnsfm.h)."""
    if not (random.random() < prob):
        return ops.jitter_record()
    brightness, contrast, saturation, hue = parameters[:4]
    factors = [random.uniform(max(0, 1 - brightness), 1 + brightness),
               random.uniform(max(0, 1 - contrast), 1 + contrast),
               random.uniform(max(0, 1 - saturation), 1 + saturation),
               random.uniform(-hue, hue)]
    order = [0, 1, 2, 3]
    random.shuffle(order)
    hue_factor = factors[3]
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError('hue_factor ({}) is not in [-0.5, 0.5].'.format(hue_factor))
    # torchvision F_pil.adjust_hue: np_h (uint8) += np.uint8(hue_factor * 255), wrapping
    hue_add = int(np.array(hue_factor * 255).astype(np.uint8))
    fac = [np.float32(factors[o]) if o < 3 else np.float32(0.0) for o in order]
    # the 3x4 'color' matrix of jittering[4] (augmentations.py:266-270): three more uniform draws AFTER the jitter transform's own,
    # a per-channel gain applied last with PIL's Image.convert('RGB', matrix) arithmetic (csrc/augment.hip: color_scale8)
    color = None
    if len(parameters) > 4 and parameters[4] > 0:
        color = [random.uniform(1. - parameters[4], 1 + parameters[4]) for _ in range(3)]
    return ops.jitter_record(order, [float(f) for f in fac], hue_add, 1, color)


class DeviceTrainTransform:
    """
    Parameters (as `get_transforms('train', ...)` of the reference)
    ----------
    image_shape : (H, W) or ()        output resolution
    jittering : (brightness, contrast, saturation, hue[, color]) or ()
    crop_train_borders : the reference's config value -- (y, height, x, width) or (y, x), negative / float forms included --
                         resolved against every incoming frame size by utils.misc.parse_crop_borders exactly like
                         train_transforms does (datasets/transforms.py:26-29), or ()
    """

    def __init__(self, image_shape=(), jittering=(), crop_train_borders=(), jitter_prob=1.0):
        self.image_shape = tuple(image_shape)
        self.jittering = tuple(jittering)
        self.crop_spec = tuple(crop_train_borders)
        self.jitter_prob = jitter_prob
        if self.crop_spec and len(self.crop_spec) not in (2, 4):
            raise NotImplementedError('Crop tuple must have 2 or 4 values.')

    def _geometry(self, frames, borders):
        if borders:
            l, t, r, b = borders
            frames = frames[:, t:b, l:r]
        if self.image_shape:
            frames = resize_frames(frames, self.image_shape)
        return frames.contiguous()

    def __call__(self, sample):
        """sample: {'rgb': uint8 [B,H,W,3], 'rgb_context': [uint8 [B,H,W,3], ...], 'intrinsics': [B,3,3]} on the device; optionally
        'depth' / 'input_depth': fp32 [B,h,w] or [B,1,h,w] and 'depth_context': a list of such maps -> fp32 [B,1,H,W] each."""
        out = dict(sample)
        rgb = sample['rgb']
        B, H0, W0, _ = rgb.shape
        ctx = list(sample.get('rgb_context', []))
        # geometry: every frame of the batch (target + contexts) in one launch per pass
        borders = parse_crop_borders(self.crop_spec, (H0, W0)) if self.crop_spec else ()
        allf = self._geometry(torch.cat([rgb] + ctx, 0) if ctx else rgb, borders)
        if 'intrinsics' in sample:
            K = sample['intrinsics'].clone()
            if borders:
                K[:, 0, 2] -= borders[0]
                K[:, 1, 2] -= borders[1]
            if self.image_shape:
                hc = (borders[3] - borders[1]) if borders else H0
                wc = (borders[2] - borders[0]) if borders else W0
                K[:, 0] *= self.image_shape[1] / wc
                K[:, 1] *= self.image_shape[0] / hc
            out['intrinsics'] = K
        # colour: one record per SAMPLE, shared by its target and context frames (augmentations.py:276-291)
        if self.jittering:
            recs = [draw_jitter(self.jittering, self.jitter_prob) for _ in range(B)]
        else:
            recs = [ops.jitter_record()] * B
        rec_all = b''.join(recs * (1 + len(ctx)))
        records = torch.frombuffer(bytearray(rec_all), dtype=torch.uint8).to(allf.device)
        jit, orig = ops.jitter_totensor(allf, records, want_original=True)
        out['rgb'], out['rgb_original'] = jit[:B], orig[:B]
        if ctx:
            out['rgb_context'] = [jit[B * (i + 1):B * (i + 2)] for i in range(len(ctx))]
            out['rgb_context_original'] = [orig[B * (i + 1):B * (i + 2)] for i in range(len(ctx))]
        # depth maps: the images' crop window (crop_sample = input + supervision), then resize_depth_preserve.  Consumes no random draw.
        keys = [k for k in ('depth', 'input_depth') if sample.get(k) is not None]
        dctx = list(sample.get('depth_context') or [])
        if keys or dctx:
            maps = depth_maps([sample[k] for k in keys] + dctx, borders, self.image_shape, ops.depth_resize_preserve)
            for k, m in zip(keys, maps):
                out[k] = m
            if dctx:
                out['depth_context'] = maps[len(keys):]
        return out


def depth_maps(maps, borders, image_shape, resize):
    """crop_depth (borders = (left, top, right, bottom) or ()) + `resize` (ops.depth_resize_preserve / ops.depth_resize_nearest) to
    image_shape, or the crop alone when image_shape is (), of a list of fp32 [B,h,w] / [B,1,h,w] maps -> a list of fp32 [B,1,H,W].  The
    crop is the kernel's window; maps of one source size share one launch."""
    maps = [m[:, 0] if m.dim() == 4 and m.shape[1] == 1 else m for m in maps]
    for m in maps:
        if m.dim() != 3 or m.dtype != torch.float32:
            raise RuntimeError('depth maps must be float32 [B,h,w] or [B,1,h,w], got %s %s' % (m.dtype, tuple(m.shape)))
    if not image_shape:
        if borders:
            l, t, r, b = borders
            maps = [m[:, t:b, l:r] for m in maps]
        return [m.unsqueeze(1).contiguous() for m in maps]
    out = [None] * len(maps)
    sizes = {}
    for i, m in enumerate(maps):
        sizes.setdefault(tuple(m.shape[1:]), []).append(i)
    for idx in sizes.values():
        group = torch.cat([maps[i] for i in idx], 0) if len(idx) > 1 else maps[idx[0]].contiguous()
        window = (borders[1], borders[0], borders[3] - borders[1], borders[2] - borders[0]) if borders else None
        res = resize(group, image_shape, window)
        n = 0
        for i in idx:
            out[i] = res[n:n + maps[i].shape[0]]
            n += maps[i].shape[0]
    return out


class DeviceEvalTransform:
    """`validation_transforms` / `test_transforms` of the reference (datasets/transforms.py:41-93) on the device, as they are:
    crop_sample_input crops 'rgb', 'rgb_context' and 'input_depth', shifts the principal point of 'intrinsics' and keeps the
    uncropped matrix in 'intrinsics_full' -- and leaves 'depth' (the ground truth) alone; only 'rgb' is resized (Lanczos), so
    'rgb_context' keeps its cropped size and 'intrinsics' are NOT rescaled; 'input_depth' is resized with resize_depth_preserve
    ('validation') or nearest ('test': cv2.resize INTER_NEAREST, restated but not pinned against OpenCV, include/pnsfm.h); ToTensor
    without '_original' copies and without jitter.

    Parameters
    ----------
    mode : 'validation' | 'test'
    image_shape : (H, W) or ()
    crop_eval_borders : the reference's config value (see DeviceTrainTransform), or ()
    dtype : torch.float32 | torch.float16 -- of 'rgb', 'rgb_context', 'depth' and 'input_depth' (what a `--half` evaluation feeds
            the network, written directly instead of an fp32 tensor and a cast)
    """

    def __init__(self, mode, image_shape=(), crop_eval_borders=(), dtype=torch.float32):
        if mode not in ('validation', 'test'):
            raise ValueError('Unknown mode {}'.format(mode))
        self.mode = mode
        self.image_shape = tuple(image_shape)
        self.crop_spec = tuple(crop_eval_borders)
        self.dtype = dtype
        if self.crop_spec and len(self.crop_spec) not in (2, 4):
            raise NotImplementedError('Crop tuple must have 2 or 4 values.')

    def __call__(self, sample):
        """sample: {'rgb': uint8 [B,H,W,3]; optionally 'rgb_context': [uint8 [B,H,W,3], ...], 'intrinsics': [B,3,3], 'depth' and
        'input_depth': fp32 [B,h,w] or [B,1,h,w]} on the device."""
        out = dict(sample)
        rgb = sample['rgb']
        ctx = list(sample.get('rgb_context', []))
        borders = parse_crop_borders(self.crop_spec, tuple(rgb.shape[1:3])) if self.crop_spec else ()
        if borders:
            l, t, r, b = borders
            rgb = rgb[:, t:b, l:r]
            ctx = [c[:, t:b, l:r] for c in ctx]
            if 'intrinsics' in sample:
                if 'intrinsics_full' not in sample:
                    out['intrinsics_full'] = sample['intrinsics'].clone()
                K = sample['intrinsics'].clone()
                K[:, 0, 2] -= l
                K[:, 1, 2] -= t
                out['intrinsics'] = K
        if self.image_shape:
            rgb = resize_frames(rgb, self.image_shape)
        out['rgb'] = ops.totensor8(rgb.contiguous(), self.dtype)
        if ctx:
            B = ctx[0].shape[0]
            allc = ops.totensor8(torch.cat(ctx, 0) if len(ctx) > 1 else ctx[0].contiguous(), self.dtype)
            out['rgb_context'] = [allc[B * i:B * (i + 1)] for i in range(len(ctx))]
        if sample.get('input_depth') is not None:
            resize = ops.depth_resize_preserve if self.mode == 'validation' else ops.depth_resize_nearest
            out['input_depth'] = depth_maps([sample['input_depth']], borders, self.image_shape, resize)[0].to(self.dtype)
        if sample.get('depth') is not None:
            out['depth'] = depth_maps([sample['depth']], (), (), None)[0].to(self.dtype)
        return out


def get_device_transforms(mode, image_shape, jittering, crop_train_borders, crop_eval_borders, **kwargs):
    """The reference's get_transforms (datasets/transforms.py:95-132) over the device pipeline: 'train' -> DeviceTrainTransform,
    'validation' | 'test' -> DeviceEvalTransform (fp32; construct it directly for fp16); any other mode raises ValueError.  Extra
    keyword arguments are ignored, as there."""
    if mode == 'train':
        return DeviceTrainTransform(image_shape=image_shape, jittering=jittering, crop_train_borders=crop_train_borders)
    elif mode in ('validation', 'test'):
        return DeviceEvalTransform(mode, image_shape=image_shape, crop_eval_borders=crop_eval_borders)
    else:
        raise ValueError('Unknown mode {}'.format(mode))
