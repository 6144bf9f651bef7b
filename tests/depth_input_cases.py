"""Depth-input cases (csrc/depth_input.h: depth_resize_preserve, depth_resize_nearest, totensor8; packnet_sfm/datasets/device_transforms.py:
the depth keys of DeviceTrainTransform, DeviceEvalTransform, get_device_transforms) shared by the emulated CPU tests
(tests/test_depth_input_emulated.py) and the GPU tests (tests/test_gpu_depth_input.py).

Depth inputs come from an integer hash, so they are the same numbers on every machine and need no storage: DISTINCT positive values
(a collision between source pixels is then visible: "first wins" or "max wins" gives another map than "last in row-major order wins")
thinned to a density.  The REFERENCE's own resize_depth_preserve / crop_depth outputs for PRESERVE_CASES are in
tests/golden/depth_input.pt with a checksum of each input (tools/make_depth_input_golden.py imports the builders below).

`resize_preserve_np` / `resize_nearest_np` restate the two rules in numpy.  The first is checked against the golden on every case
(test_restatement_matches_golden), which licenses it as the expectation of the full-size and transform cases.  The second restates
OpenCV's INTER_NEAREST; OpenCV is not installed here, so nothing pins it against the real library."""
import os
import random

import numpy as np
import torch
from PIL import Image

from oracle import augment_oracle as AO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'depth_input.pt')

# (h, w) -> (H, W), density
SHAPE_CASES = {
    'down': ((37, 124), (19, 64), 0.3),        # plain downscale
    'up': ((24, 40), (48, 56), 0.5),           # upscale: holes
    'coll3': ((41, 70), (16, 32), 0.9),        # 3x3 source pixels per cell
    'axis': ((30, 50), (30, 25), 0.2),         # one axis only
    'rows8': ((50, 31), (7, 31), 1.0),         # 8 rows per cell
    'offby1': ((33, 65), (32, 64), 0.6),       # ratios just below 1
}
PRESERVE_CASES = list(SHAPE_CASES) + ['zeros', 'invalid', 'batch3', 'window']
NEAREST_CASES = list(SHAPE_CASES) + ['double', 'half']
YAML_JITTER = (0.2, 0.2, 0.2, 0.05)


def _hash01(n, seed):
    """float64 in [0, 1) from an integer hash of (element index, seed): exact integer arithmetic, identical on every machine."""
    m = np.uint64(0xffffffff)
    h = (np.arange(n, dtype=np.uint64) + np.uint64(1 + 7919 * seed)) * np.uint64(2654435761) & m
    h ^= h >> np.uint64(15)
    h = h * np.uint64(2246822519) & m
    h ^= h >> np.uint64(13)
    h = h * np.uint64(3266489917) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.float64) / float(1 << 32)


def depth_maps(N, h, w, density, seed):
    """fp32 [N,h,w]: value (s + 1) / 64 with s = a bijection of the element index on [0, 2^22) -- distinct, exact in fp32 -- where the
    hash is below `density`, 0 elsewhere."""
    n = N * h * w
    assert n <= 1 << 22
    s = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345 + seed)) & np.uint64((1 << 22) - 1)
    v = ((s + np.uint64(1)).astype(np.float64) / 64.0).astype(np.float32)
    return np.where(_hash01(n, seed) < density, v, np.float32(0)).reshape(N, h, w)


def preserve_inputs(name):
    """-> (maps fp32 [N,h0,w0], window (y0, x0, h, w) or None, (H, W))"""
    if name in SHAPE_CASES:
        (h, w), shape, density = SHAPE_CASES[name]
        return depth_maps(1, h, w, density, 1 + list(SHAPE_CASES).index(name)), None, shape
    if name == 'zeros':
        return np.zeros((1, 21, 33), np.float32), None, (8, 16)
    if name == 'invalid':                        # NaN, negative and zero entries among the valid ones
        d = depth_maps(1, 41, 70, 1.0, 11)
        u = _hash01(d.size, 12).reshape(d.shape)
        d = np.where(u < 0.2, np.float32('nan'), np.where(u < 0.4, -d, np.where(u < 0.6, np.float32(0), d))).astype(np.float32)
        return d, None, (16, 32)
    if name == 'batch3':
        return depth_maps(3, 37, 124, 0.3, 13), None, (19, 64)
    if name == 'window':
        return depth_maps(1, 41, 70, 0.9, 14), (5, 3, 32, 64), (16, 32)
    raise KeyError(name)


def nearest_inputs(name):
    if name == 'double':
        return depth_maps(2, 12, 20, 0.7, 21), None, (24, 40)
    if name == 'half':
        return depth_maps(2, 24, 40, 0.7, 22), None, (12, 20)
    return preserve_inputs(name)


def checksum(a):
    """Bit-pattern checksum of an fp32 array."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64).reshape(-1)
    return int((b * (np.arange(b.size, dtype=np.uint64) % np.uint64(65521) + np.uint64(1))).sum() % np.uint64(1 << 61))


def crop_np(d, window):
    if window is None:
        return d
    y0, x0, h, w = window
    return d[..., y0:y0 + h, x0:x0 + w]


# ----------------------------------------------------------------------------------------------- numpy restatements
def resize_preserve_np(depth, shape):
    """[h,w] -> fp32 [H,W]: every pixel > 0 goes to (int(y * (H / h)), int(x * (W / w))); targets outside are dropped; per cell the
    source with the LARGEST row-major index wins (stated explicitly through maximum.at, not left to the assignment order)."""
    h, w = depth.shape
    H, W = shape
    ys, xs = np.nonzero(depth > 0)
    ty, tx = (ys * (H / h)).astype(np.int32), (xs * (W / w)).astype(np.int32)
    keep = (ty < H) & (tx < W)
    win = np.full(H * W, -1, dtype=np.int64)
    np.maximum.at(win, ty[keep].astype(np.int64) * W + tx[keep], ys[keep].astype(np.int64) * w + xs[keep])
    flat = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
    return np.where(win >= 0, flat[np.maximum(win, 0)], np.float32(0)).reshape(H, W).astype(np.float32)


def resize_nearest_np(depth, shape):
    """[h,w] -> [H,W]: out(Y, X) = in(min(floor(Y * ify), h - 1), min(floor(X * ifx), w - 1)), ify = 1 / (H / h), ifx = 1 / (W / w)."""
    h, w = depth.shape
    H, W = shape
    iy = np.minimum(np.floor(np.arange(H) * (1.0 / (float(H) / h))).astype(np.int64), h - 1)
    ix = np.minimum(np.floor(np.arange(W) * (1.0 / (float(W) / w))).astype(np.int64), w - 1)
    return np.ascontiguousarray(depth[iy][:, ix], dtype=np.float32)


def _stack(fn, maps, window, shape):
    return torch.from_numpy(np.stack([fn(crop_np(m, window), shape) for m in maps]))[:, None]


_GOLD = None


def golden():
    global _GOLD
    if _GOLD is None:
        _GOLD = torch.load(GOLDEN, weights_only=False)
    return _GOLD


# ----------------------------------------------------------------------------------------------- kernel cases
def preserve_case(device, name):
    from packnet_sfm.hip import ops
    maps, window, shape = preserve_inputs(name)
    g = golden()
    assert checksum(maps) == g['checksums'][name], 'input of case %s is not the one the golden was made from' % name
    got = ops.depth_resize_preserve(torch.from_numpy(maps).to(device), shape, window)
    assert got.dtype == torch.float32 and tuple(got.shape) == (maps.shape[0], 1) + tuple(shape)
    assert torch.equal(got.cpu(), g['preserve'][name]), 'depth_resize_preserve differs from the reference (%s)' % name
    if name == 'batch3':                          # the [N,1,h,w] form is the same call
        assert torch.equal(ops.depth_resize_preserve(torch.from_numpy(maps[:, None]).to(device), shape).cpu(), g['preserve'][name])


def restatement_case(name):
    maps, window, shape = preserve_inputs(name)
    g = golden()
    assert np.array_equal(_stack(resize_preserve_np, maps, window, shape).numpy(), g['preserve'][name].numpy()), name
    if name == 'window':
        assert np.array_equal(crop_np(maps, window), g['crop'][name].numpy())


def nearest_case(device, name):
    from packnet_sfm.hip import ops
    maps, window, shape = nearest_inputs(name)
    got = ops.depth_resize_nearest(torch.from_numpy(maps).to(device), shape, window)
    assert got.dtype == torch.float32
    assert torch.equal(got.cpu(), _stack(resize_nearest_np, maps, window, shape)), name
    if name in ('double', 'half'):                # exact ratios: the plain index rule
        f = 2 if name == 'double' else 1
        s = 1 if name == 'double' else 2
        exp = torch.from_numpy(maps)[:, None, ::s, ::s].repeat_interleave(f, 2).repeat_interleave(f, 3)
        assert torch.equal(got.cpu(), exp)


def window_errors_case(device):
    from packnet_sfm.hip import ops
    d = torch.zeros((1, 8, 9), device=device)
    for fn in (ops.depth_resize_preserve, ops.depth_resize_nearest):
        for window in ((0, 0, 9, 9), (2, 0, 7, 9), (0, -1, 4, 4), (0, 0, 0, 4)):
            try:
                fn(d, (4, 4), window)
            except RuntimeError:
                continue
            raise AssertionError('window %s of an 8x9 map was accepted' % (window,))
        try:
            fn(d.double(), (4, 4))
        except RuntimeError:
            continue
        raise AssertionError('float64 maps were accepted')


def frames(N, H, W, seed):
    """uint8 [N,H,W,3]: smooth content + noise (Lanczos overshoot clips at both ends)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (N, H // 4 + 1, W // 4 + 1, 3), dtype=np.uint8)
    up = np.stack([np.asarray(Image.fromarray(b).resize((W, H), Image.BILINEAR)) for b in base])
    return np.clip(up.astype(np.int32) + rng.integers(-40, 41, up.shape), 0, 255).astype(np.uint8)


def totensor_case(device, N, H, W):
    from packnet_sfm.hip import ops
    img = frames(N, H, W, 31)
    t = torch.from_numpy(img).to(device)
    got = ops.totensor8(t)
    records = torch.frombuffer(bytearray(ops.jitter_record() * N), dtype=torch.uint8).to(device)
    orig = ops.jitter_totensor(t, records, want_original=True)[1]
    assert got.dtype == torch.float32 and torch.equal(got, orig)
    assert torch.equal(got.cpu(), torch.stack([AO.to_tensor(Image.fromarray(f)) for f in img]))
    half = ops.totensor8(t, torch.float16)
    assert half.dtype == torch.float16 and torch.equal(half, got.half())


# ----------------------------------------------------------------------------------------------- transform cases
TRAIN_CASES = [  # B, H, W, image_shape, jittering, crop borders
    (2, 37, 124, (19, 64), YAML_JITTER, ()),
    (2, 41, 70, (16, 32), (), (5, 32, 3, 64)),
    (1, 41, 70, (), (), (-5, 3)),
]


def _window_of(borders):
    return (borders[1], borders[0], borders[3] - borders[1], borders[2] - borders[0])


def _expected_maps(maps, borders, shape, fn):
    """maps [B,h,w] numpy -> torch [B,1,·,·]: crop_depth, then the resize rule (or the crop alone without a shape)."""
    window = _window_of(borders) if borders else None
    if not shape:
        return torch.from_numpy(np.ascontiguousarray(crop_np(maps, window)))[:, None]
    return _stack(fn, maps, window, shape)


def train_case(device, B, H, W, shape, jitter, borders_spec):
    from packnet_sfm.datasets.device_transforms import DeviceTrainTransform
    fr = frames(3 * B, H, W, 41)
    rgb, ctx = fr[:B], [fr[B:2 * B], fr[2 * B:]]
    K = np.array([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=np.float64)
    dm = depth_maps(4 * B, H, W, 0.4, 42).reshape(4, B, H, W)          # depth, input_depth, two depth_context maps
    random.seed(141)
    ref = [AO.train_transforms({'rgb': Image.fromarray(rgb[b]), 'rgb_context': [Image.fromarray(c[b]) for c in ctx],
                                'intrinsics': K.copy()}, shape, jitter, borders_spec) for b in range(B)]
    state = random.getstate()
    random.seed(141)
    out = DeviceTrainTransform(shape, jitter, borders_spec)({
        'rgb': torch.from_numpy(rgb).to(device), 'rgb_context': [torch.from_numpy(c).to(device) for c in ctx],
        'intrinsics': torch.from_numpy(np.stack([K] * B)).to(device),
        'depth': torch.from_numpy(dm[0]).to(device), 'input_depth': torch.from_numpy(dm[1][:, None]).to(device),
        'depth_context': [torch.from_numpy(dm[2]).to(device), torch.from_numpy(dm[3]).to(device)]})
    assert random.getstate() == state, 'the depth keys changed the random draws'
    for b in range(B):
        for key in ('rgb', 'rgb_original'):
            assert torch.equal(out[key][b].cpu(), ref[b][key]), '%s differs from PIL (sample %d)' % (key, b)
        for key in ('rgb_context', 'rgb_context_original'):
            for j in range(2):
                assert torch.equal(out[key][j][b].cpu(), ref[b][key][j]), '%s[%d] differs from PIL (sample %d)' % (key, j, b)
        np.testing.assert_allclose(out['intrinsics'][b].cpu().numpy(), ref[b]['intrinsics'], rtol=1e-12)
    borders = AO.parse_crop_borders(borders_spec, (H, W)) if borders_spec else ()
    oh, ow = shape if shape else ((borders[3] - borders[1], borders[2] - borders[0]) if borders else (H, W))
    got = [out['depth'], out['input_depth']] + list(out['depth_context'])
    assert len(out['depth_context']) == 2
    for i, g in enumerate(got):
        assert g.dtype == torch.float32 and tuple(g.shape) == (B, 1, oh, ow), (i, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), _expected_maps(dm[i], borders, shape, resize_preserve_np)), 'depth map %d' % i


def eval_case(device, mode, borders_spec, dtype, B=2, H=41, W=70, shape=(16, 32), density=0.5, check_frames=None):
    from packnet_sfm.datasets.device_transforms import DeviceEvalTransform
    fr = frames(2 * B, H, W, 51)
    rgb, ctx = fr[:B], fr[B:]
    K = torch.from_numpy(np.stack([np.array([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=np.float64)] * B))
    dm = depth_maps(2 * B, H, W, density, 52).reshape(2, B, H, W)      # depth (ground truth), input_depth
    sample = {'rgb': torch.from_numpy(rgb).to(device), 'rgb_context': [torch.from_numpy(ctx).to(device)], 'intrinsics': K.to(device),
              'depth': torch.from_numpy(dm[0]).to(device), 'input_depth': torch.from_numpy(dm[1]).to(device)}
    out = DeviceEvalTransform(mode, shape, borders_spec, dtype)(sample)
    borders = AO.parse_crop_borders(borders_spec, (H, W)) if borders_spec else ()
    box = borders if borders else (0, 0, W, H)
    for b in (range(B) if check_frames is None else check_frames):
        exp = AO.to_tensor(AO.resize_image(Image.fromarray(rgb[b]).crop(box), shape)).to(dtype)
        assert out['rgb'].dtype == dtype and torch.equal(out['rgb'][b].cpu(), exp), 'rgb (sample %d)' % b
        exp = AO.to_tensor(Image.fromarray(ctx[b]).crop(box)).to(dtype)           # cropped, NOT resized
        assert torch.equal(out['rgb_context'][0][b].cpu(), exp), 'rgb_context (sample %d)' % b
    assert len(out['rgb_context']) == 1 and tuple(out['rgb_context'][0].shape) == (B, 3, box[3] - box[1], box[2] - box[0])
    Kexp = K.clone()
    Kexp[:, 0, 2] -= box[0]
    Kexp[:, 1, 2] -= box[1]
    assert torch.equal(out['intrinsics'].cpu(), Kexp)                              # principal point shifted, nothing rescaled
    if borders:
        assert torch.equal(out['intrinsics_full'].cpu(), K)
    else:
        assert 'intrinsics_full' not in out                                        # crop_sample_input alone creates it
    assert torch.equal(out['depth'].cpu(), torch.from_numpy(dm[0])[:, None].to(dtype))   # the ground truth: neither cropped nor resized
    fn = resize_preserve_np if mode == 'validation' else resize_nearest_np
    assert out['input_depth'].dtype == dtype and tuple(out['input_depth'].shape) == (B, 1) + tuple(shape)
    assert torch.equal(out['input_depth'].cpu(), _expected_maps(dm[1], borders, shape, fn).to(dtype)), 'input_depth'
    assert 'rgb_original' not in out and 'rgb_context_original' not in out


def get_transforms_case():
    from packnet_sfm.datasets import device_transforms as T
    t = T.get_device_transforms('train', (19, 64), YAML_JITTER, (5, 3), (2, 2), unused=1)
    assert type(t) is T.DeviceTrainTransform and t.image_shape == (19, 64) and t.jittering == YAML_JITTER and t.crop_spec == (5, 3)
    for mode in ('validation', 'test'):
        t = T.get_device_transforms(mode, (19, 64), YAML_JITTER, (5, 3), (2, 2))
        assert type(t) is T.DeviceEvalTransform and t.mode == mode and t.image_shape == (19, 64) and t.crop_spec == (2, 2)
        assert t.dtype == torch.float32
    for bad in ('foo', ''):
        try:
            T.get_device_transforms(bad, (), (), (), ())
        except ValueError:
            continue
        raise AssertionError('mode %r was accepted' % bad)
