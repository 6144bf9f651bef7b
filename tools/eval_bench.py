"""Evaluation / inference throughput of PackNet01 ('1A', eval mode, no grad): fp32 HIP, fp16 HIP and fp16 PyTorch eager (the reference's
`--half` path: oracle.packnet01_forward on an fp16 state dict, MIOpen convolutions) on the same device, alternated in one process.

    python tools/eval_bench.py [--sizes 192x640x1,192x640x4,384x1280x1] [--window 1.0] [--reps 3]

    python tools/eval_bench.py --layers          # the fp16 conv kernel alone, per layer class of PackNet01 at 192x640 batch 4

    python tools/eval_bench.py --metrics         # the tail of an evaluation step (post-process + 4 x depth metrics), KITTI shapes
    python tools/eval_bench.py --metrics-launches fused --calls 12     # N calls of one tail path, for a kernel trace (launch count)

    python tools/eval_bench.py --input           # the input pipeline (device validation / training transforms with depth maps) vs the host

    python tools/eval_bench.py --output          # the picture of an inference step (frame over colour-mapped inverse depth): host vs device
    python tools/eval_bench.py --output-launches --calls 12            # N calls of the device path, for a kernel trace (launch count)

Prints ONE JSON line: per size and path images/s, ms per forward (device events over windows of >= `window` s), host-issue ms per forward,
conv GFLOP from shapes (as executed, i.e. with the collapsed packing layers, and reference-algorithmic) and achieved conv TFLOP/s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'packnet-sfm_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def conv_gflop(B, H, W):
    """(executed, reference) conv GFLOP (2 x MACs, Conv3d included) of PackNet01 1A's forward at [B, 3, H, W], counted from the layer
    shapes by running oracle.packnet01_forward on meta tensors.  `executed` replaces each packing layer's Conv3d + Conv2d by what the
    collapsed form runs where PackLayerConv3d.collapse='auto' takes it: the composed (k+2)^2 convolution plus the border strips."""
    from oracle import packnet_oracle as O
    from packnet_sfm.networks.layers.packnet.layers01 import PackLayerConv3d
    F = O.F
    recs = []
    c2, c3 = F.conv2d, F.conv3d

    def conv2d(x, w, b=None, *a, **k):
        y = c2(x, w, b, *a, **k)
        recs.append(('2d', 2.0 * y.numel() * w.shape[1] * w.shape[2] * w.shape[3]))
        return y

    def conv3d(x, w, b=None, *a, **k):
        y = c3(x, w, b, *a, **k)
        recs.append(('3d', 2.0 * y.numel() * 27))
        return y
    sd = {k: torch.empty(v, device='meta') for k, v in O.packnet01_param_shapes('1A').items()}
    F.conv2d, F.conv3d = conv2d, conv3d
    try:
        O.packnet01_forward(sd, torch.empty((B, 3, H, W), device='meta'), version='1A', training=False)
    finally:
        F.conv2d, F.conv3d = c2, c3
    ref = sum(f for _, f in recs)
    ex = ref
    widths, ks = (64, 64, 128, 256, 512), (5, 3, 3, 3, 3)
    h, w = H, W
    for C, k in zip(widths, ks):
        h, w, C4, d = h // 2, w // 2, 4 * C, 8
        probe = PackLayerConv3d(C, k, d=d)
        if not probe._use_collapsed(h, w):
            continue
        r, S = k // 2, 2 * (k // 2) + 1
        orig = 2.0 * B * C * C4 * d * k * k * h * w + 2.0 * B * d * C4 * 27 * h * w
        coll = 2.0 * B * C * C4 * (k + 2) ** 2 * h * w
        coll += 2.0 * (2 * B) * C * C4 * d * k * k * (2 * r) * (w + h) + 2.0 * (2 * B) * d * C4 * 27 * S * (w + h)
        ex += coll - orig
    return ex / 1e9, ref / 1e9


# (class, Cin, Cout, H, W, ks) at 192 x 640: every distinct fp16 convolution of PackNet01 1A's eval forward (packs collapsed)
LAYER_CLASSES = [
    ('stem 5x5', 3, 64, 192, 640, 5), ('7x7 conv1', 64, 64, 192, 640, 7), ('pack1 collapsed 7x7', 256, 64, 96, 320, 7),
    ('pack2 collapsed 5x5', 256, 64, 48, 160, 5), ('pack3 collapsed 5x5', 512, 128, 24, 80, 5),
    ('pack4 collapsed 5x5', 1024, 256, 12, 40, 5), ('pack5 collapsed 5x5', 2048, 512, 6, 20, 5),
    ('3x3 96x320', 64, 64, 96, 320, 3), ('3x3 48x160', 128, 128, 48, 160, 3), ('3x3 24x80', 256, 256, 24, 80, 3),
    ('3x3 12x40', 512, 512, 12, 40, 3), ('3x3 6x20', 512, 512, 6, 20, 3), ('iconv1 3x3 cat', 129, 64, 192, 640, 3),
    ('1x1 48x160', 64, 128, 48, 160, 1), ('1x1 24x80', 128, 256, 24, 80, 1), ('1x1 12x40', 256, 512, 12, 40, 1)]


def layer_classes(B, window):
    """TFLOP/s of the fp16 convolution (pnsfm_conv2d_forward_h16, K-split stage included) per layer class, device events."""
    from packnet_sfm.hip import ops
    dev = torch.device('cuda:0')
    out = {}
    for name, Cin, Cout, H, W, ks in LAYER_CLASSES:
        x = torch.randn((B, Cin, H, W), device=dev).half()
        w = (torch.randn((Cout, Cin, ks, ks), device=dev) * (1.0 / (Cin * ks * ks)) ** 0.5).half()
        b = torch.zeros(Cout, device=dev)
        wp = ops.conv2d_pack_h16(w)
        xs = (x[:, :128].contiguous(), x[:, 128:].contiguous()) if 'cat' in name else (x,)
        fn = lambda: ops.conv2d_forward_h16(xs, wp, b, Cout, ks)       # noqa: E731
        for _ in range(3):
            fn()
        cfg = ops.conv2d_last_config()
        ms, _ = time_path(fn, window)
        gf = 2.0 * B * Cout * H * W * Cin * ks * ks / 1e9
        out[name] = {'shape': [B, Cin, Cout, H, W, ks], 'gflop': round(gf, 2), 'ms': round(ms, 4), 'tflops': round(gf / ms, 1),
                     'config': {'NT': cfg[1], 'MT': cfg[2], 'WM': cfg[3], 'ksplit': cfg[4], 'tile_w': cfg[5], 'workgroups': cfg[6]}}
    return out


def time_path(fn, window, ev_only=False):
    torch.cuda.synchronize()
    n, t_host, ms_dev = 0, 0.0, 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    while True:
        h0 = time.perf_counter()
        fn()
        t_host += time.perf_counter() - h0
        n += 1
        if time.perf_counter() - t0 >= window and n >= 3:
            break
        if n % 4 == 0:
            torch.cuda.synchronize()
    e1.record()
    torch.cuda.synchronize()
    ms_dev = e0.elapsed_time(e1)
    return ms_dev / n, 1e3 * t_host / n


def _tail_paths(cfg, gt, inv, inv_f):
    """The two forms of an evaluation step's tail after the two network forwards: (i) the Python composition -- inv2depth x 2, the
    post-process formula in torch, compute_depth_metrics x 4 (per-image gathers, medians and host syncs) -- and (ii) evaluate_depth
    (one post-process launch + 4 fused depth_metrics calls, metrics left on the device)."""
    from packnet_sfm.utils import depth as D

    def torch_post_process(a, f):
        W = a.shape[3]
        ah = f.flip(3)
        xs = torch.linspace(0., 1., W, device=a.device, dtype=a.dtype)
        mask = 1.0 - torch.clamp(20. * (xs - 0.05), 0., 1.)
        mask_hat = mask.flip(0)
        return mask_hat * a + mask * ah + (1.0 - mask - mask_hat) * (0.5 * (a + ah))

    def python_tail():
        depth, depth_pp = D.inv2depth(inv), D.inv2depth(torch_post_process(inv, inv_f))
        return [D.compute_depth_metrics(cfg, gt, depth_pp if 'pp' in m else depth, use_gt_scale='gt' in m) for m in ('', '_pp', '_gt', '_pp_gt')]

    def fused_tail():
        return list(D.evaluate_depth(cfg, gt, inv, inv_f)['metrics'].values())
    return {'python': python_tail, 'fused': fused_tail}


def _tail_inputs(B, dtype, dev):
    """KITTI-shaped: sparse ground truth 375 x 1242 (about a fifth of the pixels valid), inverse-depth predictions 192 x 640."""
    import types
    g = torch.Generator(device=dev).manual_seed(0)
    gt = 80 * torch.rand((B, 1, 375, 1242), device=dev, generator=g)
    gt[torch.rand((B, 1, 375, 1242), device=dev, generator=g) > 0.2] = 0
    inv = 1.0 / (2 + 70 * torch.rand((B, 1, 192, 640), device=dev, generator=g))
    inv_f = 1.0 / (2 + 70 * torch.rand((B, 1, 192, 640), device=dev, generator=g))
    cfg = types.SimpleNamespace(crop='garg', min_depth=0.0, max_depth=80.0, scale_output='resize')
    return cfg, gt.to(dtype), inv.to(dtype), inv_f.to(dtype)


def wall_per_call(fn, calls):
    """ms per call, host clock around the call AND a device synchronise (the Python tail syncs inside; device events alone would
    flatter it): (median, min) over `calls` calls."""
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def metrics_tail(a):
    dev = torch.device('cuda:0')
    result = {'tool': 'eval_bench --metrics', 'device': torch.cuda.get_device_name(0), 'gt': [375, 1242], 'pred': [192, 640],
              'crop': 'garg', 'modes': 4, 'timing': 'host clock around call + device synchronise, ms per call', 'settings': {}}
    with torch.no_grad():
        for B in (1, 4):
            for name, dtype in (('fp32', torch.float32), ('fp16', torch.float16)):
                paths = _tail_paths(*_tail_inputs(B, dtype, dev))
                outs = {k: [t.float().cpu() for t in fn()] for k, fn in paths.items()}
                for fn in paths.values():
                    for _ in range(5):
                        fn()
                samples = {k: [] for k in paths}
                for _ in range(a.reps):                      # alternate the two paths
                    for k, fn in paths.items():
                        samples[k].append(wall_per_call(fn, a.calls))
                entry = {k: {'ms_median': round(min(m for m, _ in v), 4), 'ms_min': round(min(lo for _, lo in v), 4),
                             'ms_median_all_rounds': [round(m, 4) for m, _ in v]} for k, v in samples.items()}
                entry['python_over_fused'] = round(entry['python']['ms_median'] / entry['fused']['ms_median'], 2)
                entry['max_abs_metric_difference'] = max(float((x - y).abs().max()) for x, y in zip(outs['python'], outs['fused']))
                result['settings']['b%d_%s' % (B, name)] = entry
        if not a.no_forward:                                 # the fp16 network forward in front of the tail, same process
            from oracle import packnet_oracle as O
            from packnet_sfm.networks.depth.PackNet01 import PackNet01
            net = PackNet01(dropout=0.0, version='1A')
            net.load_state_dict(O.init_params(O.packnet01_param_shapes('1A'), seed=0))
            net = net.to(dev, dtype=torch.float16).eval()
            result['hip16_forward_ms'] = {}
            for B in (1, 4):
                x = torch.rand((B, 3, 192, 640), device=dev).half()
                for _ in range(3):
                    net(rgb=x)
                result['hip16_forward_ms']['b%d' % B] = round(min(time_path(lambda: net(rgb=x), a.window)[0] for _ in range(a.reps)), 3)
    print(json.dumps(result))


def metrics_launches(a):
    """`--calls` calls of ONE tail path at batch 4, fp32, for `rocprofv3 --kernel-trace`: launches per call = (kernels traced with
    --calls n2) - (with --calls n1), over n2 - n1."""
    dev = torch.device('cuda:0')
    with torch.no_grad():
        fn = _tail_paths(*_tail_inputs(4, torch.float32, dev))[a.metrics_launches]
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
    print(json.dumps({'tool': 'eval_bench --metrics-launches', 'path': a.metrics_launches, 'calls': a.calls}))


def _host_resize_depth_preserve(depth, shape):
    """numpy restatement of the reference's resize_depth_preserve (datasets/augmentations.py:56-98), float64 output as there."""
    import numpy as np
    h, w = depth.shape
    ys, xs = np.nonzero(depth > 0)
    val = depth[ys, xs]
    ty, tx = (ys * (shape[0] / h)).astype(np.int32), (xs * (shape[1] / w)).astype(np.int32)
    keep = (ty < shape[0]) & (tx < shape[1])
    out = np.zeros(shape)
    out[ty[keep], tx[keep]] = val[keep]
    return out


def input_pipeline(a):
    """The input pipeline at KITTI shapes (frames and depth maps 375 x 1242 -> 192 x 640, about 5 % of the depth pixels valid), batch 1
    and batch 4: the device validation transform (fp16 out), the device training transform with 'depth' + 'input_depth' (two context
    frames, the YAML's jitter), the depth kernel alone with its achieved bytes/s next to this box's streaming-copy rate (measured as
    bench.py's calibration does), and the host path -- PIL for the images (oracle.augment_oracle), numpy for the depth maps -- per sample
    on one core."""
    import random

    import numpy as np
    from PIL import Image

    from oracle import augment_oracle as AO
    from packnet_sfm.datasets.device_transforms import DeviceEvalTransform, DeviceTrainTransform
    from packnet_sfm.hip import ops
    dev = torch.device('cuda:0')
    h, w, shape, jitter = 375, 1242, (192, 640), (0.2, 0.2, 0.2, 0.05)
    result = {'tool': 'eval_bench --input', 'device': torch.cuda.get_device_name(0), 'frames': [h, w], 'image_shape': list(shape),
              'depth_valid_fraction': 0.05, 'timing': 'device events over windows of >= %.1f s, best of %d; host: perf_counter, one core'
              % (a.window, a.reps), 'settings': {}}
    # streaming-copy rate of this box: 1 GiB -> 1 GiB float4 copy, read + write bytes (csrc/calib.hip), best of 3 after a warm-up
    src = torch.ones((1 << 30) // 4, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_gbps = 0.0
    for i in range(4):
        e0.record()
        nbytes = ops.calib_copy(src, dst)
        e1.record()
        torch.cuda.synchronize()
        if i:
            copy_gbps = max(copy_gbps, nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    del src, dst
    torch.cuda.empty_cache()
    result['streaming_copy_gbps'] = round(copy_gbps, 1)
    rng = np.random.default_rng(0)
    for B in (1, 4):
        fr = rng.integers(0, 256, (3 * B, h, w, 3), dtype=np.uint8)
        dm = (80 * rng.random((2 * B, h, w))).astype(np.float32)
        dm[rng.random(dm.shape) > 0.05] = 0
        K = np.array([[0.58 * w, 0, 0.5 * w], [0, 1.92 * h, 0.5 * h], [0, 0, 1]])
        sample = {'rgb': torch.from_numpy(fr[:B]).to(dev), 'rgb_context': [torch.from_numpy(fr[B:2 * B]).to(dev), torch.from_numpy(fr[2 * B:]).to(dev)],
                  'intrinsics': torch.from_numpy(np.stack([K] * B)).to(dev),
                  'depth': torch.from_numpy(dm[:B]).to(dev), 'input_depth': torch.from_numpy(dm[B:]).to(dev)}
        val_sample = {k: v for k, v in sample.items() if k != 'rgb_context'}
        val_t, train_t = DeviceEvalTransform('validation', shape, (), torch.float16), DeviceTrainTransform(shape, jitter, ())
        both = torch.cat([sample['depth'], sample['input_depth']], 0)
        paths = {'device_validation_fp16': lambda: val_t(val_sample), 'device_train_depth': lambda: train_t(sample),
                 'depth_resize_preserve_kernel': lambda: ops.depth_resize_preserve(both, shape)}
        for fn in paths.values():
            for _ in range(5):
                fn()
        samples = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, fn in paths.items():
                samples[k].append(time_path(fn, a.window))
        entry = {}
        for k, v in samples.items():
            ms, host = min(v)
            entry[k] = {'ms_per_call': round(ms, 4), 'samples_per_s': round(1e3 * B / ms, 1), 'host_issue_ms': round(host, 4),
                        'ms_all_windows': [round(s[0], 4) for s in v]}
        # the depth kernel's bytes from shapes: every source pixel read once, every output pixel written once (fp32)
        kbytes = 2 * B * (h * w + shape[0] * shape[1]) * 4
        kern = entry['depth_resize_preserve_kernel']
        kern.update({'maps': 2 * B, 'bytes': kbytes, 'gbps': round(kbytes / (kern['ms_per_call'] * 1e-3) / 1e9, 1),
                     'fraction_of_streaming_copy': round(kbytes / (kern['ms_per_call'] * 1e-3) / 1e9 / copy_gbps, 4),
                     'note': 'ms_per_call is device time between events around back-to-back launches: it includes the launch gap'})
        del kern['samples_per_s']

        # host path, per sample on one core
        def host_validation(b):
            img = AO.to_tensor(AO.resize_image(Image.fromarray(fr[b]), shape)).half()
            return img, torch.from_numpy(_host_resize_depth_preserve(dm[B + b], shape)).half(), torch.from_numpy(dm[b]).half()

        def host_train(b):
            s = AO.train_transforms({'rgb': Image.fromarray(fr[b]), 'rgb_context': [Image.fromarray(fr[B + b]), Image.fromarray(fr[2 * B + b])],
                                     'intrinsics': K.copy()}, shape, jitter, ())
            s['depth'] = torch.from_numpy(_host_resize_depth_preserve(dm[b], shape)).float()
            s['input_depth'] = torch.from_numpy(_host_resize_depth_preserve(dm[B + b], shape)).float()
            return s
        random.seed(0)
        torch.set_num_threads(1)
        for name, fn in (('host_validation_fp16', host_validation), ('host_train_depth', host_train)):
            fn(0)
            ts = []
            for i in range(max(4, a.reps * 2)):
                t0 = time.perf_counter()
                fn(i % B)
                ts.append(1e3 * (time.perf_counter() - t0))
            ts.sort()
            entry[name] = {'ms_per_sample': round(ts[len(ts) // 2], 3), 'ms_min': round(ts[0], 3), 'samples_per_s_per_core': round(1e3 / ts[len(ts) // 2], 1)}
        # same results on both paths (bit for bit: that is what the tests assert at these shapes too)
        dv, hv = val_t(val_sample), host_validation(0)
        entry['validation_matches_host'] = bool(torch.equal(dv['rgb'][0].cpu(), hv[0]) and torch.equal(dv['input_depth'][0, 0].cpu(), hv[1]))
        result['settings']['b%d' % B] = entry
    print(json.dumps(result))


def _host_viz():
    """(viz_inv_depth, where it comes from, the colormap argument for the device path).  The reference's own function when a checkout
    is on the path and loads; otherwise its numpy restatement (np.percentile, in-place divide, clip, colormap call), which the tests
    hold equal to it -- with matplotlib's plasma, or without matplotlib with the same table from tests/golden/viz.pt."""
    import numpy as np
    try:
        from packnet_sfm.utils import depth as D
        return D.viz_inv_depth, 'reference checkout', 'plasma'
    except Exception:
        pass
    try:
        import matplotlib
        cm, source, colormap = matplotlib.colormaps['plasma'], 'numpy restatement, matplotlib colormap call', 'plasma'
    except ImportError:
        table = torch.load(os.path.join(ROOT, 'tests', 'golden', 'viz.pt'), weights_only=False)['plasma'].numpy()

        def cm(x):
            xa = x * 256
            xa[xa == 256] = 255
            return table[xa.astype(int)]
        source, colormap = 'numpy restatement, plasma table of tests/golden/viz.pt', table

    def viz_inv_depth(inv_depth, percentile=95):
        x = inv_depth.squeeze(0).detach().cpu().numpy()
        normalizer = np.percentile(x, percentile)
        x /= (normalizer + 1e-6)
        return cm(np.clip(x, 0., 1.0))[:, :, :3]
    return viz_inv_depth, source, colormap


def output_path(a):
    """The picture an inference step writes (scripts/infer.py:97-107: the frame on top of viz_inv_depth, as bytes), fp32 maps and
    frames: (a) the host path exactly as infer.py composes it, per image -- frame and map copied to the host, viz_inv_depth(...) *
    255, the concatenation, the cast to uint8 (rint, what cv2.imwrite does with the float image) -- against (b) the device path --
    utils.depth.viz_inv_depth_u8 with rgb for the batch, then the device->host copy of the uint8 panel.  Both end with the bytes on
    the host, so both are timed on the host clock: windows of >= `window` s, alternated, best of `reps`.  The panels must be equal."""
    import numpy as np

    from packnet_sfm.utils import depth as D
    dev = torch.device('cuda:0')
    viz_inv_depth, source, colormap = _host_viz()
    result = {'tool': 'eval_bench --output', 'device': torch.cuda.get_device_name(0), 'host_function': source, 'dtype': 'fp32',
              'timing': 'host clock over windows of >= %.1f s, alternated, best of %d; both paths end with the uint8 panel on the host'
              % (a.window, a.reps),
              'launches_per_call': {'memset': 1, 'kernels': 5, 'note': 'fixed by csrc/depth_output.h whatever the batch and image size; counted with --output-launches under a kernel trace'},
              'sizes': {}}

    def window(fn):
        """(ms per call, ms per call spent in fn's first stage) over one window; fn returns its first stage's seconds."""
        torch.cuda.synchronize()
        n, first = 0, 0.0
        t0 = time.perf_counter()
        while True:
            first += fn()
            n += 1
            t = time.perf_counter() - t0
            if t >= a.window and n >= 3:
                return 1e3 * t / n, 1e3 * first / n

    for spec in a.sizes.split(','):
        H, W, B = (int(v) for v in spec.split('x'))
        g = torch.Generator(device=dev).manual_seed(0)
        image = torch.rand((B, 3, H, W), device=dev, generator=g)
        pred = 1.0 / (2 + 70 * torch.rand((B, 1, H, W), device=dev, generator=g))
        panels = {}

        def host():
            t0 = time.perf_counter()
            out = []
            for b in range(B):
                rgb = image[b].permute(1, 2, 0).detach().cpu().numpy() * 255
                viz = viz_inv_depth(pred[b]) * 255
                out.append(np.clip(np.rint(np.concatenate([rgb, viz], 0)), 0, 255).astype(np.uint8))
            panels['host'] = out
            return time.perf_counter() - t0

        def device():
            t0 = time.perf_counter()
            out = D.viz_inv_depth_u8(pred, rgb=image, colormap=colormap)
            t1 = time.perf_counter()
            panels['device'] = out.cpu().numpy()
            return t1 - t0
        paths = {'host': host, 'device': device}
        with torch.no_grad():
            for fn in paths.values():
                for _ in range(5):
                    fn()
            equal = all(np.array_equal(panels['host'][b], panels['device'][b]) for b in range(B))
            assert equal, 'the host and the device panel differ at %s' % spec
            samples = {k: [] for k in paths}
            for _ in range(a.reps):
                for k, fn in paths.items():
                    samples[k].append(window(fn))
        hm, dm = min(samples['host']), min(samples['device'])
        result['sizes']['%dx%d_b%d' % (H, W, B)] = {
            'host_ms_per_image': round(hm[0] / B, 4), 'device_ms_per_image': round(dm[0] / B, 4),
            'device_ms_per_call': round(dm[0], 4), 'device_host_issue_ms_per_call': round(dm[1], 4),
            'device_host_issue_share': round(dm[1] / dm[0], 3), 'host_over_device': round(hm[0] / dm[0], 2), 'panels_equal': equal,
            'host_ms_per_call_all_windows': [round(s[0], 4) for s in samples['host']],
            'device_ms_per_call_all_windows': [round(s[0], 4) for s in samples['device']]}
    print(json.dumps(result))


def output_launches(a):
    """`--calls` calls of the device path of --output at 192x640 batch 4 (frame and map, fp32), for `rocprofv3 --kernel-trace`: launches
    per call = (kernels traced with --calls n2) - (with --calls n1), over n2 - n1."""
    from packnet_sfm.utils import depth as D
    dev = torch.device('cuda:0')
    colormap = _host_viz()[2]
    with torch.no_grad():
        g = torch.Generator(device=dev).manual_seed(0)
        image = torch.rand((4, 3, 192, 640), device=dev, generator=g)
        pred = 1.0 / (2 + 70 * torch.rand((4, 1, 192, 640), device=dev, generator=g))
        for _ in range(a.calls):
            D.viz_inv_depth_u8(pred, rgb=image, colormap=colormap)
        torch.cuda.synchronize()
    print(json.dumps({'tool': 'eval_bench --output-launches', 'calls': a.calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='192x640x1,192x640x4,384x1280x1')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--paths', default='hip32,hip16,eager16')
    ap.add_argument('--layers', action='store_true', help='per-layer-class TFLOP/s of the fp16 conv kernel (192x640, --batch)')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--metrics', action='store_true', help='tail of an evaluation step: Python composition vs evaluate_depth')
    ap.add_argument('--metrics-launches', choices=('python', 'fused'), help='run --calls calls of one tail path (for a kernel trace)')
    ap.add_argument('--calls', type=int, default=30, help='--metrics: calls per round and path')
    ap.add_argument('--no-forward', action='store_true', help='--metrics: skip the fp16 network forward')
    ap.add_argument('--input', action='store_true', help='input pipeline at KITTI shapes: device transforms vs the host path')
    ap.add_argument('--output', action='store_true', help='the picture of an inference step at --sizes: host path vs viz_inv_depth_u8')
    ap.add_argument('--output-launches', action='store_true', help='run --calls calls of the device path of --output (for a kernel trace)')
    a = ap.parse_args()
    if a.output_launches:
        return output_launches(a)
    if a.output:
        return output_path(a)
    if a.input:
        return input_pipeline(a)
    if a.metrics_launches:
        return metrics_launches(a)
    if a.metrics:
        return metrics_tail(a)
    if a.layers:
        with torch.no_grad():
            print(json.dumps({'tool': 'eval_bench --layers', 'device': torch.cuda.get_device_name(0), 'batch': a.batch,
                              'kernel': 'conv2d_h16 (variant 9)', 'layers': layer_classes(a.batch, a.window)}))
        return
    from oracle import packnet_oracle as O
    from packnet_sfm.networks.depth.PackNet01 import PackNet01
    dev = torch.device('cuda:0')
    sd = O.init_params(O.packnet01_param_shapes('1A'), seed=0)
    n32 = PackNet01(dropout=0.0, version='1A')
    n32.load_state_dict(sd)
    n32 = n32.to(dev).eval()
    n16 = PackNet01(dropout=0.0, version='1A')
    n16.load_state_dict(sd)
    n16 = n16.to(dev, dtype=torch.float16).eval()
    sd16 = {k: v.to(dev).half() for k, v in sd.items()}
    result = {'tool': 'eval_bench', 'device': torch.cuda.get_device_name(0), 'net': 'PackNet01 1A eval, torch.no_grad', 'sizes': {}}
    for spec in a.sizes.split(','):
        H, W, B = (int(v) for v in spec.split('x'))
        x32 = torch.rand((B, 3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        x16 = x32.half()
        paths = {'hip32': lambda: n32(rgb=x32), 'hip16': lambda: n16(rgb=x16),
                 'eager16': lambda: O.packnet01_forward(sd16, x16, version='1A', training=False)}
        paths = {k: v for k, v in paths.items() if k in a.paths.split(',')}
        with torch.no_grad():
            gf_exec, gf_ref = conv_gflop(B, H, W)
            for fn in paths.values():        # warm-up: packing, allocator, MIOpen find
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            samples = {k: [] for k in paths}
            for _ in range(a.reps):          # alternate the paths, best window of each
                for k, fn in paths.items():
                    samples[k].append(time_path(fn, a.window))
        entry = {'gflop_conv_executed': round(gf_exec, 2), 'gflop_conv_reference': round(gf_ref, 2)}
        for k, v in samples.items():
            ms, host = min(v)
            gf = gf_ref if k == 'eager16' else gf_exec
            entry[k] = {'ms_per_forward': round(ms, 3), 'images_per_s': round(1e3 * B / ms, 2), 'host_issue_ms': round(host, 3),
                        'conv_tflops': round(gf / ms, 1), 'ms_all_windows': [round(s[0], 3) for s in v]}
        if 'hip16' in entry and 'hip32' in entry:
            entry['speedup_hip16_vs_hip32'] = round(entry['hip32']['ms_per_forward'] / entry['hip16']['ms_per_forward'], 3)
        result['sizes']['%dx%d_b%d' % (H, W, B)] = entry
    print(json.dumps(result))


if __name__ == '__main__':
    main()
