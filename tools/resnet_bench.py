"""What the ResNet networks cost on the MI355X.

    python tools/resnet_bench.py [--section all|bn|step|half] [--steps 10] [--repeats 7] [--out profiles/resnet_bench.json]

Step = forward + backward of SelfSupModel(DepthResNet18, PoseResNet18) at 192x640, batch 4, against the eager twin
(tests/resnet_cases.torch_forward: the same parameters through ATen) in the same process: the two alternate in windows of --steps steps,
each window timed with device events after --warmup untimed steps, medians over --repeats windows.  Launches per step are counted with
the kernel profiler's device-activity events.  For batchnorm_act forward and backward at bn1's [4,64,96,320] and layer4's [4,512,6,20]
it reports the achieved bytes/s (one read of every input, one write of every output) next to pnsfm_calib_copy's rate in the same run.
--section half (a run of its own): the eval forward of DepthResNet18 at batch 1 and 4 in fp16 on the gathering kernels, in
fp32 on this tree's kernels and in fp16 through the twin, alternating in windows as the step section does; launches per forward; achieved
TFLOP/s of the fp16 kernel per layer class at batch 1 (launch through the Python wrapper included, output preallocated).
At most 16 host threads."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'packnet-sfm_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))


def timed(fn, n):
    """Milliseconds per call of fn over n calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def bn_section(B, H, W, dev):
    """batchnorm_act forward / backward at bn1's and layer4's shapes next to the copy kernel's rate: needs no network."""
    from packnet_sfm.hip import ops
    res = {}
    src = torch.randn(64 * 1024 * 1024 // 4, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        ops.calib_copy(src, dst)
    copy_ms = statistics.median(timed(lambda: ops.calib_copy(src, dst), 20) for _ in range(5))
    res['calib_copy_GBps'] = 2.0 * src.numel() * 4 / copy_ms / 1e6
    res['batchnorm_act'] = {}
    for name, shape in (('bn1', (B, 64, H // 2, W // 2)), ('layer2', (B, 128, H // 8, W // 8)), ('layer4', (B, 512, H // 32, W // 32))):
        bn = torch.nn.BatchNorm2d(shape[1]).to(dev).train()
        x, r, dy = (torch.randn(shape, device=dev) for _ in range(3))
        w, bias = bn.weight.detach(), bn.bias.detach()
        # the wrappers of hip/ops.py directly: no autograd node in the timed region (allocation of the outputs included)
        fwd = lambda: ops.batchnorm_act_forward(x, r, w, bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, 0.1,     # noqa: E731
                                                ops.ACT_RELU, True)
        y, stats = fwd()
        bwd = lambda: ops.batchnorm_act_backward(dy, y, x, w, stats, None, None, bn.eps, ops.ACT_RELU, True)      # noqa: E731
        for f in (fwd, bwd):
            for _ in range(3):
                f()
        n = x.numel() * 4
        f_ms = statistics.median(timed(fwd, 20) for _ in range(5))
        b_ms = statistics.median(timed(bwd, 20) for _ in range(5))
        res['batchnorm_act'][name] = {'shape': list(shape), 'path': ops.batchnorm_last_path(),
                                      'forward_us': 1000 * f_ms, 'forward_GBps': 3 * n / f_ms / 1e6,          # x, res -> y
                                      'backward_us': 1000 * b_ms, 'backward_GBps': 5 * n / b_ms / 1e6}        # dy, y, x -> dx, dres
    return res


def step_section(args, B, H, W, dev):
    import resnet_cases as C
    from packnet_sfm.models.SelfSupModel import SelfSupModel
    model, dn, pn = C.our_step(dev)
    twin = C.step_model(SelfSupModel, C.Twin(dn, 'depth'), C.Twin(pn, 'pose'), dev)
    batch = C.step_batch(dev, size=(B, 3, H, W))

    def step(m):
        for p in m.parameters():
            p.grad = None
        random.seed(0)
        out = m(batch, progress=0.0)
        out['loss'].backward()

    for m in (model, twin):
        for _ in range(args.warmup):
            step(m)
    torch.cuda.synchronize()
    ms = {'hip': [], 'eager': []}
    for _ in range(args.repeats):                           # interleaved A/B: the clocks and the box's other tenants hit both alike
        ms['hip'].append(timed(lambda: step(model), args.steps))
        ms['eager'].append(timed(lambda: step(twin), args.steps))
    res = {'steps': args.steps, 'repeats': args.repeats}
    for k, v in ms.items():
        res[k] = {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v), 'images_per_s': B * 1000.0 / statistics.median(v)}
    res['launches_per_step'] = {'hip': launches(lambda: step(model)), 'eager': launches(lambda: step(twin))}
    return res


# (class, [(name, source channels, up factors, Cout, H, W of the gather grid, k, stride, reflect)]) of DepthResNet18 at 192 x 640
def _half_layer_classes(H, W):
    return [
        ('stem 7x7 s2', [('conv1', [3], (1,), 64, H, W, 7, 2, False)]),
        ('3x3 s2', [('layer%d.0.conv1' % (i + 2), [64 << i], (1,), 128 << i, H >> (2 + i), W >> (2 + i), 3, 2, False) for i in range(3)]),
        ('1x1 s2', [('layer%d.0.downsample' % (i + 2), [64 << i], (1,), 128 << i, H >> (2 + i), W >> (2 + i), 1, 2, False) for i in range(3)]),
        ('reflect full resolution', [('upconv(0,1)', [16], (2,), 16, H, W, 3, 1, True), ('dispconv(0)', [16], (1,), 1, H, W, 3, 1, True)]),
        ('512->512 @ 6x20', [('layer4.1.conv1', [512], (1,), 512, H >> 5, W >> 5, 3, 1, False)]),
    ]


def _half_stride_probe(H, W, dev, batch=16):
    """Not a layer of the network: 128 -> 128 channels, 3x3, onto (H / 4) x (W / 4) at batch 16 (enough work to stand clear of the launch
    floor, no K split) at stride 1, at stride 2 with the de-interleaved patch and at stride 2 with the plain one."""
    from packnet_sfm.hip import _lib, ops
    g = torch.Generator().manual_seed(1)
    wt = (torch.randn((128, 128, 3, 3), generator=g) * (2.0 / (128 * 9)) ** 0.5).half().to(dev)
    wp = ops.conv2d_pack_h16(wt)
    out = {}
    for name, stride, deint in (('stride 1', 1, 1), ('stride 2, de-interleaved', 2, 1), ('stride 2, plain rows', 2, 0)):
        x = torch.randn((batch, 128, (H >> 2) * stride, (W >> 2) * stride), generator=g).half().to(dev)
        y = torch.empty((batch, 128, H >> 2, W >> 2), dtype=torch.float16, device=dev)
        was = _lib.get().pnsfm_set_h16g_deinterleave(deint)
        split = _lib.get().pnsfm_set_h16_max_split(1)
        try:
            f = lambda: ops.conv2d_forward_h16g([x], wp, 128, 3, stride=stride, out=y)      # noqa: E731
            for _ in range(5):
                f()
            cfg = ops.conv2d_last_config()
            t_ms = statistics.median(timed(f, 50) for _ in range(7))
        finally:
            _lib.get().pnsfm_set_h16g_deinterleave(was)
            _lib.get().pnsfm_set_h16_max_split(split)
        out[name] = {'us': 1000 * t_ms, 'TFLOPs': 2.0 * y.numel() * 128 * 9 / t_ms / 1e9, 'config': cfg}
    return out


def half_section(args, H, W, dev):
    """DepthResNet18 eval forward, batch 1 and 4: fp16 on the gathering kernels | this tree's fp32 path | the ATen twin in fp16, alternating
    in windows in one process; launches per forward; achieved TFLOP/s of conv2d_h16g (variant 10) per layer class at batch 1."""
    import resnet_cases as C
    from packnet_sfm.hip import ops
    res = {'forward': {}, 'layer_classes': {}}
    for B in (1, 4):
        net32 = C.make_depth_net(dev).eval()
        net16 = C.make_depth_net(dev, dtype=torch.float16).eval()
        rgb = C.frames((B, 3, H, W))[0].to(dev)
        rgb16 = rgb.half()
        runs = {'hip_fp16': lambda: net16(rgb16), 'hip_fp32': lambda: net32(rgb), 'eager_fp16': lambda: C.torch_forward(net16, rgb16)}
        with torch.no_grad():
            for f in runs.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(args.repeats):
                for k, f in runs.items():
                    ms[k].append(timed(f, args.steps))
            entry = {k: {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v),
                         'images_per_s': B * 1000.0 / statistics.median(v)} for k, v in ms.items()}
            entry['launches_per_forward'] = {k: launches(f) for k, f in runs.items()}
        res['forward']['batch%d' % B] = entry
    g = torch.Generator().manual_seed(0)
    for cls, layers in _half_layer_classes(H, W):
        out = []
        for name, chans, ups, Cout, h, w, ks, stride, reflect in layers:
            xs = [torch.randn((1, c, h // u, w // u), generator=g).half().to(dev) for c, u in zip(chans, ups)]
            wt = (torch.randn((Cout, sum(chans), ks, ks), generator=g) * (2.0 / (sum(chans) * ks * ks)) ** 0.5).half().to(dev)
            wp = ops.conv2d_pack_h16(wt)
            sc, sh = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
            y = torch.empty(ops.conv2d_h16g_out_shape(xs, ups, Cout, ks, stride), dtype=torch.float16, device=dev)
            f = lambda: ops.conv2d_forward_h16g(xs, wp, Cout, ks, stride=stride, reflect=reflect, ups=ups, scale=sc, shift=sh,      # noqa: E731
                                                act=ops.ACT_RELU, out=y)
            for _ in range(5):
                f()
            cfg = ops.conv2d_last_config()
            t_ms = statistics.median(timed(f, 50) for _ in range(5))
            flops = 2.0 * y.numel() * sum(chans) * ks * ks
            out.append({'layer': name, 'in': chans, 'up': list(ups), 'out': Cout, 'grid': [h, w], 'k': ks, 'stride': stride,
                        'reflect': reflect, 'us': 1000 * t_ms, 'TFLOPs': flops / t_ms / 1e9, 'config': cfg})
        res['layer_classes'][cls] = out
    res['stride_probe_batch16'] = _half_stride_probe(H, W, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--size', type=int, nargs=3, default=[4, 192, 640])
    ap.add_argument('--section', choices=['all', 'bn', 'step', 'half'], default='all')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, H, W = args.size
    res = {'size': [B, 3, H, W]}
    if args.section in ('all', 'bn'):                       # first: it depends on nothing but its own kernels
        res.update(bn_section(B, H, W, dev))
    if args.section in ('all', 'step'):
        res['step'] = step_section(args, B, H, W, dev)
    if args.section == 'half':                              # its own run: 'all' stays the training sections
        res['half'] = half_section(args, H, W, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
