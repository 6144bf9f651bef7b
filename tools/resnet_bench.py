"""What the ResNet networks cost on the MI355X.

    python tools/resnet_bench.py [--section all|bn|step] [--steps 10] [--repeats 7] [--out profiles/resnet_bench.json]

Step = forward + backward of SelfSupModel(DepthResNet18, PoseResNet18) at 192x640, batch 4, against the eager twin
(tests/resnet_cases.torch_forward: the same parameters through ATen) in the same process: the two alternate in windows of --steps steps,
each window timed with device events after --warmup untimed steps, medians over --repeats windows.  Launches per step are counted with
the kernel profiler's device-activity events.  For batchnorm_act forward and backward at bn1's [4,64,96,320] and layer4's [4,512,6,20]
it reports the achieved bytes/s (one read of every input, one write of every output) next to pnsfm_calib_copy's rate in the same run.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--size', type=int, nargs=3, default=[4, 192, 640])
    ap.add_argument('--section', choices=['all', 'bn', 'step'], default='all')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, H, W = args.size
    res = {'size': [B, 3, H, W]}
    if args.section in ('all', 'bn'):                       # first: it depends on nothing but its own kernels
        res.update(bn_section(B, H, W, dev))
    if args.section in ('all', 'step'):
        res['step'] = step_section(args, B, H, W, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
