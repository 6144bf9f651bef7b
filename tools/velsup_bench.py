"""What velocity supervision costs a training step on the MI355X.

    python tools/velsup_bench.py                       # step time of VelSupModel against SelfSupModel, one JSON line
    python tools/velsup_bench.py --trace selfsup       # a few steps of one model and nothing else: run it under a kernel trace
    python tools/velsup_bench.py --trace velsup        #   (rocprofv3 --kernel-trace --stats) and subtract the two kernel tables

Step = forward + backward of the model (PackNet01 + PoseNet + loss) at 192x640, batch 4, the two models sharing their parameters.
Timing: one process, the two models alternating in windows of --steps steps, host clock around a window that ends in a device
synchronise, --repeats windows each; the medians and the spread of each model's windows are reported next to the box's calibration
figure (bench.box_calibration).  Ground-truth poses arrive as float64 [B,4,4] tensors on the device, as a dataset delivers them."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'packnet-sfm_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def build(device):
    import bench
    from packnet_sfm.models.VelSupModel import VelSupModel
    base = bench.build_model(device)
    kw = {**bench.LOSS_DEFAULTS, 'flip_lr_prob': 0.0}
    base.flip_lr_prob = 0.0
    vel = VelSupModel(velocity_loss_weight=0.1, **kw)
    vel.add_depth_net(base.depth_net)                   # the same parameters: the two steps differ by the velocity term only
    vel.add_pose_net(base.pose_net)
    return base, vel.to(device).train()


def batch_of(B, H, W, device):
    import bench
    batch = bench.synthetic_batch(B, H, W, 1234, device)
    g = torch.Generator().manual_seed(7)
    poses = []
    for _ in range(2):
        T = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
        T[:, :3, 3] = 0.1 * torch.randn(B, 3, generator=g, dtype=torch.float64)
        poses.append(T.to(device))
    batch['pose_context'] = poses
    return batch


def step(model, batch):
    for p in model.parameters():
        p.grad = None
    out = model(batch, progress=0.0)
    out['loss'].backward()
    return out['loss']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40, help='steps per timed window')
    ap.add_argument('--repeats', type=int, default=7, help='windows per model')
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--trace', choices=('selfsup', 'velsup'), help='run --steps steps of one model only (for a kernel trace)')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=192)
    ap.add_argument('--width', type=int, default=640)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs an MI355X'
    device = torch.device('cuda:0')
    random.seed(0)
    base, vel = build(device)
    batch = batch_of(args.batch, args.height, args.width, device)
    models = {'selfsup': base, 'velsup': vel}
    if args.trace:
        for _ in range(args.warmup + args.steps):
            step(models[args.trace], batch)
        torch.cuda.synchronize()
        print(json.dumps({'traced': args.trace, 'steps': args.warmup + args.steps}))
        return
    for _ in range(args.warmup):
        for m in models.values():
            step(m, batch)
    torch.cuda.synchronize()
    import bench
    calib = bench.box_calibration(device)
    ms = {k: [] for k in models}
    for _ in range(args.repeats):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(m, batch)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    loss = {k: float(step(m, batch)) for k, m in models.items()}
    out = {'what': 'forward + backward step, ms; windows of %d steps, %d per model, alternating' % (args.steps, args.repeats),
           'shape': [args.batch, args.height, args.width], 'date': time.strftime('%Y-%m-%d'), 'loss': loss,
           'box': {k: calib[k] for k in ('mfma_tflops', 'hbm_gbps')}}
    for k, v in ms.items():
        out[k] = {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4),
                  'windows_ms': [round(x, 4) for x in v]}
    out['velsup_minus_selfsup_ms'] = round(out['velsup']['median_ms'] - out['selfsup']['median_ms'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
