"""Cases, input builders and the ATen twin of the ResNet networks (DepthResNet / PoseResNet and the kernels of csrc/resnet.h), shared by
tests/test_resnet_emulated.py (CPU, host emulator), tests/test_gpu_resnet.py (MI355X), tools/make_resnet_golden.py (the fixture) and
tools/resnet_bench.py (the eager baseline).

Tolerances
  data movement (max pool, reflection pad, crop)   bit-equal to ATen; inputs and upstream gradients are small integers, so every sum
                                                   is exact.
  batchnorm_act, act_crop                          the oracle is ATen in fp64.  The bound of a tensor is 4 x the largest error ATen's own
                                                   fp32 CPU run makes against that oracle on the same input, floored at one fp32 ulp of
                                                   the oracle's largest magnitude.  The ATen error is measured in every run.
  networks                                         the project's network tolerances (tests/parity_cases.py, network.pt): outputs 1e-3 of
                                                   the tensor's maximum, gradient norms 5e-3 max(ref, 1e-3 gmax), gradient samples 1e-2
                                                   with the floor of case_packnet01; running statistics 1e-4 of their maximum.
  step                                             those of tests/test_gpu_velsup.py: loss 1e-4 relative, smoothness 1e-3, depth 1e-3,
                                                   gradient norms 1e-2 max(ref, 1e-4 gmax).
"""
import copy
import math
import os
import random

import pytest
import torch
import torch.nn.functional as F

import parity_cases as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet.pt')
SIZE = (2, 3, 64, 96)               # the fixture's frames (tools/make_resnet_golden.py states why this size is enough)
DEPTH_SEED, POSE_SEED, FRAME_SEED, WEIGHT_SEED = 101, 102, 103, 104
OUT_TOL, GNORM_TOL, GSAMPLE_TOL, STAT_TOL = 1e-3, 5e-3, 1e-2, 1e-4
_fx = {}


def fixture():
    if 'fx' not in _fx:
        _fx['fx'] = torch.load(GOLD, weights_only=False)
    return _fx['fx']


# ------------------------------------------------------------------------------------------------ builders (shapes -> tensors)
def build_params(shapes, seed):
    """name -> shape (a state dict's) -> name -> tensor, from one seeded generator, names in sorted order.  Convolutions and the linear
    layer: N(0, 2 / fan_in); BatchNorm weight 1 + 0.1 N, bias 0.1 N, running_mean 0.1 N, running_var in [0.5, 1.5]; conv biases 0.05 N."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        leaf = name.rsplit('.', 1)[-1]
        if leaf == 'num_batches_tracked':
            out[name] = torch.zeros(shape, dtype=torch.int64)
        elif leaf == 'running_var':
            out[name] = 0.5 + torch.rand(shape, generator=g)
        elif leaf == 'running_mean':
            out[name] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            out[name] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
        elif leaf == 'weight':              # BatchNorm
            out[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif '.bn' in name or 'downsample.1' in name:
            out[name] = 0.1 * torch.randn(shape, generator=g)
        else:
            out[name] = 0.05 * torch.randn(shape, generator=g)
    return out


def frames(size=SIZE, seed=FRAME_SEED):
    """(rgb, [context 0, context 1]): smooth seeded images in [0, 1], the contexts the same scene shifted by two pixels either way."""
    B, C, H, W = size
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((B, C, H // 8, (W + 8) // 8), generator=g)
    base = F.interpolate(coarse, size=(H, W + 8), mode='bilinear', align_corners=True)
    base = (base + 0.05 * torch.rand(base.shape, generator=g)).clamp(0.0, 1.0)
    return base[..., 4:W + 4].contiguous(), [base[..., 2:W + 2].contiguous(), base[..., 6:W + 6].contiguous()]


def out_weights(shapes, seed=WEIGHT_SEED):
    """The fixed scalar of a network's outputs is sum_i (out_i * w_i).sum() with these seeded weights."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(s), generator=g) for s in shapes]


def state_shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def make_depth_net(device, version='18', seed=DEPTH_SEED, dtype=torch.float32):
    from packnet_sfm.networks.depth.DepthResNet import DepthResNet
    net = DepthResNet(version=version)
    net.load_state_dict(build_params(state_shapes(net), seed))
    return net.to(device=device, dtype=dtype)


def make_pose_net(device, seed=POSE_SEED, dtype=torch.float32):
    from packnet_sfm.networks.pose.PoseResNet import PoseResNet
    net = PoseResNet(version='18')
    net.load_state_dict(build_params(state_shapes(net), seed))
    return net.to(device=device, dtype=dtype)


# ------------------------------------------------------------------------------------------------ the twin: plain ATen
def _t_bn(x, bn):
    if bn.training:
        bn.num_batches_tracked += 1
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)


def _t_block(x, blk):
    out = F.relu(_t_bn(F.conv2d(x, blk.conv1.weight, None, blk.stride, 1), blk.bn1))
    out = _t_bn(F.conv2d(out, blk.conv2.weight, None, 1, 1), blk.bn2)
    if blk.downsample is not None:
        x = _t_bn(F.conv2d(x, blk.downsample[0].weight, None, blk.downsample[0].stride), blk.downsample[1])
    return F.relu(out + x)


def _t_encoder(enc, image):
    e = enc.encoder
    x = (image - 0.45) / 0.225
    feats = [F.relu(_t_bn(F.conv2d(x, e.conv1.weight, None, 2, 3), e.bn1))]
    x = F.max_pool2d(feats[-1], 3, 2, 1)
    for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
        for blk in layer:
            x = _t_block(x, blk)
        feats.append(x)
    return feats


def _t_conv3x3(c3, x):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), c3.conv.weight, c3.conv.bias)


def _t_depth_decoder(dec, feats):
    convs = list(dec.decoder)
    up = {(i, j): convs[2 * (4 - i) + j] for i in range(5) for j in range(2)}
    disp = {s: convs[10 + k] for k, s in enumerate(range(4))}
    out = {}
    x = feats[-1]
    for i in range(4, -1, -1):
        x = F.elu(_t_conv3x3(up[(i, 0)].conv, x))
        x = [F.interpolate(x, scale_factor=2, mode='nearest')]
        if i > 0:
            x += [feats[i - 1]]
        x = F.elu(_t_conv3x3(up[(i, 1)].conv, torch.cat(x, 1)))
        if i in disp:
            out[i] = torch.sigmoid(_t_conv3x3(disp[i], x))
    return out


def _t_pose_decoder(dec, feats):
    net = list(dec.net)
    x = F.relu(F.conv2d(feats[-1], net[0].weight, net[0].bias))
    x = F.relu(F.conv2d(x, net[1].weight, net[1].bias, 1, 1))
    x = F.relu(F.conv2d(x, net[2].weight, net[2].bias, 1, 1))
    x = F.conv2d(x, net[3].weight, net[3].bias)
    x = 0.01 * x.mean(3).mean(2).view(-1, dec.num_frames_to_predict_for, 1, 6)
    return x[..., :3], x[..., 3:]


def torch_forward(module, *inputs):
    """`module`'s OWN parameters and buffers run through plain ATen (F.conv2d, F.batch_norm, F.max_pool2d, F.pad(mode='reflect'), F.elu,
    F.interpolate) with the reference's forward semantics.  DepthResNet: (rgb) -> the list of four scaled disparities in training mode, the
    full-resolution one in eval mode.  PoseResNet: (target, [contexts]) -> [B, n, 6].  Running statistics are updated as F.batch_norm does."""
    kind = type(module).__name__
    if kind == 'DepthResNet':
        disps = _t_depth_decoder(module.decoder, _t_encoder(module.encoder, inputs[0]))
        scaled = [1 / 100.0 + (1 / 0.1 - 1 / 100.0) * disps[i] for i in range(4)]
        return scaled if module.training else scaled[0]
    if kind == 'PoseResNet':
        target, refs = inputs
        outs = []
        for ref in refs:
            axisangle, translation = _t_pose_decoder(module.decoder, _t_encoder(module.encoder, torch.cat([target, ref], 1)))
            outs.append(torch.cat([translation[:, 0], axisangle[:, 0]], 2))
        return torch.cat(outs, 1)
    raise TypeError('torch_forward: no twin for %s' % kind)


class Twin(torch.nn.Module):
    """A module whose forward is torch_forward of a deep copy of `module` (for SelfSupModel.add_depth_net / add_pose_net)."""

    def __init__(self, module, kind):
        super().__init__()
        self.net = copy.deepcopy(module)
        self.kind = kind

    def forward(self, *args, **kwargs):
        if self.kind == 'depth':
            rgb = args[0] if args else kwargs['rgb']
            return {'inv_depths': torch_forward(self.net, rgb)}
        return torch_forward(self.net, *args)


# ------------------------------------------------------------------------------------------------ the 4 x ATen rule
def ulp(v):
    v = abs(float(v))
    return 2.0 ** -149 if v < 2.0 ** -126 else 2.0 ** (math.floor(math.log2(v)) - 23)


def within_4x_aten(got, oracle64, aten32, what):
    """|got - oracle| <= max(4 x max |ATen fp32 - oracle|, one fp32 ulp of max |oracle|), the figures printed before the assertion."""
    o = oracle64.detach().double().cpu()
    e_aten = float((aten32.detach().double().cpu() - o).abs().max()) if o.numel() else 0.0
    e_got = float((got.detach().double().cpu() - o).abs().max()) if o.numel() else 0.0
    floor = ulp(float(o.abs().max())) if o.numel() else 0.0
    bound = max(4.0 * e_aten, floor)
    print('%-28s err %.3e  aten %.3e  floor %.3e  err/aten %s' % (what, e_got, e_aten, floor, ('%.2f' % (e_got / e_aten)) if e_aten else '-'))
    assert tuple(got.shape) == tuple(o.shape), '%s: shape %s vs %s' % (what, tuple(got.shape), tuple(o.shape))
    assert e_got <= bound, '%s: error %.3e > bound %.3e (ATen fp32 error %.3e, ulp floor %.3e)' % (what, e_got, bound, e_aten, floor)
    return e_got, e_aten


def _leaf(t, where):
    """A fresh leaf copy of `t` on a device or in a dtype (Tensor.to returns `t` itself where nothing changes)."""
    return t.detach().to(where).clone().requires_grad_(True)


def _ints(shape, seed, lo=-4, hi=5):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


# ------------------------------------------------------------------------------------------------ data movement: bit-equal
POOL_SHAPES = [(1, 1, 1), (2, 2, 2), (3, 5, 7), (2, 6, 20), (1, 33, 65)]
POOL_KINDS = ['ints', 'zeros', 'repeat']
PAD_SHAPES = [(1, 2, 2), (3, 2, 3), (2, 5, 7), (2, 6, 20), (1, 33, 65)]


def maxpool_case(device, shape, kind):
    from packnet_sfm.hip import functional as HF
    N, h, w = shape
    if kind == 'zeros':
        x = torch.zeros(1, N, h, w)
    elif kind == 'repeat':                         # two values in a period-3 pattern: every window holds its maximum several times
        x = ((torch.arange(N * h * w) % 3) == 1).float().view(1, N, h, w)
    else:
        x = _ints((1, N, h, w), 7)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    dy = _ints(tuple(yr.shape), 8, 1, 6)
    yr.backward(dy)
    xh = _leaf(x, device)
    y = HF.maxpool3x3s2(xh)
    y.backward(dy.to(device))
    assert torch.equal(y.detach().cpu(), yr.detach()), 'max pool forward %s %s' % (shape, kind)
    assert torch.equal(xh.grad.cpu(), xr.grad), 'max pool backward %s %s (tie rule)' % (shape, kind)


def _ref_pad(x, s):
    if s == 2:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    return F.pad(x, (1, 1, 1, 1), mode='reflect')


def pad_case(device, shape, s):
    from packnet_sfm.hip import functional as HF
    N, h, w = shape
    x = _ints((1, N, h, w), 9)
    xr = x.clone().requires_grad_(True)
    yr = _ref_pad(xr, s)
    dy = _ints(tuple(yr.shape), 10)
    yr.backward(dy)
    xh = _leaf(x, device)
    y = HF.reflect_pad1(xh, s)
    y.backward(dy.to(device))
    assert torch.equal(y.detach().cpu(), yr.detach()), 'reflect pad forward %s s=%d' % (shape, s)
    assert torch.equal(xh.grad.cpu(), xr.grad), 'reflect pad backward %s s=%d' % (shape, s)


def pad_cat_case(device):
    """Two sources into one output: the up-sampled one in front, the skip behind (the decoder's second convolution)."""
    from packnet_sfm.hip import functional as HF
    a, b = _ints((2, 3, 3, 5), 11), _ints((2, 2, 6, 10), 12)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.cat([_ref_pad(ar, 2), _ref_pad(br, 1)], 1)
    dy = _ints(tuple(yr.shape), 13)
    yr.backward(dy)
    ah, bh = _leaf(a, device), _leaf(b, device)
    y = HF.reflect_pad1((ah, bh), (2, 1))
    y.backward(dy.to(device))
    assert torch.equal(y.detach().cpu(), yr.detach())
    assert torch.equal(ah.grad.cpu(), ar.grad) and torch.equal(bh.grad.cpu(), br.grad)
    with pytest.raises(ValueError):
        HF.reflect_pad1((ah, bh), (1, 1))


def pad_pitch_case(device):
    """A row pitch wider than the padded map: the map itself as before, zero columns behind it, and they send no gradient back; the
    matching act_crop(width=...) reads the interior only and writes zero gradients into the rest."""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    x = _ints((2, 3, 4, 5), 18)
    xr = x.clone().requires_grad_(True)
    yr = _ref_pad(xr, 2)                                   # [2, 3, 10, 12]
    dy = _ints((2, 3, 10, 32), 19)
    yr.backward(dy[..., :12])
    xh = _leaf(x, device)
    y = HF.reflect_pad1(xh, 2, pitch=32)
    y.backward(dy.to(device))
    assert tuple(y.shape) == (2, 3, 10, 32) and torch.equal(y.detach().cpu()[..., :12], yr.detach()) and bool((y[..., 12:] == 0).all())
    assert torch.equal(xh.grad.cpu(), xr.grad)
    z, g = _ints((2, 3, 10, 32), 20), _ints((2, 3, 8, 10), 21)
    zh = _leaf(z, device)
    c = HF.act_crop(zh, 1, ops.ACT_NONE, width=10)
    c.backward(g.to(device))
    assert torch.equal(c.detach().cpu(), z[..., 1:9, 1:11])
    assert torch.equal(zh.grad.cpu(), F.pad(g, (1, 21, 1, 1)))


def conv3x3_wide_case(device, shape=(1, 16, 4, 640), cout=16):
    """A map whose padded width (642) the convolution kernels do not tile: conv3x3_reflect pads to a pitch of 672.  Against ATen in fp64
    with the project's layer tolerances (tests/parity_cases.py: outputs 1e-4 of the maximum, gradients 5e-4)."""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    g = torch.Generator().manual_seed(26)
    x, w, b = torch.randn(shape, generator=g), 0.1 * torch.randn((cout, shape[1], 3, 3), generator=g), 0.1 * torch.randn(cout, generator=g)
    dy = torch.randn((shape[0], cout) + tuple(shape[2:]), generator=g)
    xr, wr, br = (_leaf(t, torch.float64) for t in (x, w, b))
    yr = F.elu(F.conv2d(F.pad(xr, (1, 1, 1, 1), mode='reflect'), wr, br))
    yr.backward(dy.double())
    xh, wh, bh = (_leaf(t, device) for t in (x, w, b))
    y = HF.conv3x3_reflect(xh, wh, bh, HF.PackedConvWeight(), act=ops.ACT_ELU)
    y.backward(dy.to(device))
    P.check(y.detach().cpu().double(), yr.detach(), 1e-4, 'wide conv3x3 forward')
    for got, ref, what in ((xh.grad, xr.grad, 'dx'), (wh.grad, wr.grad, 'dw'), (bh.grad, br.grad, 'db')):
        P.check(got.cpu().double(), ref, 5e-4, 'wide conv3x3 ' + what)


def pad_too_small_case(device):
    from packnet_sfm.hip import functional as HF
    x = _ints((1, 1, 1, 2), 14).to(device)
    with pytest.raises(RuntimeError, match='Padding size should be less than the corresponding input dimension'):
        HF.reflect_pad1(x, 1)
    with pytest.raises(RuntimeError):
        F.pad(x.cpu(), (1, 1, 1, 1), mode='reflect')
    assert torch.equal(HF.reflect_pad1(x, 2).cpu(), _ref_pad(x.cpu(), 2))


def crop_case(device, shape, m):
    """The crop of act_crop alone (no activation): exact."""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    B, C, H, W = shape
    z = _ints((B, C, H + 2 * m, W + 2 * m), 15)
    dy = _ints((B, C, H, W), 16)
    zh = _leaf(z, device)
    y = HF.act_crop(zh, m, ops.ACT_NONE)
    y.backward(dy.to(device))
    assert torch.equal(y.detach().cpu(), z[..., m:m + H, m:m + W])
    assert torch.equal(zh.grad.cpu(), F.pad(dy, (m, m, m, m)))


def affine_case(device, n):
    """x s + t and its gradient, one fused multiply-add each: within one fp32 ulp of the fp64 value (n = 7: the scalar kernel, 8 and
    4096: the float4 one)."""
    from packnet_sfm.hip import functional as HF
    x = torch.rand(n, generator=torch.Generator().manual_seed(27))
    s_, t_ = 1.0 / 0.225, -0.45 / 0.225
    xh = _leaf(x, device)
    y = HF.affine(xh, s_, t_)
    y.backward(torch.ones_like(y) * 3.0)
    ref = x.double() * float(torch.tensor(s_)) + float(torch.tensor(t_))
    assert float((y.detach().cpu().double() - ref).abs().max()) <= ulp(float(ref.abs().max()))
    assert float((xh.grad.cpu().double() - 3.0 * float(torch.tensor(s_))).abs().max()) <= ulp(3.0 * s_)


# ------------------------------------------------------------------------------------------------ act_crop: 4 x ATen
CROP_SHAPES = [(1, 1, 1, 1), (2, 3, 2, 3), (2, 16, 6, 20)]
DISP_RANGE = (0.01, 9.99)


def _ref_act(z, act):
    from packnet_sfm.hip import ops
    if act == ops.ACT_ELU:
        return F.elu(z)
    if act == ops.ACT_RELU:
        return F.relu(z)
    return DISP_RANGE[0] + DISP_RANGE[1] * torch.sigmoid(z)


def act_crop_case(device, shape, act, m):
    from packnet_sfm.hip import functional as HF
    B, C, H, W = shape
    g = torch.Generator().manual_seed(17)
    z = 2.0 * torch.randn((B, C, H + 2 * m, W + 2 * m), generator=g)
    dy = torch.randn((B, C, H, W), generator=g)
    res = []
    for dt in (torch.float64, torch.float32):
        zr = _leaf(z, dt)
        yr = _ref_act(zr[..., m:m + H, m:m + W], act)
        yr.backward(dy.to(dt))
        res.append((yr.detach(), zr.grad))
    zh = _leaf(z, device)
    y = HF.act_crop(zh, m, act, DISP_RANGE)
    y.backward(dy.to(device))
    within_4x_aten(y, res[0][0], res[1][0], 'act_crop y act=%d m=%d' % (act, m))
    within_4x_aten(zh.grad, res[0][1], res[1][1], 'act_crop dz act=%d m=%d' % (act, m))
    if m:
        frame = zh.grad.clone()
        frame[..., m:m + H, m:m + W] = 0
        assert bool((zh.grad[..., 0, :] == 0).all()) and bool((frame == 0).all()), 'dz must be zero outside the crop'


# ------------------------------------------------------------------------------------------------ batchnorm_act: 4 x ATen
# (shape, path of the training forward and of the backward): 0 one workgroup per channel, 1 per-(channel, chunk) partials.  The switch
# is at 2048 units per channel, a unit being a float4 where H W % 4 == 0 and a float otherwise: one shape on each side for both forms.
BN_SHAPES = [((2, 1, 1, 1), 0), ((1, 3, 1, 5), 0), ((3, 5, 3, 7), 0), ((2, 64, 2, 3), 0), ((2, 16, 33, 65), 1),
             ((2, 2, 64, 64), 0),       # float4 units: 2 * 4096 / 4 = 2048, the last fused size
             ((2, 2, 64, 68), 1),       # 2176 units
             ((2, 3, 31, 33), 0),       # odd plane, scalar units: 2046
             ((2, 3, 25, 41), 1)]       # 2050
BN_BIG = (1, 1, 512, 1028)              # 131584 float4 units: more than 64 chunks of 2048, so the chunks grow (path 1)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn_inputs(shape, seed, mean=0.5):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    return dict(x=mean + 1.5 * torch.randn(shape, generator=g), res=torch.randn(shape, generator=g), dy=torch.randn(shape, generator=g),
                gamma=1.0 + 0.2 * torch.randn(C, generator=g), beta=0.3 * torch.randn(C, generator=g),
                rm=0.1 * torch.randn(C, generator=g), rv=0.5 + torch.rand(C, generator=g))


def _bn_aten(d, dt, use_res, relu, training, steps=1):
    x, g, b = (_leaf(d[k], dt) for k in ('x', 'gamma', 'beta'))
    r = _leaf(d['res'], dt) if use_res else None
    rm, rv = d['rm'].to(dt).clone(), d['rv'].to(dt).clone()
    for _ in range(steps):
        y = F.batch_norm(x, rm, rv, g, b, training, BN_MOMENTUM, BN_EPS)
    if use_res:
        y = y + r
    if relu:
        y = F.relu(y)
    y.backward(d['dy'].to(dt))
    return dict(y=y.detach(), dx=x.grad, dres=r.grad if use_res else None, dgamma=g.grad, dbeta=b.grad, rm=rm, rv=rv)


def _bn_module(d, device, training):
    bn = torch.nn.BatchNorm2d(d['gamma'].numel(), eps=BN_EPS, momentum=BN_MOMENTUM)
    bn.load_state_dict({'weight': d['gamma'], 'bias': d['beta'], 'running_mean': d['rm'], 'running_var': d['rv'],
                        'num_batches_tracked': torch.tensor(0)})
    return bn.to(device).train(training)


def _bn_units(shape):
    B, _, H, W = shape
    return B * H * W // 4 if (H * W) % 4 == 0 else B * H * W


def bn_case(device, shape, path, use_res, relu, training, mean=0.5, seed=21):
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    assert (_bn_units(shape) <= ops.BN_FUSE_UNITS) == (path == 0), 'the case table does not match the documented switch'
    d = _bn_inputs(shape, seed, mean)
    o64, a32 = (_bn_aten(d, dt, use_res, relu, training) for dt in (torch.float64, torch.float32))
    bn = _bn_module(d, device, training)
    x = _leaf(d['x'], device)
    r = _leaf(d['res'], device) if use_res else None
    y = HF.batchnorm_act(x, bn, ops.ACT_RELU if relu else ops.ACT_NONE, res=r)
    assert ops.batchnorm_last_path() == (path if training else ops.BN_PATH_EVAL), 'forward path %d' % ops.batchnorm_last_path()
    y.backward(d['dy'].to(device))
    assert ops.batchnorm_last_path() == path, 'backward path %d' % ops.batchnorm_last_path()
    tag = '%s res=%d relu=%d train=%d ' % ('x'.join(map(str, shape)), use_res, relu, training)
    ratios = [within_4x_aten(y, o64['y'], a32['y'], tag + 'y'), within_4x_aten(x.grad, o64['dx'], a32['dx'], tag + 'dx'),
              within_4x_aten(bn.weight.grad, o64['dgamma'], a32['dgamma'], tag + 'dgamma'),
              within_4x_aten(bn.bias.grad, o64['dbeta'], a32['dbeta'], tag + 'dbeta')]
    if use_res:
        ratios.append(within_4x_aten(r.grad, o64['dres'], a32['dres'], tag + 'dres'))
    ratios.append(within_4x_aten(bn.running_mean, o64['rm'], a32['rm'], tag + 'running_mean'))
    ratios.append(within_4x_aten(bn.running_var, o64['rv'], a32['rv'], tag + 'running_var'))
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    if not training:
        assert torch.equal(bn.running_mean.cpu(), d['rm']) and torch.equal(bn.running_var.cpu(), d['rv'])
    return ratios


def bn_two_steps_case(device, shape=(3, 5, 3, 7)):
    """Running statistics and the step counter after two training steps on the same input."""
    from packnet_sfm.hip import functional as HF
    d = _bn_inputs(shape, 22)
    o64, a32 = (_bn_aten(d, dt, False, False, True, steps=2) for dt in (torch.float64, torch.float32))
    bn = _bn_module(d, device, True)
    with torch.no_grad():
        for _ in range(2):
            HF.batchnorm_act(d['x'].to(device), bn)
    within_4x_aten(bn.running_mean, o64['rm'], a32['rm'], 'two steps running_mean')
    within_4x_aten(bn.running_var, o64['rv'], a32['rv'], 'two steps running_var')
    assert int(bn.num_batches_tracked) == 2 and bn.num_batches_tracked.dtype == torch.int64


def bn_single_value_case(device):
    from packnet_sfm.hip import functional as HF
    d = _bn_inputs((1, 4, 1, 1), 23)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        HF.batchnorm_act(d['x'].to(device), _bn_module(d, device, True))
    y = HF.batchnorm_act(d['x'].to(device), _bn_module(d, device, False))
    ref = F.batch_norm(d['x'].double(), d['rm'].double(), d['rv'].double(), d['gamma'].double(), d['beta'].double(), False, 0.1, BN_EPS)
    within_4x_aten(y, ref, F.batch_norm(d['x'], d['rm'], d['rv'], d['gamma'], d['beta'], False, 0.1, BN_EPS), 'single value, eval')


def bn_reproducible_case(device, shape):
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    d = _bn_inputs(shape, 24)
    runs = []
    for _ in range(2):
        bn = _bn_module(d, device, True)
        x, r = _leaf(d['x'], device), _leaf(d['res'], device)
        y = HF.batchnorm_act(x, bn, ops.ACT_RELU, res=r)
        y.backward(d['dy'].to(device))
        runs.append([y.detach(), x.grad, r.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ networks
def depth_scalar(disps, device):
    ws = out_weights([tuple(d.shape) for d in disps])
    return sum((d * w.to(device=device, dtype=d.dtype)).sum() for d, w in zip(disps, ws))


def pose_scalar(pose, device):
    return (pose * out_weights([tuple(pose.shape)], WEIGHT_SEED + 1)[0].to(device=device, dtype=pose.dtype)).sum()


def grad_record(named):
    """What the fixture keeps of a set of gradients: the norm and 8 evenly spaced samples of each (parameters without one are skipped)."""
    norms, samples = {}, {}
    for n, p in named:
        if p.grad is None:
            continue
        g = p.grad.detach().float().cpu()
        norms[n] = float(g.double().norm())
        samples[n] = g.flatten()[:: max(1, g.numel() // 8)][:8].clone()
    return norms, samples


def check_grads(named, norms, samples, what, norm_tol=GNORM_TOL, rel_floor=1e-3):
    named = [(n, p) for n, p in named if p.grad is not None]
    assert sorted(n for n, _ in named) == sorted(norms), '%s: the set of parameters with a gradient differs' % what
    gmax = max(norms.values())
    worst = 0.0
    for n, p in named:
        ref, got = norms[n], float(p.grad.detach().double().norm())
        scale = max(ref, rel_floor * gmax)
        worst = max(worst, abs(got - ref) / scale)
        assert abs(got - ref) <= norm_tol * scale, '%s grad norm %s: %.6e vs %.6e' % (what, n, got, ref)
        if samples is not None:
            gs = p.grad.detach().float().cpu().flatten()[:: max(1, p.numel() // 8)][:8]
            P.check(gs, samples[n], GSAMPLE_TOL, '%s grad samples %s' % (what, n), floor=max(ref / max(p.numel(), 1) ** 0.5, 1e-6 * gmax))
    print('%s: worst gradient-norm deviation / scale %.2e' % (what, worst))


def _stats_of(net):
    e = net.encoder.encoder
    return {'bn1.running_mean': e.bn1.running_mean, 'bn1.running_var': e.bn1.running_var,
            'layer4.1.bn2.running_mean': e.layer4[1].bn2.running_mean, 'layer4.1.bn2.running_var': e.layer4[1].bn2.running_var}


def depth_record(run, net, device):
    """One training step of a depth network (`run(rgb)` -> four disparities) and the eval output after it, as the fixture stores them."""
    rgb = frames()[0].to(device=device, dtype=next(net.parameters()).dtype)
    net.train()
    disps = run(rgb)
    depth_scalar(disps, device).backward()
    norms, samples = grad_record(net.named_parameters())
    rec = dict(inv_depths=[d.detach().float().cpu() for d in disps], grad_norms=norms, grad_samples=samples,
               stats={k: v.detach().float().cpu().clone() for k, v in _stats_of(net).items()},
               num_batches_tracked=int(net.encoder.encoder.bn1.num_batches_tracked))
    net.eval()
    with torch.no_grad():
        rec['eval'] = run(rgb).detach().float().cpu()
    return rec


def pose_record(run, net, device):
    rgb, ctx = frames()
    dt = next(net.parameters()).dtype
    net.train()
    pose = run(rgb.to(device=device, dtype=dt), [c.to(device=device, dtype=dt) for c in ctx])
    pose_scalar(pose, device).backward()
    norms, samples = grad_record(net.named_parameters())
    return dict(pose=pose.detach().float().cpu(), grad_norms=norms, grad_samples=samples)


def check_depth(rec, ref, what, tol=OUT_TOL):
    for i, (a, b) in enumerate(zip(rec['inv_depths'], ref['inv_depths'])):
        P.check(a, b, tol, '%s inv_depth %d' % (what, i))
    P.check(rec['eval'], ref['eval'], tol, what + ' eval output')
    for k, v in ref['stats'].items():
        P.check(rec['stats'][k], v, max(STAT_TOL, tol * 0.1), '%s %s' % (what, k))
    assert rec['num_batches_tracked'] == ref['num_batches_tracked'] == 1


def depth_vs_fixture_case(device):
    net = make_depth_net(device)
    rec = depth_record(lambda rgb: (net(rgb)['inv_depths']), net, device)
    ref = fixture()['depth']
    check_depth(rec, ref, 'depth vs reference')
    check_grads(net.named_parameters(), ref['grad_norms'], ref['grad_samples'], 'depth vs reference')


def pose_vs_fixture_case(device):
    net = make_pose_net(device)
    rec = pose_record(lambda t, c: net(t, c), net, device)
    ref = fixture()['pose']
    assert tuple(rec['pose'].shape) == (SIZE[0], 2, 6)
    P.check(rec['pose'], ref['pose'], OUT_TOL, 'pose vs reference')
    check_grads(net.named_parameters(), ref['grad_norms'], ref['grad_samples'], 'pose vs reference')


def twin_vs_fixture_case(rel=1e-6):
    """The twin on the CPU reproduces the reference's outputs and gradients: ties the twin to the reference."""
    fx = fixture()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # as the fixture tool ran the reference: ATen's convolutions sum in a thread-dependent order
    try:
        net = make_depth_net(torch.device('cpu'))
        rec = depth_record(lambda rgb: torch_forward(net, rgb), net, torch.device('cpu'))
        pn = make_pose_net(torch.device('cpu'))
        prec = pose_record(lambda t, c: torch_forward(pn, t, c), pn, torch.device('cpu'))
    finally:
        torch.set_num_threads(threads)
    check_depth(rec, fx['depth'], 'twin depth', tol=rel)
    check_grads(net.named_parameters(), fx['depth']['grad_norms'], None, 'twin depth', norm_tol=1e-5)
    P.check(prec['pose'], fx['pose']['pose'], rel, 'twin pose')
    check_grads(pn.named_parameters(), fx['pose']['grad_norms'], None, 'twin pose', norm_tol=1e-5)


def depth_vs_twin_case(device):
    net = make_depth_net(device)
    twin = copy.deepcopy(net)
    rec = depth_record(lambda rgb: net(rgb)['inv_depths'], net, device)
    ref = depth_record(lambda rgb: torch_forward(twin, rgb), twin, device)
    check_depth(rec, ref, 'depth vs twin')
    check_grads(net.named_parameters(), ref['grad_norms'], ref['grad_samples'], 'depth vs twin')


def pose_vs_twin_case(device):
    net = make_pose_net(device)
    twin = copy.deepcopy(net)
    rec = pose_record(lambda t, c: net(t, c), net, device)
    ref = pose_record(lambda t, c: torch_forward(twin, t, c), twin, device)
    P.check(rec['pose'], ref['pose'], OUT_TOL, 'pose vs twin')
    check_grads(net.named_parameters(), ref['grad_norms'], ref['grad_samples'], 'pose vs twin')


def eval_is_stable_case(device):
    """A second eval call changes nothing: the running statistics are not touched in eval mode."""
    net = make_depth_net(device).eval()
    rgb = frames()[0].to(device)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        a = net(rgb)['inv_depths']
        b = net(rgb)['inv_depths']
    assert torch.is_tensor(a) and tuple(a.shape) == (SIZE[0], 1, SIZE[2], SIZE[3]) and torch.equal(a, b)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k


def stage_case(device, size=(2, 3, 16, 32)):
    """The encoder's first stage (input normalisation, conv1, bn1, max pool, layer1.0) and one decoder level (the up-sampled feature and
    the skip through upconv(2,1), then dispconv(2)) of DepthResNet18, forward and backward, against the twin's ATen ops in fp64 on the
    module's own parameters.  (The whole network takes more than twenty minutes on the host emulator; it runs on the GPU.)"""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    net = make_depth_net(device).train()
    ref = copy.deepcopy(net).double().cpu()
    rgb = frames(size)[0]

    e = net.encoder.encoder
    x = HF.conv2d_stride2(HF.affine(rgb.to(device), 1.0 / 0.225, -0.45 / 0.225), e.conv1.weight, None, e._packed)
    f0 = HF.batchnorm_act(x, e.bn1, ops.ACT_RELU)
    f1 = e.layer1[0](HF.maxpool3x3s2(f0))
    up, disp = net.decoder.convs[('upconv', 2, 1)], net.decoder.convs[('dispconv', 2)]
    out = disp(up((f1, f0), up=(2, 1)), act=ops.ACT_DISP, disp=DISP_RANGE)

    r = ref.encoder.encoder
    f0r = F.relu(_t_bn(F.conv2d((rgb.double() - 0.45) / 0.225, r.conv1.weight, None, 2, 3), r.bn1))
    f1r = _t_block(F.max_pool2d(f0r, 3, 2, 1), r.layer1[0])
    upr, dispr = list(ref.decoder.decoder)[5], list(ref.decoder.decoder)[12]
    xr = F.elu(_t_conv3x3(upr.conv, torch.cat([F.interpolate(f1r, scale_factor=2, mode='nearest'), f0r], 1)))
    outr = DISP_RANGE[0] + DISP_RANGE[1] * torch.sigmoid(_t_conv3x3(dispr, xr))

    P.check(out.detach().cpu().double(), outr.detach(), 1e-4, 'stage output')
    w = out_weights([tuple(out.shape)])[0]
    (out * w.to(device)).sum().backward()
    (outr * w.double()).sum().backward()
    named = [(n, p) for n, p in net.named_parameters() if p.grad is not None]
    refg = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    assert sorted(n for n, _ in named) == sorted(refg) and len(named) == 13
    for n, p in named:
        P.check(p.grad.cpu().double(), refg[n], 5e-4, 'stage gradient ' + n)
    for k in ('running_mean', 'running_var'):
        P.check(getattr(e.bn1, k).cpu().double(), getattr(r.bn1, k), 1e-5, 'stage bn1.' + k)
    assert int(e.bn1.num_batches_tracked) == 1 and int(e.layer1[0].bn2.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------ the SelfSupModel step
def step_batch(device, dtype=torch.float32, size=SIZE):
    rgb, ctx = frames(size)
    K = P.golden('step')['step_flip0']['batch']['intrinsics'][:1].repeat(size[0], 1, 1)          # a 64 x 96 camera
    K[:, 0] *= size[3] / 96.0
    K[:, 1] *= size[2] / 64.0
    rgb, ctx = rgb.to(device=device, dtype=dtype), [c.to(device=device, dtype=dtype) for c in ctx]
    return {'rgb': rgb, 'rgb_context': ctx, 'rgb_original': rgb, 'rgb_context_original': list(ctx),
            'intrinsics': K.to(device=device, dtype=dtype)}


def step_model(SelfSupModel, depth_net, pose_net, device):
    kw = dict(P.golden('step')['step_flip0']['loss_kwargs'])
    model = SelfSupModel(**kw, clip_loss=0.0, flip_lr_prob=0.0, upsample_depth_maps=True, rotation_mode='euler')
    model.add_depth_net(depth_net)
    model.add_pose_net(pose_net)
    return model.to(device).train()


def step_named(depth_net, pose_net):
    return [('depth_net.' + n, p) for n, p in depth_net.named_parameters()] + [('pose_net.' + n, p) for n, p in pose_net.named_parameters()]


def run_step(model, device, size=SIZE):
    random.seed(0)
    out = model(step_batch(device, size=size), progress=0.0)
    out['loss'].backward()
    return out


def our_step(device):
    from packnet_sfm.models.SelfSupModel import SelfSupModel
    dn, pn = make_depth_net(device), make_pose_net(device)
    return step_model(SelfSupModel, dn, pn, device), dn, pn


def check_step(out, named, ref, what):
    P.check(out['loss'].detach().float().cpu(), ref['loss'], 1e-4, what + ' loss')
    P.check(out['metrics']['smoothness_loss'].detach().float().cpu(), ref['smoothness_loss'], 1e-3, what + ' smoothness')
    d = 1.0 / out['inv_depths'][0].detach().float().cpu().clamp(min=1e-6)
    P.check(d, 1.0 / ref['inv_depth0'].clamp(min=1e-6), 1e-3, what + ' depth')
    check_grads(named, ref['grad_norms'], None, what, norm_tol=1e-2, rel_floor=1e-4)


def step_record(out, named):
    norms, samples = grad_record(named)
    return dict(loss=out['loss'].detach().float().cpu(), smoothness_loss=out['metrics']['smoothness_loss'].detach().float().cpu(),
                photometric_loss=out['metrics']['photometric_loss'].detach().float().cpu(),
                inv_depth0=out['inv_depths'][0].detach().float().cpu(), grad_norms=norms, grad_samples=samples)
