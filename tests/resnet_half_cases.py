"""fp16 evaluation / inference forward of DepthResNet (include/pnsfm.h "fp16 forward: ResNet networks"): cases shared by the emulated CPU
tests (tests/test_resnet_half_emulated.py) and the GPU tests (tests/test_gpu_resnet_half.py).

Oracle and tolerances (the project's own for fp16 kernels, tests/half_cases.py)
  convolution  float64 on the SAME fp16 values, scale and shift from a float64 fold.  An output may differ by one fp16 ulp of the oracle
               plus 2^-18 (|scale| sum |x w| + |shift| + |res|) (the fp32 accumulation and epilogue); with ACT_ELU / ACT_DISP
               invdepth_case's 2^-16 (|z| + 1) on top (expm1f / expf).  The staged value of a pre-affine is x a + b, a and b the fp32
               numbers, rounded ONCE to fp16 (the device does it in one v_fma_mixlo_f16): x a + b is exact in float64 (11 + 24
               significant bits, then a sum of close exponents), and round_once16 takes it to fp16 without the detour through fp32.
  bn_fold      scale within 2 fp32 ulps of the float64 value, shift within 2^-22 (|beta| + |mean scale|).
  max pool     bit-equal to F.max_pool2d on the same fp16 values.
Every convolution case runs twice (torch.equal) and writes into an output embedded in a NaN-filled buffer whose guards must survive.
Networks: rel(a) = ||a - anchor|| / ||anchor||, anchor = the twin (resnet_cases.torch_forward) of a .double() copy on the CPU, eager = the
twin of the fp16 copy; rule rel(ours) <= 1.5 rel(eager) + 2e-4 (tests/test_gpu_half.py's rule for PackNet).
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import half_cases as HC
import resnet_cases as RC
from packnet_sfm.hip import _lib, ops

GUARD = 64          # NaN elements on either side of an embedded output


def embedded(shape, dev, dtype=torch.float16):
    """A contiguous tensor of `shape` inside a NaN-filled buffer, and a check that the guards are still NaN."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device=dev)
    out = buf[GUARD:GUARD + n].view(shape)

    def intact():
        return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())
    return out, intact


def round_once16(d):
    """float64 -> fp16 with ONE rounding (torch's double -> half goes through float): the result of the two-step conversion, or the
    neighbour of it that is nearer to d."""
    best = d.float().half()
    bits = best.view(torch.int16)
    err = (best.double() - d).abs()
    for delta in (-1, 1):
        cand = (bits + delta).view(torch.float16)
        ce = (cand.double() - d).abs()
        take = torch.isfinite(cand) & (ce < err)
        best, err = torch.where(take, cand, best), torch.where(take, ce, err)
    return best


def _gather64(xs, ups, reflect, R, pre):
    """float64 G(x): up-sample, concatenate, pre-affine (rounded as the kernel rounds it), pad."""
    parts = []
    for t, u in zip(xs, ups):
        t = t.double().cpu()
        parts.append(F.interpolate(t, scale_factor=u, mode='nearest') if u == 2 else t)
    x = torch.cat(parts, 1)
    if pre is not None:
        a, b = (float(torch.tensor(v, dtype=torch.float32)) for v in pre)
        x = round_once16(x * a + b).double()
    if R:
        x = F.pad(x, (R, R, R, R), mode='reflect') if reflect else F.pad(x, (R, R, R, R))
    return x


def _act64(z, act, disp):
    if act == ops.ACT_ELU:
        return F.elu(z)
    if act == ops.ACT_RELU:
        return F.relu(z)
    if act == ops.ACT_DISP:
        return disp[0] + disp[1] * torch.sigmoid(z)
    return z


def fused_case(dev, B, chans, Cout, H, W, ks, stride=1, reflect=False, ups=None, scale=False, shift=False, res=False, act=ops.ACT_NONE,
               pre=None, ksplit=1, seed=0, disp=RC.DISP_RANGE):
    """One launch of the gathering convolution on sources of chans[i] channels, source i holding (H / ups[i]) x (W / ups[i]) pixels;
    returns the kernel's last_config.  ksplit: 1 = never split, n > 1 = at most n splits (the case must then split), None = default."""
    g = torch.Generator().manual_seed(seed)
    ups = tuple(ups) if ups is not None else (1,) * len(chans)
    xs = [HC._rand16((B, c, H // u, W // u), g, 1.0, dev) for c, u in zip(chans, ups)]
    Cin = sum(chans)
    w = (torch.randn((Cout, Cin, ks, ks), generator=g, dtype=torch.float64) * (2.0 / (Cin * ks * ks)) ** 0.5).half().to(dev)
    sc = (1.0 + 0.3 * torch.randn(Cout, generator=g)).float().to(dev) if scale else None
    sh = (0.2 * torch.randn(Cout, generator=g)).float().to(dev) if shift else None
    shape = ops.conv2d_h16g_out_shape(xs, ups, Cout, ks, stride)
    r = HC._rand16(shape, g, 1.0, dev) if res else None
    lib = _lib.get()
    prev = lib.pnsfm_set_h16_max_split(ksplit if ksplit is not None else 0)
    try:
        wp = ops.conv2d_pack_h16(w)
        outs = []
        for _ in range(2):
            y, intact = embedded(shape, dev)
            ops.conv2d_forward_h16g(xs, wp, Cout, ks, stride=stride, reflect=reflect, ups=ups, scale=sc, shift=sh, res=r, act=act,
                                    disp=disp, pre_affine=pre, out=y)
            assert intact(), 'the kernel wrote outside its output'
            outs.append(y)
        cfg = ops.conv2d_last_config()
        if stride == 2:                              # the interleaved LDS form of a stride-2 patch: the same sums, the same bits
            was = lib.pnsfm_set_h16g_deinterleave(0)
            try:
                y, intact = embedded(shape, dev)
                ops.conv2d_forward_h16g(xs, wp, Cout, ks, stride=stride, reflect=reflect, ups=ups, scale=sc, shift=sh, res=r, act=act,
                                        disp=disp, pre_affine=pre, out=y)
                assert was == 1 and intact()
                outs.append(y)
            finally:
                lib.pnsfm_set_h16g_deinterleave(was)
    finally:
        lib.pnsfm_set_h16_max_split(prev)
    what = 'conv2d_h16g B=%d chans=%s ups=%s Cout=%d %dx%d k=%d s=%d reflect=%d act=%d ksplit=%s' % (
        B, chans, ups, Cout, H, W, ks, stride, reflect, act, ksplit)
    assert all(torch.equal(outs[0], o) for o in outs[1:]), what + ': not deterministic, or the two LDS forms differ'
    assert not torch.isnan(outs[0]).any(), what + ': an output element was not written'
    R = ks // 2
    x64 = _gather64(xs, ups, reflect, R, pre)
    w64 = w.double().cpu()
    z = F.conv2d(x64, w64, None, stride)
    mag = F.conv2d(x64.abs(), w64.abs(), None, stride)
    sc64 = sc.double().cpu().view(1, -1, 1, 1) if scale else 1.0
    sh64 = sh.double().cpu().view(1, -1, 1, 1) if shift else 0.0
    r64 = r.double().cpu() if res else 0.0
    z = z * sc64 + sh64 + r64
    extra = 2.0 ** -18 * (mag * (sc64.abs() if scale else 1.0) + (sh64.abs() if shift else 0.0) + (r64.abs() if res else 0.0))
    if act in (ops.ACT_ELU, ops.ACT_DISP):
        extra = extra + 2.0 ** -16 * (_act64(z, act, disp).abs() + 1)
    assert tuple(z.shape) == tuple(shape), what
    HC.assert_close16(outs[0], _act64(z, act, disp), extra=extra, what=what)
    assert cfg[0] == 10, cfg
    if ksplit == 1:
        assert cfg[4] == 1, cfg
    elif ksplit is not None and Cin > 16:            # (a single 16-channel chunk -- the stem -- has nothing to split)
        assert cfg[4] > 1, cfg
    return cfg


# (name, kwargs): the smallest shapes at which each mechanism can go wrong; every one runs with the split limit at 1 and at 2 (which every
# case with more than one 16-channel chunk must then use)
OP_CASES = [
    ('stem 10x14', dict(B=2, chans=[3], Cout=64, H=10, W=14, ks=7, stride=2, scale=True, shift=True, act=ops.ACT_RELU,
                        pre=(1.0 / 0.225, -0.45 / 0.225), seed=1)),
    ('stem 9x13', dict(B=1, chans=[3], Cout=64, H=9, W=13, ks=7, stride=2, scale=True, shift=True, act=ops.ACT_RELU,
                       pre=(1.0 / 0.225, -0.45 / 0.225), seed=2)),
    ('3x3 s2 6x10', dict(B=1, chans=[20], Cout=40, H=6, W=10, ks=3, stride=2, seed=3)),
    ('3x3 s2 5x11', dict(B=2, chans=[20], Cout=40, H=5, W=11, ks=3, stride=2, seed=4)),
    ('1x1 s2 6x10', dict(B=1, chans=[20], Cout=40, H=6, W=10, ks=1, stride=2, seed=5)),
    ('1x1 s2 5x11', dict(B=2, chans=[20], Cout=40, H=5, W=11, ks=1, stride=2, seed=6)),
    ('3x3 s2 1x1 pixel', dict(B=1, chans=[20], Cout=40, H=1, W=1, ks=3, stride=2, seed=7)),
    ('1x1 s2 1x1 pixel', dict(B=1, chans=[20], Cout=40, H=1, W=1, ks=1, stride=2, seed=8)),
    ('reflect 2x2', dict(B=1, chans=[20], Cout=40, H=2, W=2, ks=3, reflect=True, shift=True, seed=9)),
    ('reflect 5x11', dict(B=2, chans=[20], Cout=40, H=5, W=11, ks=3, reflect=True, shift=True, seed=10)),
    ('reflect up2 + skip, ELU', dict(B=1, chans=[16, 13], ups=(2, 1), Cout=32, H=6, W=10, ks=3, reflect=True, shift=True, act=ops.ACT_ELU,
                                     seed=11)),
    ('reflect up2 + skip, DISP', dict(B=1, chans=[16, 13], ups=(2, 1), Cout=32, H=6, W=10, ks=3, reflect=True, shift=True,
                                      act=ops.ACT_DISP, seed=12)),
    ('scale shift res ReLU', dict(B=1, chans=[20], Cout=40, H=5, W=11, ks=3, scale=True, shift=True, res=True, act=ops.ACT_RELU, seed=13)),
]
SPLITS = [1, 2]


def op_case(dev, name, ksplit):
    return fused_case(dev, ksplit=ksplit, **dict(OP_CASES)[name])


def wide_m_case(dev):
    """Cout = 260: the surplus m-tiles of the 256-row workgroup, with a residual, K split limit 4 (as half_cases' wide-M case)."""
    cfg = fused_case(dev, 1, [129], 260, 3, 5, 3, scale=True, shift=True, res=True, act=ops.ACT_RELU, ksplit=4, seed=14)
    assert cfg[4] == 3, cfg          # nine chunks under a limit of 4: three per split


def reflect_too_small_case(dev):
    x = HC._rand16((1, 20, 1, 6), torch.Generator().manual_seed(15), 1.0, dev)
    w = HC._rand16((40, 20, 3, 3), torch.Generator().manual_seed(16), 0.1, dev)
    wp = ops.conv2d_pack_h16(w)
    with pytest.raises(ValueError):
        ops.conv2d_forward_h16g([x], wp, 40, 3, reflect=True)
    from packnet_sfm.hip import functional as HF
    with pytest.raises(ValueError):
        HF.conv3x3_reflect(x, w, None, HF.PackedConvWeight())
    assert tuple(ops.conv2d_forward_h16g([x], wp, 40, 3).shape) == (1, 40, 1, 6)          # zero padding takes it


def ties_to_h16_case(dev, ksplit):
    """Null scale, bias only, stride 1, zero padding: the new kernel gives conv2d_forward_h16's bits (same geometry, same split)."""
    g = torch.Generator().manual_seed(17)
    for chans, Cout, H, W, ks in (([20], 40, 5, 11, 3), ([16, 13], 32, 4, 7, 5), ([129], 260, 3, 5, 1)):
        xs = [HC._rand16((2, c, H, W), g, 1.0, dev) for c in chans]
        w = HC._rand16((Cout, sum(chans), ks, ks), g, 0.1, dev)
        b = (0.1 * torch.randn(Cout, generator=g)).float().to(dev)
        lib = _lib.get()
        prev = lib.pnsfm_set_h16_max_split(ksplit)
        try:
            wp = ops.conv2d_pack_h16(w)
            for bias in (b, None):
                old = ops.conv2d_forward_h16(xs, wp, bias, Cout, ks)
                c_old = ops.conv2d_last_config()
                new = ops.conv2d_forward_h16g(xs, wp, Cout, ks, shift=bias)
                c_new = ops.conv2d_last_config()
                assert (c_old[0], c_new[0]) == (9, 10) and c_old[1:] == c_new[1:], (c_old, c_new)
                assert (c_new[4] == 1) if ksplit == 1 else (c_new[4] > 1), c_new
                assert torch.equal(old, new), 'conv2d_h16g differs from conv2d_h16 at %s' % ((chans, Cout, H, W, ks),)
        finally:
            lib.pnsfm_set_h16_max_split(prev)


def errors_case(dev):
    """Shape, null-pointer and unsupported-mode errors come back as error codes with a message."""
    x = HC._rand16((1, 20, 5, 11), torch.Generator().manual_seed(18), 1.0, dev)
    w = HC._rand16((40, 20, 3, 3), torch.Generator().manual_seed(19), 0.1, dev)
    wp = ops.conv2d_pack_h16(w)
    with pytest.raises(_lib.HipError, match='stride'):
        ops.conv2d_forward_h16g([x], wp, 40, 3, stride=3)
    with pytest.raises(_lib.HipError, match='kernel size'):
        ops.conv2d_forward_h16g([x], wp, 40, 2)
    with pytest.raises(_lib.HipError, match='activation'):
        ops.conv2d_forward_h16g([x], wp, 40, 3, act=7)
    with pytest.raises(RuntimeError, match='spatial sizes'):
        ops.conv2d_forward_h16g([x[..., :3, :5].contiguous(), x], wp, 40, 3, ups=(2, 1))      # 6 x 10 against 5 x 11
    with pytest.raises(RuntimeError):
        ops.conv2d_forward_h16g([x.float()], wp, 40, 3)


def maxpool_case(dev, shape, kind):
    N, h, w = shape
    if kind == 'zeros':
        x = torch.zeros(1, N, h, w)
    elif kind == 'repeat':
        x = ((torch.arange(N * h * w) % 3) == 1).float().view(1, N, h, w)
    else:
        x = RC._ints((1, N, h, w), 7) + 0.25 * RC._ints((1, N, h, w), 8)
    x = x.half()
    ref = F.max_pool2d(x.float(), 3, 2, 1).half()              # max moves values: exact on the same fp16 values
    y, intact = embedded(tuple(ref.shape), dev)
    ops.maxpool3x3s2_forward_h16(x.to(dev), out=y)
    assert intact()
    assert torch.equal(y.cpu(), ref), 'max pool h16 %s %s' % (shape, kind)
    from packnet_sfm.hip import functional as HF
    assert torch.equal(HF.maxpool3x3s2(x.to(dev)).cpu(), ref)


def maxpool_nan_case(dev):
    x = torch.tensor([[1.0, float('nan'), 3.0], [0.0, 2.0, 9.0], [5.0, 5.0, 5.0]]).half().view(1, 1, 3, 3)
    y = ops.maxpool3x3s2_forward_h16(x.to(dev)).cpu()
    ref = F.max_pool2d(x.float(), 3, 2, 1).half()
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.nan_to_num(y), torch.nan_to_num(ref))


def bn_fold_case(dev, C):
    g = torch.Generator().manual_seed(20 + C)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).half()
    beta = (0.3 * torch.randn(C, generator=g)).half()
    mean = (0.5 * torch.randn(C, generator=g)).half()
    var = (0.5 + torch.rand(C, generator=g)).half()
    var[0] = 2.0 ** -14                                        # the smallest variance the case table asks for
    if C > 2:
        var[C // 2] = 2.0 ** -10
    eps = 1e-5
    out, intact = embedded((2, C), dev, torch.float32)
    ops.bn_fold_h16(gamma.to(dev), beta.to(dev), mean.to(dev), var.to(dev), eps, out=out)
    assert intact()
    s64 = gamma.double() / torch.sqrt(var.double() + eps)
    h64 = beta.double() - mean.double() * s64
    got = out.double().cpu()
    ulp32 = torch.tensor([RC.ulp(float(v)) for v in s64], dtype=torch.float64)
    assert bool(((got[0] - s64).abs() <= 2 * ulp32).all()), 'bn_fold scale C=%d: worst %g ulp' % (C, float(((got[0] - s64).abs() / ulp32).max()))
    bound = 2.0 ** -22 * (beta.double().abs() + (mean.double() * s64).abs())
    assert bool(((got[1] - h64).abs() <= bound).all()), 'bn_fold shift C=%d' % C
    return got


# ------------------------------------------------------------------------------------------------ stage and networks
def rel(a, anchor):
    a, anchor = a.double().cpu(), anchor.double().cpu()
    return float((a - anchor).norm() / anchor.norm())


def check_rule(ours, eager, anchor, what):
    assert bool(torch.isfinite(ours.float()).all()), what + ': non-finite output'
    r_ours, r_eager = rel(ours, anchor), rel(eager, anchor)
    print('%-40s rel(ours) %.3e  rel(eager fp16) %.3e  ratio %.2f' % (what, r_ours, r_eager, r_ours / r_eager if r_eager else math.inf))
    assert r_ours <= 1.5 * r_eager + 2e-4, '%s: rel(ours) %.3e > 1.5 x rel(eager) %.3e + 2e-4' % (what, r_ours, r_eager)
    return r_ours, r_eager


def _stage_twin(net, rgb):
    """resnet_cases.stage_case's stage in eval mode through the twin's ATen ops, on `net`'s own parameters, in their dtype."""
    r = net.encoder.encoder
    f0 = F.relu(RC._t_bn(F.conv2d((rgb - 0.45) / 0.225, r.conv1.weight, None, 2, 3), r.bn1))
    f1 = RC._t_block(F.max_pool2d(f0, 3, 2, 1), r.layer1[0])
    up, disp = list(net.decoder.decoder)[5], list(net.decoder.decoder)[12]
    x = F.elu(RC._t_conv3x3(up.conv, torch.cat([F.interpolate(f1, scale_factor=2, mode='nearest'), f0], 1)))
    return RC.DISP_RANGE[0] + RC.DISP_RANGE[1] * torch.sigmoid(RC._t_conv3x3(disp, x))


def stage_case(dev, size=(2, 3, 16, 32)):
    """The fp16 eval twin of resnet_cases.stage_case: stem, max pool, layer1.0, then upconv(2, 1) on (up-sampled feature, skip) and
    dispconv(2), six launches; against the float64 twin, beside the fp16 twin on the CPU."""
    from packnet_sfm.hip import functional as HF
    net = RC.make_depth_net('cpu', dtype=torch.float16).eval()
    ref64 = copy.deepcopy(net).double()
    rgb = RC.frames(size)[0].half()
    with torch.no_grad():
        anchor = _stage_twin(ref64, rgb.double())
        eager = _stage_twin(net, rgb)
        net = net.to(dev)
        e = net.encoder.encoder
        f0 = HF.conv2d_h16_fused(rgb.to(dev), e.conv1.weight, e._packed, stride=2, bn=e.bn1, act=ops.ACT_RELU,
                                 pre_affine=(1.0 / 0.225, -0.45 / 0.225))
        f1 = e.layer1[0](HF.maxpool3x3s2(f0))
        up, disp = net.decoder.convs[('upconv', 2, 1)], net.decoder.convs[('dispconv', 2)]
        out = disp(up((f1, f0), up=(2, 1)), act=ops.ACT_DISP, disp=RC.DISP_RANGE)
    assert out.dtype == torch.float16 and tuple(out.shape) == tuple(anchor.shape)
    return check_rule(out, eager, anchor, 'stage %s' % (size,))
