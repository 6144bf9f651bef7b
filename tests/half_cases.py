"""fp16 forward (evaluation / inference) cases shared by the emulated CPU tests (tests/test_half_emulated.py) and the GPU tests
(tests/test_gpu_half.py): every fp16 entry point of include/pnsfm.h against a float64 host computation on the SAME fp16 values.

Tolerance of a kernel that rounds its fp32 result once to fp16: one fp16 ulp of the float64 value, plus (convolutions) 2^-18 of
sum |x * w| for the fp32 accumulation."""
import torch
import torch.nn.functional as F

from packnet_sfm.hip import _lib, ops


def ulp16(v):
    """fp16 spacing at |v| (subnormal spacing 2^-24 below 2^-14)."""
    a = v.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def assert_close16(y, y64, extra=0.0, what=''):
    assert y.dtype == torch.float16, what
    y = y.double().cpu()
    y64 = y64.double().cpu()
    tol = ulp16(y64) + extra
    err = (y - y64).abs()
    bad = err > tol
    assert not bad.any(), '%s: %d of %d elements off, worst excess %g' % (what, int(bad.sum()), y.numel(), float((err - tol).max()))


def _rand16(shape, gen, scale=1.0, dev='cpu'):
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale).half().to(dev)


def conv_case(dev, B, chans, Cout, H, W, ks, seed=0, w_f32=False, ksplit=None):
    """fp16 conv of the concatenation of len(chans) sources; returns the kernel's last_config."""
    g = torch.Generator().manual_seed(seed)
    xs = [_rand16((B, c, H, W), g, 1.0, dev) for c in chans]
    Cin = sum(chans)
    wsc = (2.0 / (Cin * ks * ks)) ** 0.5
    w = torch.randn((Cout, Cin, ks, ks), generator=g, dtype=torch.float64) * wsc
    w = (w.float() if w_f32 else w.half()).to(dev)
    b = (torch.randn(Cout, generator=g) * 0.1).float().to(dev)
    lib = _lib.get()
    prev = lib.pnsfm_set_h16_max_split(ksplit if ksplit is not None else 0)
    try:
        wp = ops.conv2d_pack_h16(w)
        y = ops.conv2d_forward_h16(xs, wp, b, Cout, ks)
        cfg = ops.conv2d_last_config()
        y2 = ops.conv2d_forward_h16(xs, wp, b, Cout, ks)
    finally:
        lib.pnsfm_set_h16_max_split(prev)
    assert torch.equal(y, y2), 'fp16 conv is not deterministic'
    x64 = torch.cat([t.double().cpu() for t in xs], 1)
    w64 = w.double().cpu()
    if w_f32:
        w64 = w.half().double().cpu()         # the packer rounds an fp32 source to fp16
    y64 = F.conv2d(x64, w64, b.double().cpu(), padding=ks // 2)
    mag = F.conv2d(x64.abs(), w64.abs(), None, padding=ks // 2)
    assert_close16(y, y64, extra=2.0 ** -18 * mag, what='conv2d_h16 B=%d chans=%s Cout=%d %dx%d k=%d' % (B, chans, Cout, H, W, ks))
    assert cfg[0] == 9, cfg
    return cfg


def groupnorm_case(dev, B, C, H, W, G=16, res=True, act=ops.ACT_ELU, seed=1, fused=1):
    """fused: 1 = the one-launch form where the slab fits, 0 = the two-launch form (restored afterwards)."""
    lib = _lib.get()
    prev = lib.pnsfm_set_gn_fused(fused)
    try:
        _groupnorm_case(dev, B, C, H, W, G, res, act, seed)
    finally:
        lib.pnsfm_set_gn_fused(prev)


def _groupnorm_case(dev, B, C, H, W, G, res, act, seed):
    g = torch.Generator().manual_seed(seed)
    x = _rand16((B, C, H, W), g, 2.0, dev)
    r = _rand16((B, C, H, W), g, 1.0, dev) if res else None
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).half().to(dev)
    beta = (0.2 * torch.randn(C, generator=g)).half().to(dev)
    y = ops.groupnorm_act_forward_h16(x, r, gamma, beta, G, 1e-5, act)
    v = x.double().cpu() + (r.double().cpu() if res else 0)
    z = F.group_norm(v, G, gamma.double().cpu(), beta.double().cpu(), 1e-5)
    if act == ops.ACT_ELU:
        z = F.elu(z)
    assert_close16(y, z, extra=2e-5 * (z.abs() + 1), what='groupnorm_h16 %s res=%s' % ((B, C, H, W), res))
    assert torch.equal(y, ops.groupnorm_act_forward_h16(x, r, gamma, beta, G, 1e-5, act))


def conv3d_case(dev, B, D, H, W, NF, seed=2):
    g = torch.Generator().manual_seed(seed)
    p = _rand16((B, D, H, W), g, 1.0, dev)
    w3 = (torch.randn((NF, 1, 3, 3, 3), generator=g) * 0.3).half().to(dev)
    b3 = (torch.randn(NF, generator=g) * 0.1).half().to(dev)
    y = ops.conv3d_forward_h16(p, w3, b3)
    z = F.conv3d(p.double().cpu().unsqueeze(1), w3.double().cpu(), b3.double().cpu(), padding=1).reshape(B, NF * D, H, W)
    mag = F.conv3d(p.double().cpu().abs().unsqueeze(1), w3.double().cpu().abs(), None, padding=1).reshape(B, NF * D, H, W)
    assert_close16(y, z, extra=2.0 ** -18 * mag, what='conv3d_h16 NF=%d' % NF)


def movement_case(dev, B, C, H, W, seed=3):
    """space_to_depth / depth_to_space / upsample_nearest / region ops move fp16 values: bit-exact."""
    g = torch.Generator().manual_seed(seed)
    x = _rand16((B, C, H, W), g, 1.0, dev)
    y = ops.space_to_depth_h16(x)
    assert torch.equal(y.cpu(), F.pixel_unshuffle(x.cpu(), 2))
    assert torch.equal(ops.depth_to_space_h16(y).cpu(), x.cpu())
    u = ops.upsample_nearest_forward_h16(x, 2)
    assert torch.equal(u.cpu(), F.interpolate(x.cpu().float(), scale_factor=2, mode='nearest').half())
    dst = torch.zeros((B, C, H, W), dtype=torch.float16, device=dev)
    ops.region_ops_h16([(ops.REGION_COPY, dst[:, :, :2], x[:, :, H - 2:]), (ops.REGION_ADD, dst[:, :, 2:, :3], x[:, :, 2:, :3]),
                        (ops.REGION_ZERO, dst[:, :, 2:, 3:], None)])
    ref = torch.zeros((B, C, H, W), dtype=torch.float16)
    xc = x.cpu()
    ref[:, :, :2] = xc[:, :, H - 2:]
    ref[:, :, 2:, :3] = xc[:, :, 2:, :3]
    assert torch.equal(dst.cpu(), ref)


def invdepth_case(dev, B, C, H, W, seed=4, min_depth=0.5):
    g = torch.Generator().manual_seed(seed)
    x = _rand16((B, C, H, W), g, 1.0, dev)
    w = (torch.randn((1, C, 3, 3), generator=g) * (1.0 / (9 * C)) ** 0.5).half().to(dev)
    b = torch.tensor([0.1]).half().to(dev)
    y = ops.invdepth_conv_forward_h16(x, w, b, min_depth)
    z = torch.sigmoid(F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)) / min_depth
    assert_close16(y, z, extra=2.0 ** -16 * (z.abs() + 1), what='invdepth_h16')
