"""CPU: the fp16 forward kernels of the ResNet networks (include/pnsfm.h "fp16 forward: ResNet networks") on the host-emulated build,
against float64 on the same fp16 values (tests/resnet_half_cases.py)."""
import pytest
import torch

import resnet_cases as RC
import resnet_half_cases as C


@pytest.mark.parametrize('ksplit', C.SPLITS)
@pytest.mark.parametrize('name', [n for n, _ in C.OP_CASES])
def test_conv_h16g(emulated_kernels, name, ksplit):
    C.op_case('cpu', name, ksplit)


def test_conv_h16g_wide_m_res_split4(emulated_kernels):
    C.wide_m_case('cpu')


@pytest.mark.parametrize('ksplit', [1, 4])
def test_conv_h16g_ties_to_conv_h16(emulated_kernels, ksplit):
    C.ties_to_h16_case('cpu', ksplit)


def test_conv_h16g_reflect_too_small(emulated_kernels):
    C.reflect_too_small_case('cpu')


def test_conv_h16g_errors(emulated_kernels):
    C.errors_case('cpu')


@pytest.mark.parametrize('kind', RC.POOL_KINDS)
@pytest.mark.parametrize('shape', RC.POOL_SHAPES)
def test_maxpool_h16(emulated_kernels, shape, kind):
    C.maxpool_case('cpu', shape, kind)


def test_maxpool_h16_nan(emulated_kernels):
    C.maxpool_nan_case('cpu')


@pytest.mark.parametrize('channels', [1, 64, 513])
def test_bn_fold_h16(emulated_kernels, channels):
    C.bn_fold_case('cpu', channels)


def test_stage_h16(emulated_kernels):
    C.stage_case('cpu')


def test_fused_conv_rules(emulated_kernels):
    """conv2d_h16_fused: mixed dtypes raise RuntimeError both ways, a training-mode BatchNorm NotImplementedError, a backward raises,
    the plain memory-bound ops keep refusing fp16."""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.hip import ops
    g = torch.Generator().manual_seed(30)
    x = torch.randn((1, 16, 4, 6), generator=g).half()
    w = (0.1 * torch.randn((32, 16, 3, 3), generator=g)).half()
    bn = torch.nn.BatchNorm2d(32).half().eval()
    cache = HF.PackedConvWeight()
    y = HF.conv2d_h16_fused(x, w, cache, bn=bn, act=ops.ACT_RELU)
    assert y.dtype == torch.float16 and tuple(y.shape) == (1, 32, 4, 6)
    fold = cache.fold_h16
    assert torch.equal(HF.conv2d_h16_fused(x, w, cache, bn=bn, act=ops.ACT_RELU), y) and cache.fold_h16 is fold      # cached
    with torch.no_grad():
        bn.running_mean += 1.0                                   # an in-place change bumps the version: re-folded
    assert not torch.equal(HF.conv2d_h16_fused(x, w, cache, bn=bn, act=ops.ACT_RELU), y) and cache.fold_h16 is not fold
    with pytest.raises(RuntimeError):
        HF.conv2d_h16_fused(x.float(), w, cache, bn=bn)
    with pytest.raises(RuntimeError):
        HF.conv2d_h16_fused(x, w.float(), cache, bn=bn)
    with pytest.raises(RuntimeError):
        HF.conv2d_h16_fused(x, w, cache, bn=torch.nn.BatchNorm2d(32).eval())
    with pytest.raises(NotImplementedError, match='eval'):
        HF.conv2d_h16_fused(x, w, cache, bn=torch.nn.BatchNorm2d(32).half().train())
    with pytest.raises(NotImplementedError):
        HF.conv2d_h16_fused(x, w, cache, bn=torch.nn.BatchNorm2d(32, track_running_stats=False).half().eval())
    wl = w.clone().requires_grad_(True)
    out = HF.conv2d_h16_fused(x, wl, HF.PackedConvWeight(), bn=bn)
    with pytest.raises(NotImplementedError, match='forward pass only'):
        out.float().sum().backward()
    for call in (lambda: HF.batchnorm_act(x, bn), lambda: HF.reflect_pad1(x), lambda: HF.act_crop(x), lambda: HF.affine(x, 2.0, 1.0)):
        with pytest.raises(NotImplementedError, match='fp16'):
            call()


def test_module_rules():
    """Decided in the modules, before any kernel or library call (no emulated library here): fp16 in training mode and an fp16
    PoseResNet raise NotImplementedError, mixed dtypes RuntimeError."""
    from packnet_sfm.networks.depth.DepthResNet import DepthResNet
    from packnet_sfm.networks.pose.PoseResNet import PoseResNet
    rgb = RC.frames()[0]
    net = DepthResNet(version='18').half()
    with pytest.raises(NotImplementedError, match=r'fp16.*\.eval\(\)'):
        net(rgb.half())
    with pytest.raises(RuntimeError, match='float16 network'):
        net.eval()(rgb)
    with pytest.raises(RuntimeError, match='half'):
        DepthResNet(version='18').eval()(rgb.half())
    for pose in (PoseResNet(version='18').half().eval(), PoseResNet(version='18').half()):
        with pytest.raises(NotImplementedError, match='fp16'):
            pose(rgb.half(), [rgb.half()])
