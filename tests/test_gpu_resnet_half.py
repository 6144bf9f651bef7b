"""GPU: fp16 evaluation / inference forward of DepthResNet on the gfx950 kernels (include/pnsfm.h "fp16 forward: ResNet networks") --
per-op checks at the edge shapes and at the real layer shapes, the stage and the networks against the float64 twin, and the contract."""
import copy

import pytest
import torch

import resnet_cases as RC
import resnet_half_cases as C
from packnet_sfm.hip import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PRE = (1.0 / 0.225, -0.45 / 0.225)


@pytest.mark.parametrize('ksplit', C.SPLITS)
@pytest.mark.parametrize('name', [n for n, _ in C.OP_CASES])
def test_conv_h16g(name, ksplit):
    C.op_case(DEV, name, ksplit)


def test_conv_h16g_wide_m_res_split4():
    C.wide_m_case(DEV)


@pytest.mark.parametrize('ksplit', [1, 4])
def test_conv_h16g_ties_to_conv_h16(ksplit):
    C.ties_to_h16_case(DEV, ksplit)


def test_conv_h16g_reflect_too_small_and_errors():
    C.reflect_too_small_case(DEV)
    C.errors_case(DEV)


@pytest.mark.parametrize('kind', RC.POOL_KINDS)
@pytest.mark.parametrize('shape', RC.POOL_SHAPES)
def test_maxpool_h16(shape, kind):
    C.maxpool_case(DEV, shape, kind)


def test_maxpool_h16_nan():
    C.maxpool_nan_case(DEV)


@pytest.mark.parametrize('channels', [1, 64, 513])
def test_bn_fold_h16(channels):
    C.bn_fold_case(DEV, channels)


# ---- the layer classes of DepthResNet18 at 192 x 640, batch 1: one each (ksplit None: the launcher's own choice)
LAYER_CLASSES = [
    ('stem', dict(chans=[3], Cout=64, H=192, W=640, ks=7, stride=2, scale=True, shift=True, act=ops.ACT_RELU, pre=PRE), False),
    ('64->128 3x3 s2 @ 48x160', dict(chans=[64], Cout=128, H=48, W=160, ks=3, stride=2, scale=True, shift=True, act=ops.ACT_RELU), None),
    ('256->512 1x1 s2 onto 6x20', dict(chans=[256], Cout=512, H=12, W=40, ks=1, stride=2, scale=True, shift=True), None),
    ('512->512 3x3 @ 6x20 res', dict(chans=[512], Cout=512, H=6, W=20, ks=3, scale=True, shift=True, res=True, act=ops.ACT_RELU), True),
    ('reflect [16 up2]->16 @ 192x640', dict(chans=[16], ups=(2,), Cout=16, H=192, W=640, ks=3, reflect=True, shift=True, act=ops.ACT_ELU),
     False),
    ('reflect [32 up2 + 64]->32 @ 96x320', dict(chans=[32, 64], ups=(2, 1), Cout=32, H=96, W=320, ks=3, reflect=True, shift=True,
                                                act=ops.ACT_ELU), None),
]


@pytest.mark.parametrize('name', [n for n, _, _ in LAYER_CLASSES])
def test_conv_h16g_layer_classes(name):
    kw, split = next((k, s) for n, k, s in LAYER_CLASSES if n == name)
    cfg = C.fused_case(DEV, 1, ksplit=None, seed=40, **kw)
    if split is not None:
        assert (cfg[4] > 1) == split, cfg


def test_stage_h16():
    C.stage_case(DEV)


# ---- networks
_ANCHORS = {}


def _network(version, size):
    """(fp16 eval net on the device, fp16 rgb, anchor, eager fp16 output), computed once per (version, size)."""
    key = (version, size)
    if key not in _ANCHORS:
        net = RC.make_depth_net(DEV, version, dtype=torch.float16).eval()
        rgb = RC.frames(size)[0].half()
        with torch.no_grad():
            anchor = RC.torch_forward(copy.deepcopy(net).cpu().double(), rgb.double())
            eager = RC.torch_forward(net, rgb.to(DEV))
        _ANCHORS[key] = (net, rgb.to(DEV), anchor, eager)
    return _ANCHORS[key]


@pytest.mark.parametrize('version,size', [('18', RC.SIZE), ('34', RC.SIZE), ('18', (1, 3, 192, 640))])
def test_network_half_vs_fp64(version, size):
    net, rgb, anchor, eager = _network(version, size)
    with torch.no_grad():
        y = net(rgb)['inv_depths']
        y2 = net(rgb)['inv_depths']
    assert y.dtype == torch.float16 and tuple(y.shape) == (size[0], 1, size[2], size[3]) and torch.equal(y, y2)
    C.check_rule(y, eager, anchor, 'DepthResNet%s %s' % (version, 'x'.join(map(str, size))))


def test_half_contract():
    from packnet_sfm.networks.depth.DepthResNet import DepthResNet
    rgb = RC.frames()[0].to(DEV)
    net = RC.make_depth_net(DEV).eval()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        net(rgb)                                             # packs the fp32 weights
    net = net.half()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        y = net(rgb.half())['inv_depths']
        assert torch.equal(y, net(rgb.half())['inv_depths'])
    assert y.dtype == torch.float16 and tuple(y.shape) == (RC.SIZE[0], 1, RC.SIZE[2], RC.SIZE[3])
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    # fp32 -> half -> float equals a fresh fp32 net with the fp16-rounded state dict: the weight and fold caches follow the parameters
    net = net.float()
    fresh = DepthResNet(version='18')
    fresh.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(net(rgb)['inv_depths'], fresh(rgb)['inv_depths'])
        # ... and back to fp16: the same bits as before the round trip
        assert torch.equal(net.half()(rgb.half())['inv_depths'], y)
    # mixed dtypes raise, both ways
    with torch.no_grad(), pytest.raises(RuntimeError):
        net(rgb)
    with torch.no_grad(), pytest.raises(RuntimeError):
        fresh(rgb.half())
    # training mode, pose network, backward
    with pytest.raises(NotImplementedError, match='fp16'):
        net.train()(rgb.half())
    pose = RC.make_pose_net(DEV, dtype=torch.float16).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match='fp16'):
        pose(rgb.half(), [rgb.half(), rgb.half()])
    out = net.eval()(rgb.half())['inv_depths']
    assert out.requires_grad
    with pytest.raises(NotImplementedError):
        out.float().sum().backward()


def test_sfm_model_half_eval():
    """SfmModel with an fp16 DepthResNet on a batch without rgb_context; its output through post_process_inv_depth and evaluate_depth
    in fp16."""
    import types
    from packnet_sfm.models.SfmModel import SfmModel
    from packnet_sfm.utils.depth import evaluate_depth
    net, rgb, anchor, _ = _network('18', RC.SIZE)
    m = SfmModel()
    m.add_depth_net(copy.deepcopy(net))
    m = m.to(DEV).half().eval()

    def inv_of(batch):
        inv = m(batch)['inv_depths']
        return inv[0] if isinstance(inv, (list, tuple)) else inv
    with torch.no_grad():
        inv = inv_of({'rgb': rgb})
        flipped = inv_of({'rgb': torch.flip(rgb, [3])})
        gt = (1.0 / anchor.clamp(min=1e-6)).half().to(DEV)
        cfg = types.SimpleNamespace(min_depth=0.0, max_depth=80.0, crop='', scale_output='resize')
        res = evaluate_depth(cfg, gt, inv, flipped)
    assert inv.dtype == torch.float16 and tuple(inv.shape) == (RC.SIZE[0], 1, RC.SIZE[2], RC.SIZE[3])
    pp = res['inv_depth']
    assert pp.dtype == torch.float16 and tuple(pp.shape) == tuple(inv.shape) and bool(torch.isfinite(pp.float()).all())
    assert sorted(res['metrics']) == sorted(['', '_pp', '_gt', '_pp_gt'])
    for mode, v in res['metrics'].items():
        assert v.dtype == torch.float16 and tuple(v.shape) == (7,) and bool(torch.isfinite(v.float()).all()), mode
    assert float(res['metrics'][''][0]) < 0.05          # abs_rel of the un-flipped prediction against the depth of its own fp64 anchor
