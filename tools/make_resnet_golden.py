"""Write tests/golden/resnet.pt: the REFERENCE's outputs for the ResNet network cases of tests/resnet_cases.py.

    python tools/make_resnet_golden.py

Runs on the CPU where a reference checkout is present; loads it through oracle._refstubs (imports only, nothing is copied).  The
reference's encoder sits on torchvision.models, which is not installed: BEFORE the stubs are installed this tool registers its own
stand-in for `torchvision.models` -- ResNet, resnet.BasicBlock, resnet18, resnet34, written here from the published architecture with
torchvision's attribute names (conv1, bn1, layer{1..4}, downsample, fc) -- and an empty `torchvision.transforms`.  The reference's
DepthResNet, PoseResNet and SelfSupModel are then imported and run as they are.

The fixture holds data only and no weights: parameters come from resnet_cases.build_params (shapes -> seeded tensors), frames from
resnet_cases.frames.

  'keys'   {'depth', 'pose'}: name -> shape of the two reference networks' state dicts
  'depth'  DepthResNet('18') on frames [2, 3, 64, 96], train mode: the four inv_depths, gradient norms and 8 samples per parameter for the
           scalar resnet_cases.depth_scalar, the running statistics of bn1 and layer4.1.bn2 after the step, and the eval-mode output
           after that step
  'pose'   PoseResNet('18') on the same frames and their two contexts: the [2, 2, 6] output and its gradients for pose_scalar
  'step'   one SelfSupModel step on those networks (loss configuration of tests/golden/step.pt['step_flip0'], flip off, one thread):
           loss, metrics, inv_depths[0], gradient norms and samples

Conditioning.  BatchNorm over the 12 values per channel that layer4 sees at 64 x 96, batch 2, amplifies round-off.  Every case is also
run with the reference in fp64, and the tool ASSERTS that the reference's own fp32 results lie within a quarter of every tolerance the
tests apply (resnet_cases: OUT_TOL, GNORM_TOL, STAT_TOL; the step's 1e-4 / 1e-3 / 1e-2).  They do at 64 x 96, batch 2 (the printed
margins), so that size is kept; were they not, the size would have to grow (128 x 192, then batch 3), never the tolerance."""
import copy
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


# ---- the stand-in for torchvision.models (architecture of He et al. 2015, attribute names of torchvision)
class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out = out + identity
        return self.relu(out)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


def _unavailable(*a, **k):
    raise NotImplementedError('not part of the stand-in')


def install_torchvision_stand_in():
    assert 'torchvision' not in sys.modules, 'a torchvision is already imported'
    tv, models, resnet, transforms = (types.ModuleType(n) for n in ('torchvision', 'torchvision.models', 'torchvision.models.resnet',
                                                                   'torchvision.transforms'))
    resnet.BasicBlock, resnet.Bottleneck, resnet.ResNet, resnet.model_urls = BasicBlock, _unavailable, ResNet, {}
    models.ResNet, models.resnet = ResNet, resnet
    models.resnet18 = lambda pretrained=False, **k: ResNet(BasicBlock, [2, 2, 2, 2])
    models.resnet34 = lambda pretrained=False, **k: ResNet(BasicBlock, [3, 4, 6, 3])
    models.resnet50 = models.resnet101 = models.resnet152 = _unavailable
    tv.models, tv.transforms = models, transforms
    for m in (tv, models, resnet, transforms):
        sys.modules[m.__name__] = m


def quarter(a, b, tol, what, floor=0.0):
    """The reference's fp32 result `a` against its fp64 result `b`: within tol / 4 of b's maximum."""
    e = float((a.double() - b.double()).abs().max() / max(float(b.abs().max()), floor, 1e-30))
    print('    %-44s fp32 vs fp64 %.2e  (allowed %.2e)' % (what, e, tol / 4))
    assert e <= tol / 4, '%s: the reference itself is off by %.2e, more than a quarter of %.1e: raise the size' % (what, e, tol)


def quarter_norms(n32, n64, tol, rel_floor, what):
    gmax = max(n64.values())
    worst = max(abs(n32[k] - n64[k]) / max(n64[k], rel_floor * gmax) for k in n64)
    print('    %-44s fp32 vs fp64 %.2e  (allowed %.2e)' % (what + ' gradient norms', worst, tol / 4))
    assert worst <= tol / 4, '%s: gradient norms of the reference are off by %.2e: raise the size' % (what, worst)


def main():
    install_torchvision_stand_in()
    import resnet_cases as C
    for name in [n for n in sys.modules if n == 'packnet_sfm' or n.startswith('packnet_sfm.')]:
        del sys.modules[name]
    if os.path.join(ROOT, 'packnet-sfm_amd') in sys.path:
        sys.path.remove(os.path.join(ROOT, 'packnet-sfm_amd'))
    from oracle import pin_against_reference as pin           # installs oracle._refstubs and imports the reference's modules
    from packnet_sfm.networks.depth.DepthResNet import DepthResNet as RefDepthResNet
    from packnet_sfm.networks.pose.PoseResNet import PoseResNet as RefPoseResNet
    import packnet_sfm.networks.depth.DepthResNet as RD
    assert RD.__file__.startswith(pin._refstubs.REFERENCE), RD.__file__
    torch.set_num_threads(1)
    torch.manual_seed(0)
    cpu = torch.device('cpu')

    def nets(dtype):
        dn, pn = RefDepthResNet(version='18'), RefPoseResNet(version='18')
        dn.load_state_dict(C.build_params(C.state_shapes(dn), C.DEPTH_SEED))
        pn.load_state_dict(C.build_params(C.state_shapes(pn), C.POSE_SEED))
        return dn.to(dtype), pn.to(dtype)

    dn, pn = nets(torch.float32)
    fx = {'size': C.SIZE, 'keys': {'depth': C.state_shapes(dn), 'pose': C.state_shapes(pn)}}

    print('depth')
    dn64, pn64 = nets(torch.float64)
    fx['depth'] = C.depth_record(lambda rgb: dn(rgb)['inv_depths'], dn, cpu)
    d64 = C.depth_record(lambda rgb: dn64(rgb)['inv_depths'], dn64, cpu)
    for i in range(4):
        quarter(fx['depth']['inv_depths'][i], d64['inv_depths'][i], C.OUT_TOL, 'inv_depth %d' % i)
    quarter(fx['depth']['eval'], d64['eval'], C.OUT_TOL, 'eval output')
    for k in d64['stats']:
        quarter(fx['depth']['stats'][k], d64['stats'][k], C.STAT_TOL, k)
    quarter_norms(fx['depth']['grad_norms'], d64['grad_norms'], C.GNORM_TOL, 1e-3, 'depth')
    assert 'encoder.encoder.fc.weight' not in fx['depth']['grad_norms'] and len(fx['depth']['grad_norms']) == len(list(dn.parameters())) - 2

    print('pose')
    fx['pose'] = C.pose_record(lambda t, c: pn(t, c), pn, cpu)
    p64 = C.pose_record(lambda t, c: pn64(t, c), pn64, cpu)
    quarter(fx['pose']['pose'], p64['pose'], C.OUT_TOL, 'pose')
    quarter_norms(fx['pose']['grad_norms'], p64['grad_norms'], C.GNORM_TOL, 1e-3, 'pose')

    print('step')

    def step(dtype):
        d, p = nets(dtype)
        model = C.step_model(pin.RefSelfSup, d, p, cpu).to(dtype)
        import random
        random.seed(0)
        batch = C.step_batch(cpu, dtype)
        # the fp64 run: the reference's loss casts the intrinsics with K.float() (multiview_photometric_loss.py:156-157) and builds its
        # identity poses as torch.float (geometry/pose.py:35); for this run only, .float() leaves a double tensor as it is, identity
        # poses are fp64 and so is the default dtype
        to_float, identity = torch.Tensor.float, pin.RefPose.__dict__['identity']
        torch.set_default_dtype(dtype)
        if dtype == torch.float64:
            pin.RefPose.identity = classmethod(lambda cls, N=1, device=None, dtype=None: identity.__func__(cls, N, device, torch.float64))
            torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else to_float(self, *a, **k)
        try:
            out = model(batch, progress=0.0)
            out['loss'].backward()
        finally:
            torch.Tensor.float, pin.RefPose.identity = to_float, identity
            torch.set_default_dtype(torch.float32)
        return C.step_record(out, C.step_named(d, p))

    fx['step'] = step(torch.float32)
    s64 = step(torch.float64)
    quarter(fx['step']['loss'].reshape(1), s64['loss'].reshape(1), 1e-4, 'loss')
    quarter(fx['step']['smoothness_loss'].reshape(1), s64['smoothness_loss'].reshape(1), 1e-3, 'smoothness')
    quarter(1.0 / fx['step']['inv_depth0'].clamp(min=1e-6), 1.0 / s64['inv_depth0'].clamp(min=1e-6), 1e-3, 'depth')
    quarter_norms(fx['step']['grad_norms'], s64['grad_norms'], 1e-2, 1e-4, 'step')
    print('    loss %.7f  photometric %.7f  smoothness %.7f' % (float(fx['step']['loss']), float(fx['step']['photometric_loss']),
                                                                float(fx['step']['smoothness_loss'])))
    assert all(bool(torch.isfinite(t).all()) for t in fx['depth']['inv_depths']) and bool(torch.isfinite(fx['step']['loss']).all())
    out = os.path.join(ROOT, 'tests', 'golden', 'resnet.pt')
    torch.save(fx, out)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
