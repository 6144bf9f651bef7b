"""GPU: the ResNet networks on the MI355X -- the kernel cases of tests/resnet_cases.py (csrc/resnet.h), DepthResNet18 / PoseResNet18 and
one SelfSupModel step against the reference's fixture (tests/golden/resnet.pt) and against the ATen twin on the same device, run-to-run
reproducibility, FlatAdam against torch.optim.Adam on the twin, and the eval mode."""
import copy

import pytest
import torch

import parity_cases as P
import resnet_cases as C

pytestmark = pytest.mark.gpu
_ids = lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s)       # noqa: E731


def _dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950' and _lib.REQUIRE_CUDA and _lib.get().pnsfm_version() >= 8


# ---- data movement: bit-equal to ATen
@pytest.mark.parametrize('kind', C.POOL_KINDS)
@pytest.mark.parametrize('shape', C.POOL_SHAPES, ids=_ids)
def test_maxpool(shape, kind):
    C.maxpool_case(_dev(), shape, kind)


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('shape', C.PAD_SHAPES, ids=_ids)
def test_reflect_pad(shape, s):
    C.pad_case(_dev(), shape, s)


def test_reflect_pad_concatenation():
    C.pad_cat_case(_dev())


def test_reflect_pad_pitch():
    C.pad_pitch_case(_dev())


def test_conv3x3_reflect_wide_map():
    C.conv3x3_wide_case(_dev())


def test_reflect_pad_too_small():
    C.pad_too_small_case(_dev())


@pytest.mark.parametrize('m', [0, 1])
@pytest.mark.parametrize('shape', C.CROP_SHAPES, ids=_ids)
def test_crop_exact(shape, m):
    C.crop_case(_dev(), shape, m)


@pytest.mark.parametrize('n', [7, 8, 4096])
def test_affine(n):
    C.affine_case(_dev(), n)


# ---- 4 x ATen
@pytest.mark.parametrize('m', [0, 1])
@pytest.mark.parametrize('act', [1, 2, 3], ids=['elu', 'relu', 'disp'])
@pytest.mark.parametrize('shape', C.CROP_SHAPES, ids=_ids)
def test_act_crop(shape, act, m):
    C.act_crop_case(_dev(), shape, act, m)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('relu', [False, True], ids=['none', 'relu'])
@pytest.mark.parametrize('use_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('shape,path', C.BN_SHAPES, ids=[_ids(s) for s, _ in C.BN_SHAPES])
def test_batchnorm_act(shape, path, use_res, relu, training):
    C.bn_case(_dev(), shape, path, use_res, relu, training)


def test_batchnorm_act_grown_chunks():
    C.bn_case(_dev(), C.BN_BIG, 1, True, True, True)


@pytest.mark.parametrize('shape,path', [C.BN_SHAPES[2], C.BN_SHAPES[4]], ids=['fused', 'chunked'])
def test_batchnorm_act_large_mean(shape, path):
    C.bn_case(_dev(), shape, path, True, True, True, mean=1000.0, seed=25)


def test_batchnorm_act_two_steps():
    C.bn_two_steps_case(_dev())


def test_batchnorm_act_single_value():
    C.bn_single_value_case(_dev())


@pytest.mark.parametrize('shape', [C.BN_SHAPES[2][0], C.BN_SHAPES[4][0], C.BN_BIG], ids=['fused', 'chunked', 'grown'])
def test_batchnorm_act_reproducible(shape):
    C.bn_reproducible_case(_dev(), shape)


# ---- networks
def test_stage_vs_twin_f64():
    C.stage_case(_dev())


def test_depth_resnet18_vs_reference():
    C.depth_vs_fixture_case(_dev())


def test_pose_resnet18_vs_reference():
    C.pose_vs_fixture_case(_dev())


def test_depth_resnet18_vs_twin():
    C.depth_vs_twin_case(_dev())


def test_pose_resnet18_vs_twin():
    C.pose_vs_twin_case(_dev())


def test_depth_resnet_eval_is_stable():
    C.eval_is_stable_case(_dev())


def test_resnet_step_vs_reference():
    """One SelfSupModel(DepthResNet18, PoseResNet18) step against the reference's: the tolerances of tests/test_gpu_velsup.py."""
    model, dn, pn = C.our_step(_dev())
    out = C.run_step(model, _dev())
    C.check_step(out, C.step_named(dn, pn), C.fixture()['step'], 'step vs reference')


def test_resnet_step_vs_twin():
    from packnet_sfm.models.SelfSupModel import SelfSupModel
    model, dn, pn = C.our_step(_dev())
    td, tp = C.Twin(dn, 'depth'), C.Twin(pn, 'pose')
    twin = C.step_model(SelfSupModel, td, tp, _dev())
    out = C.run_step(model, _dev())
    ref = C.step_record(C.run_step(twin, _dev()), C.step_named(td.net, tp.net))
    C.check_step(out, C.step_named(dn, pn), ref, 'step vs twin')


def test_depth_resnet18_full_size_vs_twin_f64():
    """DepthResNet18 forward and backward at the training configuration's map size (192x640, batch 1) against the twin in fp64, network
    tolerances.  At this size the decoder's padded maps (642 columns) take the pitched layout and layer4.0's stride-2 convolutions
    (256 -> 512 onto 6x20) the stride-1 weight gradient; tools/resnet_bench.py runs the whole SelfSupModel step there."""
    size = (1, 3, 192, 640)
    dev = _dev()
    net = C.make_depth_net(dev).train()
    twin = copy.deepcopy(net).double().train()
    rgb = C.frames(size)[0].to(dev)
    a = net(rgb)['inv_depths']
    b = C.torch_forward(twin, rgb.double())
    assert tuple(a[0].shape) == (1, 1, 192, 640)
    for i in range(4):
        P.check(a[i].detach().double(), b[i].detach(), C.OUT_TOL, 'full-size inv_depth %d' % i)
    C.depth_scalar(a, dev).backward()
    C.depth_scalar(b, dev).backward()
    norms, samples = C.grad_record(twin.named_parameters())
    C.check_grads(net.named_parameters(), norms, samples, 'full-size depth vs fp64 twin')


def test_resnet_step_reproducible():
    """Two steps from the same state: loss and every gradient bit for bit (after one step in which the autotuner has chosen)."""
    runs = []
    for _ in range(3):
        model, dn, pn = C.our_step(_dev())
        out = C.run_step(model, _dev())
        runs.append((out['loss'].detach().clone(), [p.grad.clone() for _, p in C.step_named(dn, pn) if p.grad is not None],
                     [b.clone() for b in dn.buffers()]))
    assert torch.equal(runs[1][0], runs[2][0]) and len(runs[1][1]) == len(runs[2][1]) > 100
    for a, b in zip(runs[1][1] + runs[1][2], runs[2][1] + runs[2][2]):
        assert torch.equal(a, b)


def test_flat_adam_tracks_torch_adam_on_the_twin():
    """Three FlatAdam steps of DepthResNet18 against three torch.optim.Adam steps of the twin on a copy of the parameters, within the
    step tolerances at EVERY step: the scalar loss 1e-4 relative, the outputs 1e-3, every gradient norm 1e-2 max(ref, 1e-4 gmax).
    The twin runs in fp64 (its role as the oracle): Adam's first steps are lr * g / (|g| + eps), which turns round-off in small
    gradients into full-size steps, and the fp32 ATEN twin itself drifts from the fp64 one by 1.4e-3 of the outputs after ONE step at
    lr 1e-3 and by 2e-4 after two at lr 1e-4 (measured on the MI355X; the HIP network stayed closer to fp64 than ATen's fp32 did) -- an
    fp32 reference would spend the tolerance on its own error.  lr = 1e-5 keeps that drift small; each step must still move the outputs
    by more than 3x their tolerance (asserted), so a packed weight left stale by the optimizer would show in the next step's outputs
    and gradients.  At the end the trained parameters as a whole have followed the twin's: their 2-norm distance from the twin's is at
    most 5 % of the distance the twin's moved from the start.  An optimizer that skipped one of the three steps would be off by about
    a third of it, one that stepped from stale values or the wrong way by more; a sign flip in an element whose gradient is at round-off
    level costs 2 lr per step, so 5 % allows such flips in up to 6e-4 of the elements (2 sqrt(f) = 0.05) -- which is why the bound is
    on the whole set and not per tensor, where one flip in a 16-element bias would be 50 %."""
    from packnet_sfm.rccl.flat_adam import FlatAdam
    dev = _dev()
    net = C.make_depth_net(dev).train()
    twin = copy.deepcopy(net).double().train()
    lr = 1e-5
    trained = lambda m: [(n, p) for n, p in m.named_parameters() if '.fc.' not in n]          # noqa: E731
    opt = FlatAdam([{'params': [p for _, p in trained(net)], 'lr': lr}])
    topt = torch.optim.Adam([p for _, p in trained(twin)], lr=lr)
    rgb = C.frames()[0].to(dev)
    prev = None
    for step in range(3):
        opt.zero_grad()
        topt.zero_grad(set_to_none=True)
        a = net(rgb)['inv_depths']
        b = C.torch_forward(twin, rgb.double())
        for i in range(4):
            print('step %d inv_depth %d: deviation %.2e' % (step, i, P.err(a[i].detach().double(), b[i].detach())))
            P.check(a[i].detach().double(), b[i].detach(), C.OUT_TOL, 'step %d inv_depth %d' % (step, i))
        if prev is not None:
            moved = max(P.err(b[i].detach(), prev[i]) for i in range(4))
            print('step %d: outputs moved by %.2e of their maximum' % (step, moved))
            assert moved > 3 * C.OUT_TOL, 'the optimizer step moved the outputs by %.2e only: the test could not see a stale weight' % moved
        prev = [t.detach().clone() for t in b]
        la, lb = C.depth_scalar(a, dev), C.depth_scalar(b, dev)
        P.check(la.detach().double().reshape(1), lb.detach().reshape(1), 1e-4, 'step %d loss' % step)
        la.backward()
        lb.backward()
        norms, _ = C.grad_record(trained(twin))
        C.check_grads(trained(net), norms, None, 'step %d' % step, norm_tol=1e-2, rel_floor=1e-4)
        opt.step()
        topt.step()
    start = C.build_params(C.state_shapes(net), C.DEPTH_SEED)
    dist2 = dev2 = 0.0
    for (n, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        if '.fc.' in n:
            assert torch.equal(p.detach().cpu(), start[n])
            continue
        dist2 += float((q.detach().cpu() - start[n].double()).norm()) ** 2
        dev2 += float((p.detach().double() - q.detach()).norm()) ** 2
    print('distance from the twin / distance moved: %.2e' % ((dev2 / dist2) ** 0.5))
    assert dist2 > 0 and dev2 <= (5e-2 ** 2) * dist2
