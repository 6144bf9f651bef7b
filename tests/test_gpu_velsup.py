"""GPU: the velocity-supervision kernels (csrc/velocity.h) on the MI355X -- the cases of tests/velsup_cases.py, plus the full VelSupModel
training step (PackNet01 + PoseNet + both losses, forward and backward) against the reference's composed step in
tests/golden/velsup.pt['step'] and its run-to-run reproducibility."""
import random

import pytest
import torch

import parity_cases as P
import velsup_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950' and _lib.REQUIRE_CUDA


@pytest.mark.parametrize('shape', C.SHAPES, ids=lambda s: '%dx%d' % s)
def test_velocity_loss_vs_fp64(shape):
    C.kernel_case(_dev(), *shape)


@pytest.mark.parametrize('shape', C.REFERENCE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_velocity_loss_vs_reference(shape):
    C.reference_case(_dev(), *shape)


def test_velocity_loss_exact_rows():
    C.exact_case(_dev())


def test_velocity_loss_reproducible():
    C.reproducible_case(_dev())


def test_velocity_loss_module():
    C.module_case(_dev())


def test_velsup_model_contract():
    C.model_case(_dev())


def _velsup(device, fx):
    from oracle import packnet_oracle as O
    from packnet_sfm.models.VelSupModel import VelSupModel
    from packnet_sfm.networks.depth.PackNet01 import PackNet01
    from packnet_sfm.networks.pose.PoseNet import PoseNet
    sd = O.init_params(O.packnet01_param_shapes('1A'), seed=fx['depth_seed'])
    psd = O.init_params(O.posenet_param_shapes(2), seed=fx['pose_seed'])
    psd['pose_pred.bias'] = fx['pose_pred_bias'].clone()
    model = VelSupModel(velocity_loss_weight=fx['velocity_loss_weight'], **fx['loss_kwargs'], clip_loss=0.0, flip_lr_prob=0.0,
                        upsample_depth_maps=True, rotation_mode='euler')
    dn, pn = PackNet01(dropout=0.0, version='1A'), PoseNet(nb_ref_imgs=2)
    dn.load_state_dict(sd)
    pn.load_state_dict(psd)
    model.add_depth_net(dn)
    model.add_pose_net(pn)
    return model.to(device).train(), dn, pn


def _step_batch(fx):
    batch = dict(P.golden('step')['step_flip0']['batch'], pose_context=fx['pose_context'])
    assert C.checksum(batch['rgb'], *batch['rgb_context']) == fx['batch_checksum']
    return {k: ([t.to(_dev()) for t in v] if isinstance(v, list) else v.to(_dev())) for k, v in batch.items()}


def test_velsup_step_golden():
    """Full VelSupModel step vs the reference's loss and gradients: the checks and tolerances of test_training_step_golden
    (tests/test_gpu_parity.py), plus the velocity loss itself.  Dropping or mis-weighting the term moves the loss by more than 10x its
    tolerance (asserted by the fixture tool).  The gradient NORMS cannot tell the term's backward from its absence -- an L1 of lengths
    has a gradient of w / (B J) per context whatever the mismatch, which moves no pose_net norm by more than 1.9x its tolerance (10x
    was the aim) -- so the whole gradient of pose_pred.bias is compared as well, at the same 1e-2 in the 2-norm (which implies the norm
    check); the velocity term moves it by 2.5x that."""
    fx = C.fixture()['step']
    model, dn, pn = _velsup(_dev(), fx)
    random.seed(0)
    out = model(_step_batch(fx), progress=0.0)
    P.check(out['loss'], fx['loss'], 1e-4, 'loss')
    P.check(out['metrics']['velocity_loss'], fx['velocity_loss'], 1e-4, 'velocity loss')
    P.check(out['metrics']['smoothness_loss'], fx['smoothness_loss'], 1e-3, 'smoothness')
    d = 1.0 / out['inv_depths'][0].clamp(min=1e-6)
    dref = 1.0 / fx['inv_depth0'].clamp(min=1e-6)
    P.check(d, dref, 1e-3, 'depth (north-star 1e-3 rel)')
    out['loss'].backward()
    named = [('depth_net.' + n, p) for n, p in dn.named_parameters()] + [('pose_net.' + n, p) for n, p in pn.named_parameters()]
    gmax = max(fx['grad_norms'].values())
    worst = 0.0
    for n, p in named:
        ref = fx['grad_norms'][n]
        got = float(p.grad.norm())
        tol = 1e-2 * max(ref, 1e-4 * gmax)
        assert abs(got - ref) <= tol, 'grad norm %s: %.6e vs reference %.6e' % (n, got, ref)
        worst = max(worst, abs(got - ref) / max(ref, 1e-4 * gmax))
    print('worst relative grad-norm deviation vs reference: %.2e' % worst)
    got, ref = pn.pose_pred.bias.grad.cpu(), fx['pose_pred_bias_grad']
    dev = float((got - ref).norm()) / float(ref.norm())
    print('pose_pred.bias gradient: relative 2-norm deviation vs reference %.2e' % dev)
    assert dev <= 1e-2


def test_velsup_step_reproducible():
    """Two steps from the same state: loss and every gradient bit for bit (after one step in which the autotuner, which times
    candidates, has made its choices)."""
    fx = C.fixture()['step']
    model, dn, pn = _velsup(_dev(), fx)
    params = list(dn.parameters()) + list(pn.parameters())
    runs = []
    for _ in range(3):
        model.zero_grad(set_to_none=True)
        random.seed(0)
        out = model(_step_batch(fx), progress=0.0)
        out['loss'].backward()
        runs.append((out['loss'].detach().clone(), out['metrics']['velocity_loss'].clone(), [p.grad.clone() for p in params]))
    assert torch.equal(runs[1][0], runs[2][0]) and torch.equal(runs[1][1], runs[2][1])
    for a, b in zip(runs[1][2], runs[2][2]):
        assert torch.equal(a, b)
