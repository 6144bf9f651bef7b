"""Write tests/golden/velsup.pt: the REFERENCE's outputs for the velocity-supervision cases of tests/velsup_cases.py.

    python tools/make_velsup_golden.py

Runs on the CPU where a reference checkout is present; loads it through oracle._refstubs (imports only, nothing is copied).  The
fixture holds data only:

  'loss'   {(3,2), (4,2)}: the reference's VelocityLoss on velsup_cases.loss_inputs -- loss, the gradient with respect to each predicted
           matrix, and a bit-pattern checksum of the inputs, which the tests rebuild from the same integer hash
  'exact'  the same for velsup_cases.exact_inputs (one row with p == g, one with p == 0)
  'step'   one full training step at 64x96, B=1 on the set-up of case_step in oracle/pin_against_reference.py (its parameter seeds 42 /
           43, its pose_pred.bias, its loss configuration, flip off, and the very frames of tests/golden/step.pt['step_flip0'], so the
           gradients are comparable with that fixture's) plus two ground-truth poses whose translation lengths are about 0.5x and 2x
           the predicted ones.  The reference's VelSupModel cannot be constructed (models/VelSupModel.py:26 indexes a list with a
           string), so the total is composed here from the reference's SelfSupModel output and the reference's VelocityLoss at weight
           0.1 -- exactly what VelSupModel.forward:47-51 computes.  Stored under the keys of the `step` fixture, without the frames
           (the test takes them from step.pt; their checksum is stored).

The tool checks that the step case can tell the velocity term from its absence: the loss moves by more than 10x the step test's loss
tolerance, and the gradient of pose_pred.bias by more than 2x its tolerance.  Gradient NORMS alone cannot (see step_entry)."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'packnet-sfm_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WEIGHT = 0.1


def loss_entry(RefVelocityLoss, RefPose, pred, gt, checksum):
    pd = [t.clone().requires_grad_(True) for t in pred]
    out = RefVelocityLoss()([RefPose(t) for t in pd], [t.clone() for t in gt])
    assert tuple(out['loss'].shape) == (1,)
    out['loss'].sum().backward()
    return {'loss': out['loss'].detach()[0].clone(), 'grads': [t.grad.clone() for t in pd], 'checksum': checksum(*pred, *gt)}


def step_entry(pin, RefVelocityLoss, checksum):
    O = pin.O
    # one thread: with several, the reference's pose gradients (grid_sample's backward scatters with a thread-dependent order) change
    # in the last bits from run to run, and the fixture would not regenerate bit for bit
    torch.set_num_threads(1)
    fx0 = torch.load(os.path.join(ROOT, 'tests', 'golden', 'step.pt'), weights_only=False)['step_flip0']
    B, H, W = 1, 64, 96
    batch = fx0['batch']
    assert tuple(batch['rgb'].shape) == (B, 3, H, W) and torch.equal(batch['intrinsics'], pin.kitti_K(B, H, W)) and not fx0['flip']
    sd = O.init_params(O.packnet01_param_shapes('1A'), seed=fx0['depth_seed'])
    psd = O.init_params(O.posenet_param_shapes(2), seed=fx0['pose_seed'])
    psd['pose_pred.bias'] = fx0['pose_pred_bias'].clone()
    assert (fx0['depth_seed'], fx0['pose_seed']) == (42, 43)

    def run(pose_context):
        model = pin.RefSelfSup(num_scales=4, ssim_loss_weight=0.85, occ_reg_weight=0.1, smooth_loss_weight=0.001, C1=1e-4, C2=9e-4,
                               photometric_reduce_op='min', disp_norm=True, clip_loss=0.0, progressive_scaling=0.0,
                               padding_mode='zeros', automask_loss=True, flip_lr_prob=0.0, rotation_mode='euler',
                               upsample_depth_maps=True)
        dn, pn = pin.RefPackNet01(dropout=0.0, version='1A'), pin.RefPoseNet(nb_ref_imgs=2)
        dn.load_state_dict(sd)
        pn.load_state_dict(psd)
        model.add_depth_net(dn)
        model.add_pose_net(pn)
        model.train()
        random.seed(0)
        out = model({k: (v if not isinstance(v, list) else list(v)) for k, v in batch.items()}, progress=0.0)
        names = ['depth_net.' + n for n, _ in dn.named_parameters()] + ['pose_net.' + n for n, _ in pn.named_parameters()]
        params = list(dn.parameters()) + list(pn.parameters())
        velocity = None
        if pose_context is not None:
            velocity = RefVelocityLoss()(out['poses'], pose_context)
            out['loss'] += WEIGHT * velocity['loss']                 # VelSupModel.forward:51
        return out, velocity, names, pin.grads_of(out['loss'].sum(), params)

    plain, _, names, g_plain = run(None)
    assert abs(float(plain['loss'].detach()) - float(fx0['loss'])) <= 1e-6 * abs(float(fx0['loss'])), 'the set-up is not step.pt\'s'
    # ground truth: the predicted transforms with their translations scaled by 0.5 and by 2 (rotations are not read by the loss)
    pose_context = []
    for pose, scale in zip(plain['poses'], (0.5, 2.0)):
        T = pose.mat.detach().clone()
        T[:, :3, 3] *= scale
        pose_context.append(T)
    out, velocity, names, g = run(pose_context)
    norms = {n: float(t.norm()) for n, t in zip(names, g)}
    # Can the step test tell the velocity term from its absence?
    # (1) forward: its loss tolerance is 1e-4 relative; dropping or mis-weighting the term must move the loss by more than 10x that
    moved = abs(float(out['loss'].detach()) - float(plain['loss'].detach())) / abs(float(out['loss'].detach()))
    assert moved > 10 * 1e-4, 'the velocity term moves the loss by %.2e only' % moved
    # (2) backward: the gradient-norm tolerance is 1e-2 * max(ref, 1e-4 * gmax).  The loss is an L1 of lengths, so its gradient is
    # w / (B J) times a unit vector WHATEVER the mismatch -- a larger mismatch cannot raise it -- and PoseNet scales its output by
    # 0.01: on pose_pred.bias the term has length 0.01 * 0.1 / 2 * sqrt(2) = 7.1e-4 against a photometric gradient of 2.8e-2.  No
    # pose_net NORM moves by 10x its tolerance (the largest move is 1.9x, printed below), so the fixture also stores the whole
    # gradient of pose_pred.bias, which the velocity term moves by 2.5x the same 1e-2 tolerance taken in the 2-norm.
    gmax = max(fx0['grad_norms'].values())
    ratios = {n: abs(norms[n] - fx0['grad_norms'][n]) / (1e-2 * max(fx0['grad_norms'][n], 1e-4 * gmax))
              for n in names if n.startswith('pose_net.')}
    best = max(ratios, key=ratios.get)
    print('  step: largest pose_net gradient-norm move / tolerance: %.2f (%s); 10 was asked for and is out of reach' % (ratios[best], best))
    k = names.index('pose_net.pose_pred.bias')
    bias_move = float((g[k] - g_plain[k]).norm()) / (1e-2 * float(g[k].norm()))
    print('  step: pose_pred.bias gradient moves by %.2f x its 2-norm tolerance' % bias_move)
    assert bias_move > 2.0
    p = [float(q.mat[0, :3, 3].norm()) for q in out['poses']]
    gn = [float(T[0, :3, 3].norm()) for T in pose_context]
    assert (p[0] - gn[0]) * (p[1] - gn[1]) < 0, 'one predicted length must lie above its target and one below'
    print('  step: loss %.7f (self-supervised %.7f), velocity %.7f, |t| predicted %s, ground truth %s' %
          (float(out['loss'].detach()), float(fx0['loss']), float(velocity['loss'].detach()), p, gn))
    return dict(depth_seed=42, pose_seed=43, pose_pred_bias=psd['pose_pred.bias'], loss_kwargs=fx0['loss_kwargs'], flip=False,
                velocity_loss_weight=WEIGHT, pose_context=pose_context, batch_checksum=checksum(batch['rgb'], *batch['rgb_context']),
                loss=out['loss'].detach(), velocity_loss=velocity['loss'].detach()[0].clone(),
                photometric_loss=out['metrics']['photometric_loss'], smoothness_loss=out['metrics']['smoothness_loss'],
                inv_depth0=out['inv_depths'][0].detach(), grad_norms=norms, pose_pred_bias_grad=g[k].clone(),
                grad_samples={n: t.flatten()[:: max(1, t.numel() // 8)][:8].clone() for n, t in zip(names, g)})


def main():
    import velsup_cases as C                     # our package first: the input builders
    inputs = {shape: C.loss_inputs(*shape) for shape in C.REFERENCE_SHAPES}
    exact = C.exact_inputs()
    checksum = C.checksum
    for pred, gt in inputs.values():
        C.assert_separated(pred, gt)
    for name in [n for n in sys.modules if n == 'packnet_sfm' or n.startswith('packnet_sfm.')]:
        del sys.modules[name]                    # ... then the reference's package of the same name
    sys.path.remove(os.path.join(ROOT, 'packnet-sfm_amd'))
    from oracle import pin_against_reference as pin          # installs oracle._refstubs and imports the reference's modules
    from packnet_sfm.losses.velocity_loss import VelocityLoss as RefVelocityLoss
    import packnet_sfm.losses.velocity_loss as RV
    assert RV.__file__.startswith(pin._refstubs.REFERENCE), RV.__file__
    torch.manual_seed(0)
    fx = {'loss': {shape: loss_entry(RefVelocityLoss, pin.RefPose, *inputs[shape], checksum) for shape in inputs},
          'exact': loss_entry(RefVelocityLoss, pin.RefPose, *exact, checksum)}
    for key, e in list(fx['loss'].items()) + [('exact', fx['exact'])]:
        assert all(bool(torch.isfinite(t).all()) for t in e['grads'])
        print(' ', key, 'loss %.9g' % float(e['loss']))
    assert bool((fx['exact']['grads'][0][1] == 0).all()) and bool((fx['exact']['grads'][1][2] == 0).all())
    fx['step'] = step_entry(pin, RefVelocityLoss, checksum)
    out = os.path.join(ROOT, 'tests', 'golden', 'velsup.pt')
    torch.save(fx, out)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
