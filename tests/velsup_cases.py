"""Velocity-supervision cases (csrc/velocity.h: velocity_loss_fwd_kernel / velocity_loss_bwd_kernel; HF.velocity_loss,
packnet_sfm.losses.velocity_loss.VelocityLoss, packnet_sfm.models.VelSupModel.VelSupModel) shared by the emulated CPU tests
(tests/test_velsup_emulated.py) and the GPU tests (tests/test_gpu_velsup.py).

Inputs come from depth_eval_cases.uniform (an integer hash): the same numbers on every machine, no storage.  The reference's own
VelocityLoss on the (3,2) and (4,2) inputs and on the `exact` inputs is in tests/golden/velsup.pt (tools/make_velsup_golden.py,
which imports the builders below), with a bit-pattern checksum of every input it was run on.

Every kernel case is compared with an fp64 evaluation of the formula on the fp32 inputs,

    p[j,b] = |pred_j[b,:3,3]|, g[j,b] = |gt_j[b,:3,3]|, L = (1/J) sum_j mean_b |p - g|,
    dpred_j[b,:3,3] = upstream w sign(p - g) / (B J) pred_j[b,:3,3] / p,

with u = 2^-24:
    loss       |L - L64| <= 2 u (4 mean(p + g) + (B + J + 2) L64): a norm costs at most 4 roundings relative to itself, the B-term and
               the J-term sums (B + J) u relative, the factor 2 covers the divide and the weight
    total      the same bound + u |total|
    gradient   |d - d64| <= 16 u / (B J) componentwise (the true gradient is at most 1 / (B J) in magnitude)
    elsewhere  entries outside column 3, rows 0..2 are exactly zero
The inputs keep every |p - g| >= 1e-3 (p + g) (asserted in fp64), so no element sits near a sign flip and none is excluded.
Against the reference (fp32 as well) both bounds are doubled."""
import functools

import pytest
import torch

import parity_cases as P
from depth_eval_cases import checksum, uniform
from packnet_sfm.hip import _lib
from packnet_sfm.hip import functional as HF
from packnet_sfm.hip import ops

U = 2.0 ** -24
SHAPES = [(1, 1), (3, 2), (4, 2), (63, 1), (64, 1), (65, 1), (33, 2), (257, 2), (300, 3)]
REFERENCE_SHAPES = [(3, 2), (4, 2)]
MAX_CONTEXTS = 8
LOSS_IN, WEIGHT = 0.7321, 0.1


def fixture():
    return P.golden('velsup')


def _signed(shape, seed, lo, hi):
    """float64 values of magnitude in [lo, hi) with hash-chosen signs."""
    mag = lo + (hi - lo) * uniform(shape, seed)
    return torch.where(uniform(shape, seed + 1) < 0.5, -mag, mag)


@functools.lru_cache(maxsize=None)
def loss_inputs(B, J):
    """(pred, gt): two lists of J [B,4,4] fp32 CPU stacks.  Translations have components of magnitude 0.3..3 with mixed signs; the
    ground-truth lengths are 0.6..0.9 (even rows) or 1.2..2.0 (odd rows) times the predicted ones, so both signs of p - g occur.
    The rotation blocks and bottom rows hold unrelated non-zero values: nothing but column 3, rows 0..2 may be read."""
    pred, gt = [], []
    for j in range(J):
        seed = 1000 * B + 10 * j
        mp, mg = _signed((B, 4, 4), seed, 0.5, 5.0), _signed((B, 4, 4), seed + 2, 0.5, 5.0)
        tp, tg = _signed((B, 3), seed + 4, 0.3, 3.0), _signed((B, 3), seed + 6, 0.3, 3.0)
        f = torch.where(torch.arange(B) % 2 == 0, 0.6 + 0.3 * uniform((B,), seed + 8), 1.2 + 0.8 * uniform((B,), seed + 8))
        if j % 2:
            f = f.flip(0) if B > 1 else 1.0 / f
        tg = tg * (f * tp.norm(dim=1) / tg.norm(dim=1))[:, None]
        mp[:, :3, 3], mg[:, :3, 3] = tp, tg
        pred.append(mp.float().contiguous())
        gt.append(mg.float().contiguous())
    return pred, gt


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """The (4,2) inputs with two special rows: context 0, row 1 has its predicted translation bit-copied from the ground truth
    (p == g); context 1, row 2 has predicted translation (0, 0, 0) against a non-zero ground truth (p == 0)."""
    pred, gt = loss_inputs(4, 2)
    pred = [t.clone() for t in pred]
    pred[0][1, :3, 3] = gt[0][1, :3, 3]
    pred[1][2, :3, 3] = 0.0
    return pred, gt


def formula64(pred, gt, weight=1.0, loss_in=None):
    """fp64 evaluation on the given (fp32) inputs -> dict(p, g [J,B], loss, total, grads: list of J [B,4,4])."""
    J, B = len(pred), pred[0].shape[0]
    tp = torch.stack([t.double()[:, :3, 3] for t in pred])
    tg = torch.stack([t.double()[:, :3, 3] for t in gt])
    p, g = tp.norm(dim=2), tg.norm(dim=2)
    loss = (p - g).abs().mean(dim=1).sum() / J
    total = weight * loss + (0.0 if loss_in is None else float(loss_in))
    c = weight * torch.sign(p - g) / (B * J) / p.clamp(min=1e-300)
    c = torch.where(p > 0, c, torch.zeros_like(c))
    grads = []
    for j in range(J):
        d = torch.zeros(B, 4, 4, dtype=torch.float64)
        d[:, :3, 3] = c[j][:, None] * tp[j]
        grads.append(d)
    return dict(p=p, g=g, loss=loss, total=total, grads=grads)


def assert_separated(pred, gt):
    r = formula64(pred, gt)
    assert bool(((r['p'] - r['g']).abs() >= 1e-3 * (r['p'] + r['g'])).all()), 'an element sits near the sign flip of p - g'
    if r['p'].numel() > 1:
        assert bool((r['p'] > r['g']).any()) and bool((r['p'] < r['g']).any()), 'both signs of p - g must occur'
    return r


def loss_bound(r, B, J, factor=1.0):
    return factor * 2 * U * (4 * float((r['p'] + r['g']).mean()) + (B + J + 2) * float(r['loss']))


def _run(pred, gt, device, weight=1.0, loss_in=None):
    """One forward and backward of HF.velocity_loss on `device` -> (total, L, [gradients], gradient of loss_in | None), on the CPU."""
    pd = [t.clone().to(device).requires_grad_(True) for t in pred]      # the builders' tensors are cached: never touch them
    gd = [t.to(device) for t in gt]
    li = None if loss_in is None else torch.tensor([loss_in], dtype=torch.float32, device=device, requires_grad=True)
    total, L = HF.velocity_loss(pd, gd, weight=weight, loss_in=li)
    assert total.dim() == 0 and L.dim() == 0 and total.requires_grad and not L.requires_grad
    total.backward()
    return total.detach().cpu(), L.detach().cpu(), [t.grad.cpu() for t in pd], None if li is None else li.grad.cpu()


def _check_grads(got, want, B, J, factor, what):
    mask = torch.zeros(4, 4, dtype=torch.bool)
    mask[:3, 3] = True
    for j in range(J):
        assert got[j].dtype == torch.float32 and tuple(got[j].shape) == (B, 4, 4)
        assert bool((got[j][:, ~mask] == 0).all()), '%s: context %d has a non-zero entry outside column 3, rows 0..2' % (what, j)
        err = float((got[j].double() - want[j].double()).abs().max())
        print('%s: context %d gradient error %.3e (bound %.3e)' % (what, j, err, factor * 16 * U / (B * J)))
        assert err <= factor * 16 * U / (B * J), '%s: context %d gradient error %.3e' % (what, j, err)


def kernel_case(device, B, J):
    """Forward and backward against the fp64 formula: once with w = 1 and no loss_in, once with w = 0.1 and a loss_in."""
    pred, gt = loss_inputs(B, J)
    r = assert_separated(pred, gt)
    total, L, grads, _ = _run(pred, gt, device)
    bound = loss_bound(r, B, J)
    print('(%d,%d) w=1: L %.9g, fp64 %.9g, error %.3e (bound %.3e)' % (B, J, float(L), float(r['loss']), abs(float(L) - float(r['loss'])), bound))
    assert abs(float(L.double()) - float(r['loss'])) <= bound
    assert torch.equal(total, L)                                     # 1 * L is exact
    _check_grads(grads, r['grads'], B, J, 1.0, '(%d,%d) w=1' % (B, J))
    r2 = formula64(pred, gt, WEIGHT, torch.tensor(LOSS_IN, dtype=torch.float32))
    total2, L2, grads2, dli = _run(pred, gt, device, WEIGHT, LOSS_IN)
    err = abs(float(total2.double()) - float(r2['total']))
    print('(%d,%d) w=0.1: total %.9g, fp64 %.9g, error %.3e (bound %.3e)' % (B, J, float(total2), float(r2['total']), err, bound + U * abs(float(total2))))
    assert err <= bound + U * abs(float(total2))
    assert torch.equal(L2, L)
    _check_grads(grads2, r2['grads'], B, J, 1.0, '(%d,%d) w=0.1' % (B, J))
    assert torch.equal(dli, torch.ones(1))


def reference_case(device, B, J):
    """The reference's own VelocityLoss (fp32, CPU) on the same inputs: both bounds doubled."""
    pred, gt = loss_inputs(B, J)
    fx = fixture()['loss'][(B, J)]
    assert checksum(*pred, *gt) == fx['checksum'], 'the inputs are not the ones the fixture was made from'
    r = formula64(pred, gt)
    _, L, grads, _ = _run(pred, gt, device)
    err = abs(float(L.double()) - float(fx['loss'].double()))
    print('(%d,%d) vs reference: L %.9g, reference %.9g, error %.3e (bound %.3e)' % (B, J, float(L), float(fx['loss']), err, loss_bound(r, B, J, 2.0)))
    assert err <= loss_bound(r, B, J, 2.0)
    _check_grads(grads, fx['grads'], B, J, 2.0, '(%d,%d) vs reference' % (B, J))


def exact_case(device):
    """p == g (bit-copied translation) and p == 0: the gradient is exactly zero, nothing is NaN, and a p == g term adds exactly 0."""
    pred, gt = exact_inputs()
    fx = fixture()['exact']
    assert checksum(*pred, *gt) == fx['checksum']
    total, L, grads, _ = _run(pred, gt, device)
    assert all(bool(torch.isfinite(t).all()) for t in grads + [total, L])
    assert bool((grads[0][1] == 0).all()) and bool((grads[1][2] == 0).all())
    assert bool((fx['grads'][0][1] == 0).all()) and bool((fx['grads'][1][2] == 0).all())      # ... as in the reference
    r = formula64(pred, gt)
    assert abs(float(L.double()) - float(fx['loss'].double())) <= loss_bound(r, 4, 2, 2.0)
    _check_grads(grads, fx['grads'], 4, 2, 2.0, 'exact vs reference')
    # the p == g term is exactly 0: a batch of that row alone has loss 0 and leaves loss_in untouched, bit for bit
    one_p, one_g = [pred[0][1:2].clone()], [gt[0][1:2].clone()]
    total1, L1, g1, _ = _run(one_p, one_g, device, WEIGHT, LOSS_IN)
    assert float(L1) == 0.0 and torch.equal(total1, torch.tensor(LOSS_IN, dtype=torch.float32)) and bool((g1[0] == 0).all())


def reproducible_case(device, B=257, J=2):
    pred, gt = loss_inputs(B, J)
    a, b = _run(pred, gt, device, WEIGHT, LOSS_IN), _run(pred, gt, device, WEIGHT, LOSS_IN)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def module_case(device):
    """VelocityLoss on Pose objects; list lengths; float64 ground truth; dtype errors; the context limit."""
    from packnet_sfm.geometry.pose import Pose
    from packnet_sfm.losses.velocity_loss import VelocityLoss
    pred, gt = loss_inputs(3, 2)
    pd = [t.clone().to(device).requires_grad_(True) for t in pred]      # the builders' tensors are cached: never touch them
    gd = [t.to(device) for t in gt]
    mod = VelocityLoss(some_option_of_another_loss=1)
    out = mod([Pose(t) for t in pd], gd)
    want, _ = HF.velocity_loss([t.detach() for t in pd], gd)
    assert tuple(out['loss'].shape) == (1,) and torch.equal(out['loss'].detach(), want.reshape(1))
    assert torch.equal(out['metrics']['velocity_loss'], want) and not out['metrics']['velocity_loss'].requires_grad
    out['loss'].sum().backward()
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in pd)
    with pytest.raises(AssertionError):
        mod([Pose(t) for t in pd], gd[:1])
    # float64 ground truth (what a dataset delivers) is cast once: storing a translation as fp32 moves each norm by at most one u
    gt64 = [t.double() * (1.0 + 1e-9) + 1e-10 for t in gt]
    assert any(not torch.equal(t.float().double(), t) for t in gt64)
    L64 = mod([Pose(t.detach()) for t in pd], [t.to(device) for t in gt64])['loss']
    L32 = mod([Pose(t.detach()) for t in pd], [t.float().to(device) for t in gt64])['loss']
    assert L64.dtype == torch.float32 and abs(float(L64) - float(L32)) <= 2 * U * float(L32)
    with pytest.raises(TypeError, match='pred_mats'):
        HF.velocity_loss([t.detach().half() for t in pd], gd)
    with pytest.raises(TypeError, match='gt_mats'):
        HF.velocity_loss([t.detach() for t in pd], [t.half() for t in gd])
    with pytest.raises(TypeError, match='loss_in'):
        HF.velocity_loss([t.detach() for t in pd], gd, loss_in=torch.zeros(1, dtype=torch.float64, device=device))
    many = MAX_CONTEXTS + 1
    with pytest.raises(_lib.HipError, match=r'1\.\.%d contexts \(got %d\)' % (MAX_CONTEXTS, many)):
        ops.velocity_loss_forward([pd[0].detach()] * many, [gd[0]] * many, 1.0)
    with pytest.raises(_lib.HipError, match=r'1\.\.%d contexts \(got %d\)' % (MAX_CONTEXTS, many)):
        ops.velocity_loss_backward([pd[0].detach()] * many, [gd[0]] * many, 1.0, torch.ones(1, device=device))
    full, _ = HF.velocity_loss([pd[0].detach()] * MAX_CONTEXTS, [gd[0]] * MAX_CONTEXTS)        # the maximum itself runs
    one, _ = HF.velocity_loss([pd[0].detach()], [gd[0]])
    assert abs(float(full) - float(one)) <= 2 * MAX_CONTEXTS * U * float(one)


# ---- VelSupModel on stub networks (the kernels of the loss are the real ones; the networks are not what is tested here)
class _StubDepth(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.7))

    def forward(self, rgb):
        d = 0.1 + self.w * rgb.mean(1, keepdim=True)
        scales = [d, d[:, :, ::2, ::2].contiguous(), d[:, :, ::4, ::4].contiguous(), d[:, :, ::8, ::8].contiguous()]
        return {'inv_depths': scales if self.training else d}


class _StubPose(torch.nn.Module):
    def __init__(self, J=2):
        super().__init__()
        self.v = torch.nn.Parameter(torch.tensor([[0.20, 0.05, -0.10, 0.010, -0.020, 0.010],
                                                  [-0.20, -0.05, 0.10, -0.010, 0.020, -0.010]])[:J])

    def forward(self, image, contexts):
        return self.v[None].expand(image.shape[0], -1, -1) * (0.5 + image.mean(dim=(1, 2, 3)))[:, None, None]


def _model(cls, device, **kwargs):
    m = cls(num_scales=4, ssim_loss_weight=0.85, smooth_loss_weight=0.001, photometric_reduce_op='min', automask_loss=True,
            clip_loss=0.0, flip_lr_prob=0.0, upsample_depth_maps=True, rotation_mode='euler', **kwargs)
    m.add_depth_net(_StubDepth())
    m.add_pose_net(_StubPose())
    return m.to(device)


def _batch(device, B=2, H=16, W=24):
    rgb = uniform((B, 3, H, W), 901).float()
    ctx = [uniform((B, 3, H, W), 902 + i).float() for i in range(2)]
    K = torch.tensor([[0.58 * W, 0., 0.5 * W], [0., 1.92 * H, 0.5 * H], [0., 0., 1.]]).repeat(B, 1, 1)
    poses = []
    for i in range(2):
        T = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)            # float64, as a dataset delivers them
        T[:, :3, 3] = _signed((B, 3), 910 + 2 * i, 0.1, 0.4)
        poses.append(T)
    batch = {'rgb': rgb, 'rgb_context': ctx, 'rgb_original': rgb, 'rgb_context_original': ctx, 'intrinsics': K, 'pose_context': poses}
    return {k: ([t.to(device) for t in v] if isinstance(v, list) else v.to(device)) for k, v in batch.items()}


def model_case(device):
    from packnet_sfm.models.SelfSupModel import SelfSupModel
    from packnet_sfm.models.VelSupModel import VelSupModel
    vel, base, vel0 = _model(VelSupModel, device), _model(SelfSupModel, device), _model(VelSupModel, device, velocity_loss_weight=0)
    assert vel.velocity_loss_weight == 0.1
    assert 'gt_pose' in vel.train_requirements and 'gt_pose' not in base.train_requirements
    assert isinstance(vel.train_requirements, list)
    batch = _batch(device)
    vel.train(), base.train(), vel0.train()
    out, ref, out0 = vel(dict(batch)), base(dict(batch)), vel0(dict(batch))
    assert tuple(out['loss'].shape) == tuple(ref['loss'].shape) == (1,)
    assert 'velocity_loss' in out['metrics'] and 'velocity_loss' not in ref['metrics'] and 'photometric_loss' in out['metrics']
    v = out['metrics']['velocity_loss']
    want, _ = HF.velocity_loss([p.mat.detach() for p in out['poses']], batch['pose_context'])
    assert torch.equal(v, want) and float(v) > 0
    r = float(ref['loss'].detach().double()) + 0.1 * float(v.double())
    assert abs(float(out['loss'].detach()) - r) <= 2 * U * abs(r)                              # loss = self-supervised + w * velocity
    assert torch.equal(out0['loss'], ref['loss'])                                        # weight 0: the self-supervised loss, bit for bit
    out['loss'].backward(), ref['loss'].backward()
    gv, gr = vel.pose_net.v.grad, base.pose_net.v.grad
    assert bool(torch.isfinite(gv).all()) and not torch.equal(gv[:, :3], gr[:, :3])   # the velocity term reaches the translations
    P.check(gv[:, 3:], gr[:, 3:], 1e-5, 'rotation gradients are untouched by the velocity term')
    P.check(vel.depth_net.w.grad, base.depth_net.w.grad, 1e-5, 'the depth gradient is untouched by the velocity term')
    missing = {k: t for k, t in batch.items() if k != 'pose_context'}
    with pytest.raises(KeyError, match='gt_pose'):
        vel(missing)
    vel.eval(), base.eval()
    with torch.no_grad():
        ev, eb = vel(missing), base(missing)
    assert 'loss' not in ev and set(ev) == set(eb)
    assert torch.equal(ev['inv_depths'], eb['inv_depths'])
    assert all(torch.equal(a.mat, b.mat) for a, b in zip(ev['poses'], eb['poses']))


def product_modules_stand_alone():
    """The two product modules (and the kernel header) import neither the oracle nor the reference checkout."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'packnet-sfm_amd')
    for rel in ('packnet_sfm/losses/velocity_loss.py', 'packnet_sfm/models/VelSupModel.py', 'csrc/velocity.h'):
        src = open(os.path.join(root, rel)).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|emu_loader|build_emu)\b', src, re.M), rel
        assert 'sys.path' not in src and '_refstubs' not in src, rel
