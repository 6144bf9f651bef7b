"""GPU: fp16 evaluation / inference forward of PackNet01 ('1A', '1B') and PackNetSlim01 on the gfx950 fp16 kernels
(include/pnsfm.h "fp16 forward") -- per-op checks at the real layer shapes, networks against the float64 anchors, and the contract."""
import json
import os

import pytest
import torch

import half_cases as HC
import parity_cases as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---- per op at the PackNet01 layer shapes (192 x 640, batch 1): one per distinct layer class
@pytest.mark.parametrize('chans,Cout,H,W,ks', [
    ([3], 64, 192, 640, 5),            # stem
    ([64], 64, 192, 640, 7),           # conv1
    ([256], 64, 96, 320, 7),           # pack1, collapsed (composed 7x7 over the 4C packed channels)
    ([64], 128, 96, 320, 3),           # conv3 first 3x3
    ([128], 128, 48, 160, 3),          # 3x3 @ 48x160
    ([512], 256, 24, 80, 5),           # pack3 collapsed (5x5)
    ([256], 512, 12, 40, 3),           # 3x3 @ 12x40
    ([512], 512, 6, 20, 3),            # 3x3 @ 6x20 (K split)
    ([256], 512, 12, 40, 1),           # 1x1 shortcut
    ([64, 64, 1], 64, 192, 640, 3),    # iconv1: three sources, ragged
])
def test_conv_h16_layer_shapes(chans, Cout, H, W, ks):
    HC.conv_case(DEV, 1, chans, Cout, H, W, ks, seed=H + ks)


def test_other_ops_h16_layer_shapes():
    for fused in (1, 0):
        HC.groupnorm_case(DEV, 1, 64, 192, 640, res=False, fused=fused)
        HC.groupnorm_case(DEV, 1, 256, 24, 80, res=True, fused=fused)
    HC.conv3d_case(DEV, 1, 64, 96, 320, 8)
    HC.conv3d_case(DEV, 1, 32, 96, 320, 4)
    HC.movement_case(DEV, 1, 64, 96, 320)
    HC.invdepth_case(DEV, 1, 64, 192, 640)


# ---- networks at golden size
def _net(kind, collapse=None):
    from oracle import packnet_oracle as O
    if kind == 'slim':
        from packnet_sfm.networks.depth.PackNetSlim01 import PackNetSlim01
        fx = P.golden('slim')['packnetslim01']
        net = PackNetSlim01(dropout=0.0, version='1A')
        sd = O.init_params(O.packnet01_param_shapes('1A', ni=32, n1=32, d=4), seed=fx['seed'], randomize_affine=True)
        version = '1A'
    elif kind == '1B':
        from packnet_sfm.networks.depth.PackNet01 import PackNet01
        fx = P.golden('slim')['packnet01_1B']
        net = PackNet01(dropout=0.0, version='1B')
        sd = O.init_params(O.packnet01_param_shapes('1B'), seed=fx['seed'], randomize_affine=True)
        version = '1B'
    else:
        from packnet_sfm.networks.depth.PackNet01 import PackNet01
        fx = P.golden('network')['packnet01']
        net = PackNet01(dropout=0.0, version='1A')
        sd = O.init_params(O.packnet01_param_shapes('1A'), seed=fx['seed'], randomize_affine=False)
        version = '1A'
    net.load_state_dict(sd)
    if collapse is not None:
        for m in net.modules():
            if hasattr(m, '_use_collapsed'):
                m.collapse = collapse
    return net, sd, fx, version


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize('kind', ['1A', '1B', 'slim'])
@pytest.mark.parametrize('collapse', [True, False])
def test_network_half_vs_fp64(kind, collapse):
    from oracle import packnet_oracle as O
    net, sd, fx, version = _net(kind, collapse)
    net = net.to(DEV, dtype=torch.float16).eval()
    rgb = fx['rgb'].to(DEV).half()
    with torch.no_grad():
        y = net(rgb=rgb)['inv_depths']
        y2 = net(rgb=rgb)['inv_depths']
        sd16 = {k: v.to(DEV).half() for k, v in sd.items()}
        e16 = O.packnet01_forward(sd16, rgb, version=version, training=False)
    assert y.dtype == torch.float16 and tuple(y.shape) == tuple(fx['disps_f64'][0].shape)
    assert torch.equal(y, y2)
    anchor = fx['disps_f64'][0]
    r_hip, r_eager = _rel(y, anchor), _rel(e16, anchor)
    assert r_hip <= 1.5 * r_eager + 2e-4, (kind, collapse, r_hip, r_eager)


def test_half_contract():
    from packnet_sfm.networks.depth.PackNet01 import PackNet01
    net, sd, fx, _ = _net('1A')
    rgb = fx['rgb'].to(DEV)
    # fp32 -> half -> float gives the fp32 outputs of a fresh fp32 net with the same (fp16-rounded) weights
    net = net.to(DEV)
    with torch.no_grad():
        net.eval()(rgb=rgb)
    net = net.half()
    with torch.no_grad():
        net(rgb=rgb.half())
    net = net.float()
    fresh = PackNet01(dropout=0.0, version='1A')
    fresh.load_state_dict({k: v.half().float() for k, v in sd.items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(net(rgb=rgb)['inv_depths'], fresh(rgb=rgb)['inv_depths'])
    # mixed dtypes raise, both ways
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            net(rgb=rgb.half())
    net16 = net.half()
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            net16(rgb=rgb)
    # backward in fp16 raises
    net16.train()
    for m in net16.modules():
        if hasattr(m, '_use_collapsed'):
            m.collapse = False
    out = net16(rgb=rgb.half())['inv_depths'][0]
    with pytest.raises(NotImplementedError):
        out.float().sum().backward()


def test_full_size_half_eval_vs_fp64():
    """PackNet01 1A at 192 x 640 b1 (xavier weights): fp16 HIP vs the float64 oracle on the fp16-rounded weights and input, beside
    fp16 eager (MIOpen) and fp32 HIP; recorded in profiles/r07_half_parity.json."""
    from oracle import packnet_oracle as O
    from packnet_sfm.networks.depth.PackNet01 import PackNet01
    sd = O.init_params(O.packnet01_param_shapes('1A'), seed=7)
    sd = {k: v.half().float() for k, v in sd.items()}
    rgb = torch.rand((1, 3, 192, 640), generator=torch.Generator().manual_seed(7)).half()
    with torch.no_grad():
        ref = O.packnet01_forward({k: v.double() for k, v in sd.items()}, rgb.double(), version='1A', training=False)
        net = PackNet01(dropout=0.0, version='1A')
        net.load_state_dict(sd)
        net = net.to(DEV).eval()
        y32 = net(rgb=rgb.float().to(DEV))['inv_depths']
        net = net.half()
        y16 = net(rgb=rgb.to(DEV))['inv_depths']
        e16 = O.packnet01_forward({k: v.to(DEV).half() for k, v in sd.items()}, rgb.to(DEV), version='1A', training=False)

    def absrel(y):
        d, d0 = 1 / y.double().cpu().clamp(min=1e-6), 1 / ref.double().clamp(min=1e-6)
        return float(((d - d0).abs() / d0).mean())
    res = {'shape': [1, 3, 192, 640], 'anchor': 'oracle float64 on the fp16-rounded weights and input',
           'inv_depth_rel_l2': {'hip16': _rel(y16, ref), 'eager16': _rel(e16, ref), 'hip32': _rel(y32, ref)},
           'depth_abs_rel': {'hip16': absrel(y16), 'eager16': absrel(e16), 'hip32': absrel(y32)}}
    out = os.environ.get('PNSFM_HALF_PARITY_OUT')          # where to record the numbers (the committed copy: profiles/)
    if out:
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    assert y16.dtype == torch.float16
    assert res['inv_depth_rel_l2']['hip16'] <= 1.5 * res['inv_depth_rel_l2']['eager16'] + 2e-4, res


def test_half_out_of_scope_networks_raise():
    """PoseNet, PackNetSAN01 and SfmModel with fp16 context images have no fp16 path: a clear NotImplementedError, not a kernel's
    dtype check."""
    from packnet_sfm.models.SfmModel import SfmModel
    from packnet_sfm.networks.depth.PackNet01 import PackNet01
    from packnet_sfm.networks.depth.PackNetSAN01 import PackNetSAN01
    from packnet_sfm.networks.pose.PoseNet import PoseNet
    img = torch.rand((1, 3, 64, 96), device=DEV).half()
    pn = PoseNet(nb_ref_imgs=2).to(DEV).half().eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match='PoseNet'):
        pn(img, [img, img])
    san = PackNetSAN01(dropout=0.0, version='1A').to(DEV).half().eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match='PackNetSAN01'):
        san(rgb=img)
    m = SfmModel()
    m.add_depth_net(PackNet01(dropout=0.0, version='1A'))
    m.add_pose_net(PoseNet(nb_ref_imgs=2))
    m = m.to(DEV).half().eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match='rgb_context'):
        m({'rgb': img, 'rgb_context': [img, img]})


def test_collapsed_half_forward_runs_with_grad_backward_raises():
    """With grad enabled the fp16 forward runs in both packing forms; only the backward raises."""
    for collapse in (True, False):
        net, _, fx, _ = _net('1A', collapse)
        net = net.to(DEV).half().eval()
        out = net(rgb=fx['rgb'].to(DEV).half())['inv_depths']
        assert out.dtype == torch.float16 and out.requires_grad
        with pytest.raises(NotImplementedError):
            out.float().sum().backward()


def test_trainer_half_test_on_selfsup_model():
    """HorovodTrainer(dtype=torch.float16).test(module): the reference's `eval.py --half` path (module.to('cuda', float16), batches
    cast by sample_to_cuda) through SelfSupModel + compute_depth_metrics; parameters come out fp16 and the metrics are within fp16
    tolerance of the float32 run's."""
    import types
    from packnet_sfm.models.SelfSupModel import SelfSupModel
    from packnet_sfm.networks.depth.PackNet01 import PackNet01
    from packnet_sfm.networks.pose.PoseNet import PoseNet
    from packnet_sfm.trainers.horovod_trainer import HorovodTrainer
    from packnet_sfm.utils.depth import compute_depth_metrics, inv2depth
    from oracle import packnet_oracle as O
    g = torch.Generator().manual_seed(21)
    batches = [{'rgb': torch.rand((2, 3, 64, 96), generator=g), 'depth': 1 + 40 * torch.rand((2, 1, 64, 96), generator=g)}
               for _ in range(2)]
    sd = O.init_params(O.packnet01_param_shapes('1A'), seed=4, randomize_affine=True)

    class Loader(list):
        sampler = None

    class Wrapper(torch.nn.Module):                 # the surface of the reference's ModelWrapper that trainer.test touches
        def __init__(self):
            super().__init__()
            self.model = SelfSupModel()
            dn = PackNet01(dropout=0.0, version='1A')
            dn.load_state_dict(sd)
            self.model.add_depth_net(dn)
            self.model.add_pose_net(PoseNet(nb_ref_imgs=2))
            self.config = types.SimpleNamespace(datasets=types.SimpleNamespace(test=types.SimpleNamespace(batch_size=2)))
            self.metrics_cfg = types.SimpleNamespace(min_depth=0.0, max_depth=80.0, crop='', scale_output='resize')
            self.result = None

        def test_dataloader(self):
            return [Loader(batches)]

        def test_step(self, batch, i, n):
            inv = self.model({'rgb': batch['rgb']})['inv_depths']
            return {'dtype': inv.dtype, 'metrics': compute_depth_metrics(self.metrics_cfg, batch['depth'], inv2depth(inv))}

        def test_epoch_end(self, outputs):
            self.result = outputs[0]
            return {}

    res = {}
    for dt in (torch.float32, torch.float16):
        w = Wrapper()
        HorovodTrainer(max_epochs=1, dtype=dt).test(w)
        assert all(p.dtype == dt for p in w.parameters())
        assert all(o['dtype'] == dt for o in w.result)
        res[dt] = torch.stack([o['metrics'].double().cpu() for o in w.result])
    assert torch.isfinite(res[torch.float16]).all()
    assert torch.allclose(res[torch.float16], res[torch.float32], rtol=1e-2, atol=2e-3), (res[torch.float16], res[torch.float32])
