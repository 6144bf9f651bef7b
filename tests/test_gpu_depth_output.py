"""GPU: the depth-output kernels (csrc/depth_output.h) on the MI355X -- the cases of tests/depth_output_cases.py, plus inference-size
maps against the CPU-tensor path, run-to-run reproducibility and the absence of host synchronisation."""
import pytest
import torch

import depth_output_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('key', C.SUB_KEYS)
def test_viz_inv_depth(key):
    C.viz_case(_dev(), key)


def test_viz_all_zero_image():
    C.all_zero_case(_dev())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_viz_panel(dtype):
    C.panel_case(_dev(), dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_depth_png16(dtype):
    C.png16_case(_dev(), dtype)


def test_public_functions():
    C.public_case(_dev())


def test_depth_output_errors():
    C.errors_case(_dev())


@pytest.mark.parametrize('shape', [(4, 192, 640), (1, 384, 1280)])
def test_viz_inference_sizes_against_the_cpu_tensor_path(shape):
    """Inference-size batches (128 workgroups per image, grid-stride loops) against the numpy formula, twice: two runs are equal."""
    from packnet_sfm.utils import depth as D
    B, H, W = shape
    inv = torch.cat([C._map((1, 1, H, W), 140 + b, 0.02, 0.3 + 0.4 * b) for b in range(B)])
    inv[0, 0, :7, :11] = 0
    u8 = (C.uniform((B, H, W, 3), 150) * 256).to(torch.uint8)
    rgb = (u8.permute(0, 3, 1, 2).float() / 255).contiguous()
    tab = C.table('plasma')
    for kw in (dict(), dict(filter_zeros=True, percentile=99.5), dict(rgb=rgb, bgr=True)):
        want = C.host_path(D.viz_inv_depth_u8, inv, colormap=tab, details=True, **kw)
        dkw = dict(kw, rgb=rgb.to(_dev())) if 'rgb' in kw else kw
        got = D.viz_inv_depth_u8(inv.to(_dev()), colormap=tab, details=True, **dkw)
        again = D.viz_inv_depth_u8(inv.to(_dev()), colormap=tab, details=True, **dkw)
        assert C.same(got, want), kw.keys()
        assert C.same(got, again)
    d16 = D.depth_png16(inv.to(_dev()))
    assert torch.equal(d16.cpu().to(torch.int32), C.png16_expected(inv)) and torch.equal(d16, D.depth_png16(inv.to(_dev())))


def test_viz_does_not_sync():
    """Case 5 under torch's sync debug mode: any device->host copy or synchronisation inside the calls raises."""
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.utils import depth as D
    inv = C.viz_input('batch').to(_dev())
    tab = C.table('plasma')
    lut8 = D.colormap_lut8(tab, _dev())
    want = HF.viz_inv_depth_u8(inv, lut8, details=True)          # library load, first-use work
    D.viz_inv_depth_u8(inv, colormap='plasma')                   # fills the per-(name, device) table cache
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = HF.viz_inv_depth_u8(inv, lut8, details=True)
        named = D.viz_inv_depth_u8(inv, colormap='plasma')
        d16 = HF.depth_png16(inv)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert C.same(got, want) and torch.equal(named, want[0]) and int(d16.to(torch.int32).max()) > 0
    assert torch.equal(got[1].cpu(), C.fixture()['index']['c5'])
