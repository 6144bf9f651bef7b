"""CPU: the depth-output kernels (csrc/depth_output.h) compiled for the host and run on the emulator, through the same wrappers and
against the same expectations as on the GPU (tests/depth_output_cases.py), plus the CPU-tensor paths of packnet_sfm.utils.depth."""
import numpy as np
import pytest
import torch

import depth_output_cases as C

CPU = torch.device('cpu')


@pytest.mark.parametrize('key', C.SUB_KEYS)
def test_viz_inv_depth_emulated(emulated_kernels, key):
    C.viz_case(CPU, key)


def test_viz_all_zero_image_emulated(emulated_kernels):
    C.all_zero_case(CPU)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_viz_panel_emulated(emulated_kernels, dtype):
    C.panel_case(CPU, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_depth_png16_emulated(emulated_kernels, dtype):
    C.png16_case(CPU, dtype)


def test_public_functions_emulated(emulated_kernels):
    C.public_case(CPU)


def test_depth_output_errors_emulated(emulated_kernels):
    C.errors_case(CPU)


# ---- no emulator: the inputs, the fixture and the CPU-tensor paths of packnet_sfm.utils.depth
def test_case_2_covers_both_interpolation_branches():
    gammas = []
    for sub in C.SUBS:
        if sub.case == 2:
            v = C.virtual_index(C.viz_input(sub.input)[0].numel(), sub.percentile)
            gammas.append(float(v - np.floor(v)))
    assert any(0 < g < 0.5 for g in gammas) and any(g >= 0.5 for g in gammas) and any(g == 0 for g in gammas), gammas
    ties = C.viz_input('ties')
    assert ties.unique().numel() <= 33                                  # case 3: long runs of ties
    zeros = C.viz_input('zeros')
    assert 0.25 < float((zeros == 0).float().mean()) < 0.35             # case 4: about 30 % zeros


@pytest.mark.parametrize('key', C.SUB_KEYS)
def test_viz_cpu_tensor_path(key):
    """CPU tensors, product loader: the numpy formula of packnet_sfm.utils.depth against the reference's recorded indices."""
    from packnet_sfm.hip import _lib
    from packnet_sfm.utils import depth as D
    assert _lib.REQUIRE_CUDA
    sub, fx = C.BY_KEY[key], C.fixture()
    inv, tab = C.viz_input(sub.input), C.table(sub.table)
    out, index, norms = D.viz_inv_depth_u8(inv, normalizer=sub.normalizer, percentile=sub.percentile, colormap=tab,
                                           filter_zeros=sub.filter_zeros, details=True)
    assert torch.equal(index, fx['index'][key])
    assert torch.equal(out, C.lut8_of(tab)[index.long()])
    assert np.array_equal(C.bits(norms.numpy()), C.bits(C.host_normalizers(sub, inv)))


def test_cpu_tensor_path_panel_all_zero_and_errors():
    from packnet_sfm.utils import depth as D
    u8, inv = C.panel_inputs()
    rgb = u8.permute(0, 3, 1, 2).float() / 255
    tab = C.table('plasma')
    for bgr in (False, True):
        out = D.viz_inv_depth_u8(inv, rgb=rgb, colormap=tab, bgr=bgr)
        assert torch.equal(out[:, :8], u8.flip(3) if bgr else u8)
        assert torch.equal(out[:, 8:], D.viz_inv_depth_u8(inv, colormap=tab, bgr=bgr))
    out, index, norms = D.viz_inv_depth_u8(torch.zeros((1, 1, 3, 7)), colormap=tab, filter_zeros=True, details=True)
    assert float(norms[0]) == 0.0 and not bool(index.any())
    with pytest.raises(ValueError):
        D.viz_inv_depth_u8(inv, colormap=tab, percentile=101)
    with pytest.raises(ValueError):
        D.viz_inv_depth_u8(inv, rgb=rgb[:, :, :4], colormap=tab)
    with pytest.raises(ValueError):
        D.viz_inv_depth_u8(inv, colormap=np.zeros((257, 3)))


def test_plasma_resolves_to_the_fixture_table():
    from packnet_sfm.utils import depth as D
    import matplotlib
    fx = C.fixture()
    cmap = matplotlib.colormaps['plasma']
    assert np.array_equal(cmap(np.arange(cmap.N))[:, :3], fx['plasma'].numpy())
    lut8 = D.colormap_lut8('plasma', 'cpu')
    assert torch.equal(lut8, C.lut8_of(fx['plasma'].numpy())) and D.colormap_lut8('plasma', 'cpu') is lut8      # cached per (name, device)
    inv = C.viz_input('zeros')
    assert torch.equal(D.viz_inv_depth_u8(inv), D.viz_inv_depth_u8(inv, colormap=fx['plasma']))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_depth_png16_cpu_tensor_path_and_png_round_trip(tmp_path, dtype):
    """CPU only: the uint16 values survive a 16-bit PNG (what write_depth's .png branch produces) unchanged."""
    from PIL import Image
    from packnet_sfm.utils import depth as D
    out = C.png16_case(CPU, dtype, D.depth_png16)
    arr = out[0, 0].numpy()
    path = str(tmp_path / 'depth.png')
    Image.fromarray(arr).save(path)
    back = np.array(Image.open(path))
    assert back.dtype == np.uint16 or int(back.max()) == 65535
    assert np.array_equal(back.astype(np.int64), arr.astype(np.int64))


def test_names_resolve_without_a_reference_checkout():
    from packnet_sfm.utils import depth as D
    for name in ('viz_inv_depth_u8', 'depth_png16', 'colormap_lut8'):
        assert name in vars(D), name
    for name in ('viz_inv_depth', 'write_depth'):          # those stay the reference's (tests/test_package_merge.py)
        assert name not in vars(D), name
