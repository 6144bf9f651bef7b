"""GPU (MI355X): the row-window convolution of the collapsed packing block's border strips -- the cases of tests/conv_rows_cases.py
on the gfx950 kernels, at the project's bounds for these kernels (2e-5 forward and backward-data, 5e-5 weight gradient: the P.check
bounds of tests/test_gpu_parity.py / test_gpu_round6.py)."""
import pytest
import torch

import conv_rows_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL, TOL_W = 2e-5, 5e-5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


@pytest.mark.parametrize('shape', C.SHAPES, ids=lambda s: 'r%d-B%d-Cin%d-w%d' % s)
def test_rows_vs_reference(shape):
    C.shape_case(DEV, shape, TOL, TOL_W)


@pytest.mark.parametrize('case', C.BX3_VARIANTS, ids=lambda c: 'r%d-B%d-Cin%d-w%d' % c[0] + '-v%d-NT%d-m%d-tm%d-split%d' % c[1] + ('-' + c[2] if len(c) > 2 else ''))
def test_rows_split_bf16_variants(case):
    C.bx3_variant_case(DEV, case, TOL)


@pytest.mark.parametrize('case', C.F32_VARIANTS, ids=lambda c: 'r%d-B%d-Cin%d-w%d' % c[0] + '-v%d-NT%d-split%d' % c[1])
def test_rows_f32_variants(case):
    C.f32_variant_case(DEV, case, TOL)


@pytest.mark.parametrize('case', C.WGRAD_KERNEL_CASES, ids=lambda c: 'r%d-B%d-Cin%d-w%d' % c[0] + '-' + '.'.join(map(str, c[3])) + '-s%d' % c[2]['split'])
def test_rows_weight_gradient_kernels(case):
    C.wgrad_kernel_case(DEV, case, TOL_W)


def test_rows_refused_by_the_1x1_and_stem_kernels():
    C.refusal_case(DEV)


@pytest.mark.parametrize('k,hw', C.BLOCK_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_pack_block_frame_rows_vs_full_strips(k, hw):
    C.block_case(DEV, k, hw, TOL, TOL_W)


@pytest.mark.parametrize('k,hw', [(3, (12, 40)), (5, (12, 40)), (3, (8, 24))], ids=lambda v: str(v).replace(' ', ''))
def test_pack_block_frame_rows_bit_equal_to_full_strips(k, hw):
    C.block_bits_case(DEV, k, hw)
