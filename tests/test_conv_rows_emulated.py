"""CPU (host-emulated kernels): the row-window convolution of the collapsed packing block's border strips -- the cases of
tests/conv_rows_cases.py at the emulator's tolerance (1e-5, as tests/test_kernels_emulated.py)."""
import pytest

import conv_rows_cases as C

TOL = 1e-5


@pytest.mark.parametrize('shape', C.SHAPES, ids=lambda s: 'r%d-B%d-Cin%d-w%d' % s)
def test_rows_vs_reference(emulated_kernels, shape):
    C.shape_case('cpu', shape, TOL, TOL)


@pytest.mark.parametrize('case', C.BX3_VARIANTS, ids=lambda c: 'r%d-B%d-Cin%d-w%d' % c[0] + '-v%d-NT%d-m%d-tm%d-split%d' % c[1] + ('-' + c[2] if len(c) > 2 else ''))
def test_rows_split_bf16_variants(emulated_kernels, case):
    C.bx3_variant_case('cpu', case, TOL)


@pytest.mark.parametrize('case', C.F32_VARIANTS, ids=lambda c: 'r%d-B%d-Cin%d-w%d' % c[0] + '-v%d-NT%d-split%d' % c[1])
def test_rows_f32_variants(emulated_kernels, case):
    C.f32_variant_case('cpu', case, TOL)


@pytest.mark.parametrize('case', C.WGRAD_KERNEL_CASES, ids=lambda c: 'r%d-B%d-Cin%d-w%d' % c[0] + '-' + '.'.join(map(str, c[3])) + '-s%d' % c[2]['split'])
def test_rows_weight_gradient_kernels(emulated_kernels, case):
    C.wgrad_kernel_case('cpu', case, TOL)


def test_rows_refused_by_the_1x1_and_stem_kernels(emulated_kernels):
    C.refusal_case('cpu')


@pytest.mark.parametrize('k,hw', C.BLOCK_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_pack_block_frame_rows_vs_full_strips(emulated_kernels, k, hw):
    C.block_case('cpu', k, hw, TOL, 5e-5)
