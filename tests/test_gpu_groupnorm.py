"""GPU (MI355X): the kernels of csrc/groupnorm.hip per element against the float64 oracle, at the cases, routes, masks and tolerances
of tests/groupnorm_cases.py.

The host emulator runs the same table (tests/test_groupnorm_emulated.py); what only the device can show is checked here: its
exponential in gn_expm1_neg and act_grad (the exact-z cases are the measurement of the 1e-7 derived for it), FMA contraction, the
wave and LDS reductions on real workgroups, the parts of a slab on different compute units (S = 4, with and without the XCD
interleave), and the three shapes the emulator leaves out: the largest one-launch slab and 64 chunks per row, vector and scalar,
where the two-launch workspace is used to its last slot."""
import pytest
import torch

import groupnorm_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


@pytest.mark.parametrize('case', C.CASES, ids=C.ids(C.CASES))
def test_groupnorm_elements(case):
    C.run_case(DEV, case)


@pytest.mark.parametrize('case', C.FUNCTIONAL_CASES, ids=C.ids(C.FUNCTIONAL_CASES))
def test_groupnorm_functional_residual(case):
    C.run_functional(DEV, case)


@pytest.mark.parametrize('case', C.H16_CASES, ids=C.ids(C.H16_CASES))
def test_groupnorm_h16_edges(case):
    C.run_h16(DEV, case)
