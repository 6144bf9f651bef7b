"""GPU (MI355X): the kernels of csrc/loss.hip per element against the float64 oracle, at the cases, masks and tolerances of
tests/loss_cases.py.

The host emulator runs the same table (tests/test_loss_emulated.py) and agrees with the oracle; what only the device can show is
checked here: FMA contraction in the projection, the device's division, fmodf and expf, the LDS tiles and their halos across
16-pixel seams, the XCD tile renumbering at block counts that are no multiple of 8, and the four-wave pose-gradient reduction with
waves that hold no pixel."""
import pytest
import torch

import loss_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_loss_error_returns():
    C.run_rejects(DEV)


@pytest.mark.parametrize('case', C.VS_CASES, ids=C.ids(C.VS_CASES))
def test_view_synthesis_pixels(case):
    C.run_vs(DEV, case)


@pytest.mark.parametrize('case', C.PH_CASES, ids=C.ids(C.PH_CASES))
def test_photometric_pixels(case):
    C.run_ph(DEV, case)


@pytest.mark.parametrize('case', C.L1_CASES, ids=C.ids(C.L1_CASES))
def test_photometric_l1_pixels(case):
    C.run_l1(DEV, case)


@pytest.mark.parametrize('case', C.SM_CASES, ids=C.ids(C.SM_CASES))
def test_smoothness_pixels(case):
    C.run_sm(DEV, case)
