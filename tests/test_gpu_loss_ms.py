"""GPU (MI355X): the all-scales entry points of csrc/loss.hip bit for bit against the per-scale path, at the cases of
tests/loss_ms_cases.py.

The host emulator runs the same table (tests/test_loss_ms_emulated.py); what only the device can show is checked here: that the
smoothness term is ADDED to the photometric gradient as one rounded sum (no FMA into the product), the XCD tile renumbering over a
grid that holds several scales, and the order in which the autograd engine's device thread sums the per-scale pose gradients."""
import pytest
import torch

import loss_ms_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA and _lib.get().pnsfm_version() >= 10


def test_loss_ms_rejects():
    C.run_rejects(DEV)


@pytest.mark.parametrize('case', C.NODE_CASES, ids=C.ids(C.NODE_CASES))
def test_loss_ms_node_equals_per_scale(case):
    C.run_node(DEV, case)


@pytest.mark.parametrize('case', C.THIN_CASES, ids=C.ids(C.THIN_CASES))
def test_loss_ms_block_edge(case):
    C.run_thin(DEV, case)


@pytest.mark.parametrize('case', C.ID_CASES, ids=C.ids(C.ID_CASES))
def test_loss_ms_identity_map(case):
    C.run_identity(DEV, case)


def test_loss_ms_smoothness_mixed_resolutions():
    C.run_smoothness_mixed(DEV)


def test_loss_ms_fallback():
    C.run_fallback(DEV)
