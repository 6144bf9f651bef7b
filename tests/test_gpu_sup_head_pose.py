"""GPU (MI355X): the kernels of csrc/supervised.hip and csrc/invdepth.hip and the invdepth_act / pose_vec2mat kernels of
csrc/elementwise.hip per element against the float64 oracle, at the cases, masks and tolerances of tests/sup_head_pose_cases.py.

The host emulator runs the same table (tests/test_sup_head_pose_emulated.py); what only the device can show is checked here: its
expf, logf, sinf, cosf and division, FMA contraction, the wave reductions and double atomics of the supervised reduction on 1024
real workgroups, the buffer range check that is the zero padding of the head's backward, and the head's backward at the two shapes
where the launcher's own rule walks 2 and 16 pixel slices per thread (too slow for the emulator)."""
import pytest
import torch

import sup_head_pose_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


@pytest.mark.parametrize('case', C.SUP_CASES, ids=C.ids(C.SUP_CASES))
def test_supervised_loss_pixels(case):
    C.run_sup(DEV, case)


@pytest.mark.parametrize('case', C.IDC_BWD_CASES + C.IDC_BWD_AUTO_CASES, ids=C.ids(C.IDC_BWD_CASES + C.IDC_BWD_AUTO_CASES))
def test_invdepth_conv_backward_pixels(monkeypatch, case):
    C.run_idc_bwd(DEV, case, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('case', C.IDC_FWD_CASES, ids=C.ids(C.IDC_FWD_CASES))
def test_invdepth_conv_forward_pixels(monkeypatch, case):
    C.run_idc_fwd(DEV, case, monkeypatch.setenv)


@pytest.mark.parametrize('case', C.ACT_CASES, ids=C.ids(C.ACT_CASES))
def test_invdepth_act_pixels(case):
    C.run_act(DEV, case)


@pytest.mark.parametrize('case', C.POSE_CASES, ids=C.ids(C.POSE_CASES))
def test_pose_vec2mat_entries(case):
    C.run_pose(DEV, case)
