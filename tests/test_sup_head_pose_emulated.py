"""CPU: the kernels of csrc/supervised.hip and csrc/invdepth.hip and the invdepth_act / pose_vec2mat kernels of csrc/elementwise.hip
compiled for the host and run on the emulator, per element against the float64 oracle, at the cases, masks and tolerances of
tests/sup_head_pose_cases.py (which tests/test_gpu_sup_head_pose.py runs on the device)."""
import pytest

import sup_head_pose_cases as C

CPU = 'cpu'


def test_sup_head_pose_case_tables():
    """From the oracle alone: every supervised case meets the cap on its excluded share and is the edge case its name says; the
    copy of the launcher's rule gives the automatic head cases 2 and 16 pixel slices per thread and the forced ones 1."""
    for c in C.SUP_CASES:
        C.check_sup_case(c)
    for c in C.IDC_BWD_AUTO_CASES:
        assert C.bwd_ppt(*c['shape']) == c['expect']
    for c in C.IDC_BWD_CASES:
        assert C.bwd_ppt(*c['shape']) == 1


@pytest.mark.parametrize('case', C.SUP_CASES_EMU, ids=C.ids(C.SUP_CASES_EMU))
def test_supervised_loss_pixels_emulated(emulated_kernels, case):
    C.run_sup(CPU, case)


@pytest.mark.parametrize('case', C.IDC_BWD_CASES, ids=C.ids(C.IDC_BWD_CASES))
def test_invdepth_conv_backward_pixels_emulated(emulated_kernels, monkeypatch, case):
    C.run_idc_bwd(CPU, case, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('case', C.IDC_FWD_CASES, ids=C.ids(C.IDC_FWD_CASES))
def test_invdepth_conv_forward_pixels_emulated(emulated_kernels, monkeypatch, case):
    C.run_idc_fwd(CPU, case, monkeypatch.setenv)


@pytest.mark.parametrize('case', C.ACT_CASES, ids=C.ids(C.ACT_CASES))
def test_invdepth_act_pixels_emulated(emulated_kernels, case):
    C.run_act(CPU, case)


@pytest.mark.parametrize('case', C.POSE_CASES, ids=C.ids(C.POSE_CASES))
def test_pose_vec2mat_entries_emulated(emulated_kernels, case):
    C.run_pose(CPU, case)
