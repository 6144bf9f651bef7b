"""CPU: the kernels of csrc/loss.hip compiled for the host and run on the emulator, per element against the float64 oracle, at the
cases, masks and tolerances of tests/loss_cases.py (which tests/test_gpu_loss.py runs on the device)."""
import pytest

import loss_cases as C

CPU = 'cpu'


def test_loss_case_tables():
    """From the oracle alone: every case meets the cap on its excluded share and has the off-frame, reflection, behind-camera and
    clamp shares that make it an edge case."""
    for c in C.VS_CASES:
        C.check_vs_case(c)
    for c in C.PH_CASES:
        C.check_ph_case(c)
    for c in C.L1_CASES:
        C.check_l1_case(c)
    C.check_sm_table()


def test_loss_error_returns_emulated(emulated_kernels):
    C.run_rejects(CPU)


@pytest.mark.parametrize('case', C.VS_CASES, ids=C.ids(C.VS_CASES))
def test_view_synthesis_pixels_emulated(emulated_kernels, case):
    C.run_vs(CPU, case)


@pytest.mark.parametrize('case', C.PH_CASES, ids=C.ids(C.PH_CASES))
def test_photometric_pixels_emulated(emulated_kernels, case):
    C.run_ph(CPU, case)


@pytest.mark.parametrize('case', C.L1_CASES, ids=C.ids(C.L1_CASES))
def test_photometric_l1_pixels_emulated(emulated_kernels, case):
    C.run_l1(CPU, case)


@pytest.mark.parametrize('case', C.SM_CASES, ids=C.ids(C.SM_CASES))
def test_smoothness_pixels_emulated(emulated_kernels, case):
    C.run_sm(CPU, case)
