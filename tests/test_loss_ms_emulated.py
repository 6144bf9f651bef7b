"""CPU: the all-scales entry points of csrc/loss.hip compiled for the host and run on the emulator, bit for bit against the per-scale
path, at the cases of tests/loss_ms_cases.py (which tests/test_gpu_loss_ms.py runs on the device)."""
import pytest

import loss_ms_cases as C

CPU = 'cpu'


def test_loss_ms_rejects_emulated(emulated_kernels):
    C.run_rejects(CPU)


@pytest.mark.parametrize('case', C.NODE_CASES, ids=C.ids(C.NODE_CASES))
def test_loss_ms_node_equals_per_scale_emulated(emulated_kernels, case):
    C.run_node(CPU, case)


@pytest.mark.parametrize('case', C.THIN_CASES, ids=C.ids(C.THIN_CASES))
def test_loss_ms_block_edge_emulated(emulated_kernels, case):
    C.run_thin(CPU, case)


@pytest.mark.parametrize('case', C.ID_CASES, ids=C.ids(C.ID_CASES))
def test_loss_ms_identity_map_emulated(emulated_kernels, case):
    C.run_identity(CPU, case)


def test_loss_ms_smoothness_mixed_resolutions_emulated(emulated_kernels):
    C.run_smoothness_mixed(CPU)


def test_loss_ms_fallback_emulated(emulated_kernels):
    C.run_fallback(CPU)
