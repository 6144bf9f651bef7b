"""CPU: the kernels of csrc/groupnorm.hip compiled for the host and run on the emulator, per element against the float64 oracle, at
the cases, routes, masks and tolerances of tests/groupnorm_cases.py (which tests/test_gpu_groupnorm.py runs on the device).  Seven
shapes of that table (groupnorm_cases.GPU_ONLY) run on the device only: 64 chunks per row, (1,16,512,1024) and (1,16,359,361), take
50 s each here, and twelve or sixteen slabs of 1024-thread workgroups take 5-10 s: (1,16,128,512), (1,16,4,16385), (1,112,4,439),
(1,80,24,160), (3,16,64,64)."""
import pytest

import groupnorm_cases as C

CPU = 'cpu'


def test_groupnorm_case_tables():
    """From the restated launch rules alone: every case, the device-only ones included, takes the route its table entry names (each
    case checks its own cap on the excluded share before it compares anything: groupnorm_cases.check_case)."""
    for c in C.CASES + C.FUNCTIONAL_CASES + C.H16_CASES:
        C.check_route(c)
    assert {c['shape'] for c in C.CASES} - {c['shape'] for c in C.CASES_EMU} == C.GPU_ONLY
    assert all(C.tol(cls, q) >= C.FLOOR for cls in C.GN_BASE for q in C.GN_BASE[cls])


@pytest.mark.parametrize('case', C.CASES_EMU, ids=C.ids(C.CASES_EMU))
def test_groupnorm_elements_emulated(emulated_kernels, case):
    C.run_case(CPU, case)


@pytest.mark.parametrize('case', C.FUNCTIONAL_CASES, ids=C.ids(C.FUNCTIONAL_CASES))
def test_groupnorm_functional_residual_emulated(emulated_kernels, case):
    C.run_functional(CPU, case)


@pytest.mark.parametrize('case', C.H16_CASES, ids=C.ids(C.H16_CASES))
def test_groupnorm_h16_edges_emulated(emulated_kernels, case):
    C.run_h16(CPU, case)
