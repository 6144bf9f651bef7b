"""GPU (MI355X): the tuning-key query and tune.pinned on the device, one launch per key rule (tests/tune_cases.py; the host
emulator runs the same table in tests/test_kernels_emulated.py).  Every shape is a few thousand pixels: milliseconds per launch."""
import pytest
import torch

import tune_cases as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_tune_key_reproduces_database_lines_gpu():
    TC.check_key_reproduces_database_lines()


@pytest.mark.parametrize('case', TC.LAUNCH_CASES, ids=TC.LAUNCH_IDS)
def test_tune_launch_case(case):
    """Tolerances: 2e-5 forward / backward-data (tests/test_gpu_round6.py), 5e-5 weight gradients (the pinned weight gradients of
    tests/test_gpu_round6.py and tests/test_gpu_conv_nodes.py)."""
    TC.run_launch_case(DEV, case, 2e-5, 5e-5)
