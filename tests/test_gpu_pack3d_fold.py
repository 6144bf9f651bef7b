"""GPU (MI355X): the folded launch sequences of the packing / unpacking blocks against the unfolded sequences of the same build
(pnsfm_set_pack3d_fold(0)) -- torch.equal, through the C ABI into NaN-guarded slots, a bit-identical second launch of every gradient.

The table and the runners are tests/pack3d_fold_cases.py, which the host emulator runs too (tests/test_pack3d_fold_emulated.py).
What only the device can show: that the compiler kept the fmaf order of conv3d_fwd_x4_kernel in the two-plane build, float4 stores
at the depth-to-space address at grids of 1 / 8 / 13 / 25 blocks, a row window's out-of-range offsets in the buffer loads of the
gradient kernels next to their wave shifts, and the same contraction of the bias tail's multiply-adds.
The unfolded sequences are pinned against float64 by tests/test_gpu_pack3d.py."""
import pytest
import torch

import pack3d_fold_cases as FC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_pack3d_fold_table():
    FC.check_table()


@pytest.mark.parametrize('case', FC.FWD_CASES, ids=FC.ids(FC.FWD_CASES))
def test_pack3d_fold_forward(case):
    FC.run_forward(DEV, case)


@pytest.mark.parametrize('case', FC.ROWS_CASES, ids=FC.ids(FC.ROWS_CASES))
def test_pack3d_fold_strip_rows(monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    FC.run_rows(DEV, case)


@pytest.mark.parametrize('case', FC.BIAS_CASES, ids=FC.ids(FC.BIAS_CASES))
def test_pack3d_fold_bias(case):
    FC.run_bias(DEV, case)


@pytest.mark.parametrize('name', FC.BLOCK_CASES)
def test_pack3d_fold_blocks(name):
    FC.run_block(DEV, name)
