"""GPU (MI355X): the kernels of csrc/pack3d.hip at kernel level, at the shapes where their lane, chunk and row arithmetic has edges.

The table is tests/pack3d_cases.py, which the host emulator runs too (tests/test_kernels_emulated.py, tests/test_half_emulated.py).
The emulator runs one fiber at a time and restates the wave shifts, the buffer range check and 16-byte alignment in C++; what only
the device can show is checked here: a shift executed under divergence, zero padding that comes from the hardware range check of a
buffer load, a misaligned float4, the XCD renumbering at a grid that is no multiple of 8, weights held in SGPRs and packed FMAs.

Every launch goes through the C ABI into NaN-guarded slots and is compared per element with a float64 reference at derived bounds
(the shuffles: bit-exact); the gradient launches are repeated and must be bit-identical.  There is no read-back of the kernel a
launch chose: pack3d_cases.check_table() restates the launchers' conditions on each case's shape and pointer alignment instead.
The tests run the product's defaults of PNSFM_CONV3D_DGRAD_COL, PNSFM_STENCIL_XCD_MAP and PNSFM_BLOCK_MAP (read once per process)."""
import pytest
import torch

import pack3d_cases as PC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_pack3d_table():
    PC.check_table()


def test_pack3d_error_returns():
    PC.run_rejects(DEV)


@pytest.mark.parametrize('case', PC.FWD_CASES, ids=PC.ids(PC.FWD_CASES))
def test_pack3d_forward(case):
    PC.run_forward(DEV, case)


@pytest.mark.parametrize('case', PC.FWD16_CASES, ids=PC.ids(PC.FWD16_CASES))
def test_pack3d_forward_h16(case):
    PC.run_forward16(DEV, case)


@pytest.mark.parametrize('case', PC.DGRAD_CASES, ids=PC.ids(PC.DGRAD_CASES))
def test_pack3d_dgrad(monkeypatch, case):
    if case['run'] is None:
        monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    else:
        monkeypatch.setenv('PNSFM_CONV3D_LEN', str(case['run']))
    PC.run_dgrad(DEV, case)


@pytest.mark.parametrize('case', PC.WGRAD_CASES, ids=PC.ids(PC.WGRAD_CASES))
def test_pack3d_wgrad(monkeypatch, case):
    monkeypatch.setenv('PNSFM_CONV3D_WGRAD_RING', case['variant'])
    PC.run_wgrad(DEV, case)


@pytest.mark.parametrize('case', PC.SHUFFLE_CASES, ids=PC.ids(PC.SHUFFLE_CASES))
def test_pack3d_shuffle(case):
    PC.run_shuffle(DEV, case)
