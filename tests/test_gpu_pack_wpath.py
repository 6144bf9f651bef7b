"""GPU (MI355X): the collapsed packing block's weight path without ATen copies and adds against the former path of the same build --
torch.equal, nothing here may change a rounding.  The table and the runners are tests/pack_wpath_cases.py, which the host emulator
runs too (tests/test_pack_wpath_emulated.py).  What only the device can show: the column window's out-of-range offsets in the buffer
loads of the stencil gradients next to their wave shifts, that the compiler kept the multiply-add of the composed bias's gradient
under the added term, the epilogue's add against ATen's on the same values, and the whole block -- the gradient owner, its stream
order between the side stream and the compute stream, and what AccumulateGrad does with the tensors it is handed."""
import pytest
import torch

import pack_wpath_cases as WC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_pack_wpath_table():
    WC.check_table()


@pytest.mark.parametrize('case', WC.PACK_CASES, ids=WC.ids(WC.PACK_CASES))
def test_pack_wpath_packer(case):
    WC.run_packer(DEV, case)


@pytest.mark.parametrize('case', WC.C3D_CASES, ids=WC.ids(WC.C3D_CASES))
def test_pack_wpath_conv3d(monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_conv3d(DEV, case)


@pytest.mark.parametrize('case', WC.RING_CASES, ids=WC.ids(WC.RING_CASES))
def test_pack_wpath_ring(monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    if case['len'] is None:
        monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    else:
        monkeypatch.setenv('PNSFM_CONV3D_LEN', str(case['len']))
    WC.run_ring(DEV, case)


@pytest.mark.parametrize('case', WC.COMPOSE_CASES, ids=WC.ids(WC.COMPOSE_CASES))
def test_pack_wpath_composition_node(monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_compose(DEV, case)


@pytest.mark.parametrize('case', WC.ADD2_CASES, ids=WC.ids(WC.ADD2_CASES))
def test_pack_wpath_add_conv2d(case):
    WC.run_add2(DEV, case)


@pytest.mark.parametrize('case', WC.ADD3_CASES, ids=WC.ids(WC.ADD3_CASES))
def test_pack_wpath_add_conv3d(monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_add3(DEV, case)


@pytest.mark.parametrize('case', WC.ADDB_CASES, ids=WC.ids(WC.ADDB_CASES))
def test_pack_wpath_add_bias(case):
    WC.run_addb(DEV, case)


@pytest.mark.parametrize('case', WC.BLOCK_CASES, ids=WC.ids(WC.BLOCK_CASES))
def test_pack_wpath_blocks(monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_block(DEV, case)
