"""CPU: the collapsed packing block's weight path without ATen copies and adds, on the host-emulated build of the kernel sources --
torch.equal against the former path of the same build.  The table and the runners are tests/pack_wpath_cases.py;
tests/test_gpu_pack_wpath.py runs the same cases on the gfx950 build.  What the emulator checks is the index arithmetic: the packers'
source tap, the stencil kernels' tap map and column window, the epilogue's destination tap and its add.  The whole blocks run on the
device only (too slow to emulate)."""
import pytest

import pack_wpath_cases as WC


def test_pack_wpath_table_is_sound():
    WC.check_table()


@pytest.mark.parametrize('case', WC.PACK_CASES, ids=WC.ids(WC.PACK_CASES))
def test_packer_tap_transpose(emulated_kernels, case):
    WC.run_packer('cpu', case)


@pytest.mark.parametrize('case', WC.C3D_CASES, ids=WC.ids(WC.C3D_CASES))
def test_conv3d_tap_transpose(emulated_kernels, monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_conv3d('cpu', case)


@pytest.mark.parametrize('case', WC.RING_CASES, ids=WC.ids(WC.RING_CASES))
def test_implicit_ring(emulated_kernels, monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    if case['len'] is None:
        monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    else:
        monkeypatch.setenv('PNSFM_CONV3D_LEN', str(case['len']))
    WC.run_ring('cpu', case)


@pytest.mark.parametrize('case', WC.COMPOSE_CASES[:1], ids=WC.ids(WC.COMPOSE_CASES[:1]))
def test_composition_node(emulated_kernels, monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_compose('cpu', case)


@pytest.mark.parametrize('case', WC.ADD2_CASES, ids=WC.ids(WC.ADD2_CASES))
def test_add_into_conv2d_weight_gradient(emulated_kernels, case):
    WC.run_add2('cpu', case)


@pytest.mark.parametrize('case', WC.ADD3_CASES, ids=WC.ids(WC.ADD3_CASES))
def test_add_into_conv3d_weight_gradient(emulated_kernels, monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    WC.run_add3('cpu', case)


@pytest.mark.parametrize('case', WC.ADDB_CASES, ids=WC.ids(WC.ADDB_CASES))
def test_add_into_composed_bias(emulated_kernels, case):
    WC.run_addb('cpu', case)
