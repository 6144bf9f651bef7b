"""CPU: the folded launch sequences of the packing / unpacking blocks on the host-emulated build of the kernel sources, against the
unfolded sequences of the same build (pnsfm_set_pack3d_fold(0)) -- torch.equal, through the C ABI into NaN-guarded slots.  The table
and the runners are tests/pack3d_fold_cases.py; tests/test_gpu_pack3d_fold.py runs the same cases on the gfx950 build.  The emulator
restates the wave shifts and the buffer range check in C++, so what it checks is the index arithmetic of the folds: the
depth-to-space address of every store, the row window of the border strips in the forward and both gradient kernels, the (d, C)
grid of the bias sums."""
import pytest

import pack3d_fold_cases as FC


def test_pack3d_fold_table_is_sound():
    FC.check_table()


@pytest.mark.parametrize('case', FC.FWD_CASES, ids=FC.ids(FC.FWD_CASES))
def test_conv3d_forward_d2s(emulated_kernels, case):
    FC.run_forward('cpu', case)


@pytest.mark.parametrize('case', FC.ROWS_CASES, ids=FC.ids(FC.ROWS_CASES))
def test_conv3d_strip_rows(emulated_kernels, monkeypatch, case):
    monkeypatch.delenv('PNSFM_CONV3D_LEN', raising=False)
    monkeypatch.delenv('PNSFM_CONV3D_WGRAD_RING', raising=False)
    FC.run_rows('cpu', case)


@pytest.mark.parametrize('case', FC.BIAS_CASES, ids=FC.ids(FC.BIAS_CASES))
def test_pack_bias_eff_grid(emulated_kernels, case):
    FC.run_bias('cpu', case)


def test_unpack_block_both_switch_settings(emulated_kernels):
    """UnpackLayerConv3d forward and backward (the autograd node over the folded forward) under both switch settings.  The
    packing blocks run on the device only (too slow to emulate)."""
    FC.run_block('cpu', 'unpack-k3')
