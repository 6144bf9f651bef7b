"""CPU: the fp16 forward kernels (include/pnsfm.h "fp16 forward") on the host-emulated build, against float64 on the same fp16 values
(tests/half_cases.py)."""
import pytest

import half_cases as HC
import pack3d_cases as PC


@pytest.mark.parametrize('ks', [1, 3, 5, 7])
@pytest.mark.parametrize('ksplit', [1, None])
def test_conv_h16_kernel_sizes(emulated_kernels, ks, ksplit):
    cfg = HC.conv_case('cpu', 1, [20], 40, 5, 11, ks, seed=ks, ksplit=ksplit)
    assert (cfg[4] == 1) if ksplit == 1 else (cfg[4] > 1)


def test_conv_h16_stem(emulated_kernels):
    HC.conv_case('cpu', 2, [3], 64, 6, 9, 5, seed=11)


def test_conv_h16_cat_two_and_three_sources(emulated_kernels):
    HC.conv_case('cpu', 1, [16, 13], 32, 4, 7, 3, seed=12)
    HC.conv_case('cpu', 1, [64, 64, 1], 32, 4, 6, 3, seed=13)          # 129 channels, ragged last source (the decoder's inverse depth)


def test_conv_h16_wide_m_and_f32_source(emulated_kernels):
    HC.conv_case('cpu', 1, [129], 260, 3, 5, 3, seed=14, ksplit=4)      # surplus m-tiles of the 256-row workgroup, K split in 4
    HC.conv_case('cpu', 1, [16], 64, 4, 6, 5, seed=15, w_f32=True)    # the collapsed pack's fp32 composed weight


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('res', [True, False])
def test_groupnorm_h16(emulated_kernels, fused, res):
    HC.groupnorm_case('cpu', 2, 32, 4, 8, res=res, fused=fused)
    HC.groupnorm_case('cpu', 1, 32, 3, 5, res=res, fused=fused)        # HW % 4 != 0: the scalar two-launch form


@pytest.mark.parametrize('nf', [4, 8])
def test_conv3d_h16(emulated_kernels, nf):
    """Every fp16 forward case of tests/pack3d_cases.py (the per-voxel shapes), through the C ABI into NaN-guarded slots."""
    for case in PC.select(PC.FWD16_CASES, nf=nf):
        PC.run_forward16('cpu', case)


def test_movement_h16(emulated_kernels):
    HC.movement_case('cpu', 2, 3, 4, 8)


def test_invdepth_h16(emulated_kernels):
    HC.invdepth_case('cpu', 2, 24, 5, 9)


def test_packed_weight_cache_survives_half_float_round_trip(emulated_kernels):
    """module.half().float() swaps a parameter's storage without bumping its version counter, so the cache key tells the packed fp32
    weight from the fp16-rounded one by the storage address alone -- which the allocator may hand back once the old storage is freed.
    The cache therefore keeps every storage it packed alive: whatever the allocator does, no live tensor can sit at a packed address
    while that packed image is cached.  Checked directly (the storage behind each key is alive, at that address, after the swap), with
    same-size allocations probing for the address, and on the output."""
    import torch
    from packnet_sfm.networks.layers.packnet.layers01 import _HipConv2d
    torch.manual_seed(3)
    conv = _HipConv2d(16, 32, 3)
    x = torch.randn(1, 16, 6, 8)
    with torch.no_grad():
        conv(x)                                          # packs the original fp32 weight
        c = conv._packed
        old = conv.weight.data_ptr()
        for p in conv.parameters():                      # what Module.half() / .float() do: swap .data, same version counter
            p.data = p.data.half()
            p.data = p.data.float()
        assert c._src_f is not None and c._src_f.data_ptr() == c.key_fwd[1] == old, 'packed storage not kept alive'
        probes = [torch.empty_like(conv.weight) for _ in range(16)]
        assert conv.weight.data_ptr() != old and all(p.data_ptr() != old for p in probes), 'packed address reused'
        fresh = _HipConv2d(16, 32, 3)
        fresh.load_state_dict(conv.state_dict())
        assert torch.equal(conv(x), fresh(x))
        h16 = _HipConv2d(16, 32, 3).half()
        h16(x.half())
        assert h16._packed._src_h16[0].data_ptr() == h16._packed.key_h16[0][1]
