"""GPU (MI355X): the stride-1 conv autograd nodes (hip/functional.py: Conv2dFn, ConvGnActFn) with the weight gradient beside the data
gradient -- on the side stream or not, forked by the one C call or the torch way, inside the block sequencer or in the Python bodies.
The host emulator runs everything on one queue; only the device can tell a missing fork, join or wait from a present one."""
import pytest
import torch

import parity_cases as P
from test_kernels_emulated import CONV_NODE_SOURCES, WGRAD_CAT_PINNED, _check_wgrad_cat_pinned, _conv_node_data, _conv_node_run

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# every source configuration with each weight used once, and two with the node applied twice to the same parameters (what a Conv2D
# module called twice in one graph does): their gradients are accumulated on the compute stream, so each node waits for its own
_CASES = [(Cs, tap, gn, False) for Cs, tap in CONV_NODE_SOURCES for gn in (False, True)] + [((32,), False, True, True), ((32, 16), False, True, True)]


@pytest.mark.parametrize('Cs,tap,gn,twice', _CASES)
def test_conv_nodes_side_stream_fork_and_sequencer(Cs, tap, gn, twice):
    """Output and every gradient with the weight-gradient side stream on -- one-call fork on / off x sequencer on / off -- against the
    side stream off, at the tolerance of test_gpu_parity's accumulation test (the K-split kernels use atomics).  With the one-call
    fork off the sequencer must hand the node to the Python body, whose _WgradStream.run forks the torch way."""
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _seq, functional as HF
    WS = HF._WgradStream
    data = _conv_node_data(Cs, 100 + 7 * sum(Cs) + Cs[0])
    assert _seq.get() is not None, 'the sequencer extension must be loaded on the GPU box'
    was_side, was_fork, run = WS.enabled, HF._FAST_FORK, WS.run.__func__
    calls = []

    def spy(cls, *args, **kwargs):
        calls.append(1)
        return run(cls, *args, **kwargs)
    WS.run = classmethod(spy)
    try:
        _conv_node_run(DEV, data, tap, gn, twice)                       # autotune outside the comparison
        HF.set_wgrad_stream(False)
        torch.cuda.synchronize()
        del calls[:]                                                    # (the warm-up ran with the side stream as it was)
        ref = _conv_node_run(DEV, data, tap, gn, twice)
        torch.cuda.synchronize()
        assert not calls
        gmax = max(float(g.abs().max()) for g in ref[1:])
        HF.set_wgrad_stream(True)
        for fast in (True, False):
            HF._FAST_FORK = fast
            for seq_on in (True, False):
                _seq.set_enabled(seq_on)
                del calls[:]
                got = _conv_node_run(DEV, data, tap, gn, twice)
                torch.cuda.synchronize()
                if seq_on and not fast:
                    assert calls, 'the sequencer kept a side-stream weight gradient although the one-call fork is off'
                assert len(got) == len(ref)
                P.check(got[0], ref[0], 2e-5, 'output (fast fork %s, sequencer %s)' % (fast, seq_on))
                for i, (a, b) in enumerate(zip(got[1:], ref[1:])):
                    P.check(a, b, 2e-5, 'gradient %d (fast fork %s, sequencer %s)' % (i, fast, seq_on), floor=1e-2 * gmax)
    finally:
        WS.run = classmethod(run)
        HF._FAST_FORK = was_fork
        HF.set_wgrad_stream(was_side)
        _seq.set_enabled(True)


@pytest.mark.parametrize('kernel', [3, 2])
@pytest.mark.parametrize('case', WGRAD_CAT_PINNED)
def test_conv2d_wgrad_cat_pinned_kernel_gpu(case, kernel):
    """The multi-source (cat) weight gradient pinned to the nine-taps kernel and to wgrad3 (test_kernels_emulated's cases) on the
    device, vs F.conv2d's autograd on the concatenated tensor."""
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    _check_wgrad_cat_pinned(DEV, case, kernel, 5e-5)
