"""GPU: the depth-evaluation kernels (csrc/depth_eval.h) on the MI355X -- the cases of tests/depth_eval_cases.py, plus run-to-run
reproducibility and the absence of host synchronisation."""
import pytest
import torch

import depth_eval_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('use_gt_scale', [False, True])
@pytest.mark.parametrize('case', [1, 2, 3, 4, 5])
def test_depth_metrics(case, use_gt_scale):
    C.metric_case(_dev(), case, use_gt_scale)


def test_depth_metrics_empty_image():
    C.empty_image_case(_dev())


def test_depth_metrics_inverse():
    C.inverse_case(_dev())


@pytest.mark.parametrize('method', ['mean', 'max', 'min'])
def test_post_process_vs_reference(method):
    from packnet_sfm.hip import functional as HF
    from packnet_sfm.utils import depth as D
    C.pp_reference_case(_dev(), method, HF.post_process_inv_depth)
    C.pp_reference_case(_dev(), method, D.post_process_inv_depth)        # device tensors: the same kernel behind the reference's name


@pytest.mark.parametrize('W', [64, 53])
def test_post_process_half_and_symmetry(W):
    for method in ('mean', 'max', 'min'):
        C.pp_half_case(_dev(), method, W)
    C.pp_symmetry_case(_dev(), W)


def test_post_process_errors():
    C.pp_errors_case(_dev())


def test_evaluate_depth():
    C.evaluate_case(_dev())


@pytest.mark.parametrize('case', [2, 3, 5])
def test_depth_metrics_reproducible(case):
    from packnet_sfm.hip import functional as HF
    gt, pred, (c,) = C.metric_inputs(case)
    g, p = gt.to(_dev()), pred.to(_dev())
    for ugs in (False, True):
        a = HF.depth_metrics(g, p, c.min_depth, c.max_depth, scale_output=c.scale_output, use_gt_scale=ugs, details=True)
        b = HF.depth_metrics(g, p, c.min_depth, c.max_depth, scale_output=c.scale_output, use_gt_scale=ugs, details=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if ugs:
            assert torch.equal(a[2], b[2])


def test_depth_metrics_does_not_sync():
    """Case 2 under torch's sync debug mode: any device->host copy or synchronisation inside the call raises."""
    from packnet_sfm.hip import functional as HF
    gt, pred, (c,) = C.metric_inputs(2)
    g, p = gt.to(_dev()), pred.to(_dev())
    HF.depth_metrics(g, p, c.min_depth, c.max_depth)          # library load, first-use work
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        m = HF.depth_metrics(g, p, c.min_depth, c.max_depth, use_gt_scale=True)
        inv_pp = HF.post_process_inv_depth(p, p, 'mean')
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(inv_pp).all())
