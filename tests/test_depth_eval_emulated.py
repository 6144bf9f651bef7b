"""CPU: the depth-evaluation kernels (csrc/depth_eval.h) compiled for the host and run on the emulator, through the same wrappers and
against the same expectations as on the GPU (tests/depth_eval_cases.py), plus the CPU-tensor paths of packnet_sfm.utils.depth."""
import pytest
import torch

import depth_eval_cases as C

CPU = torch.device('cpu')


@pytest.mark.parametrize('use_gt_scale', [False, True])
@pytest.mark.parametrize('case', [1, 2, 3, 4, 5])
def test_depth_metrics_emulated(emulated_kernels, case, use_gt_scale):
    C.metric_case(CPU, case, use_gt_scale)


def test_depth_metrics_empty_image_emulated(emulated_kernels):
    C.empty_image_case(CPU)


def test_depth_metrics_inverse_emulated(emulated_kernels):
    C.inverse_case(CPU)


@pytest.mark.parametrize('method', ['mean', 'max', 'min'])
def test_post_process_vs_reference_emulated(emulated_kernels, method):
    from packnet_sfm.hip import functional as HF
    C.pp_reference_case(CPU, method, HF.post_process_inv_depth)


@pytest.mark.parametrize('W', [64, 53])
def test_post_process_half_and_symmetry_emulated(emulated_kernels, W):
    for method in ('mean', 'max', 'min'):
        C.pp_half_case(CPU, method, W)
    C.pp_symmetry_case(CPU, W)


def test_post_process_errors_emulated(emulated_kernels):
    C.pp_errors_case(CPU)


def test_evaluate_depth_emulated(emulated_kernels):
    C.evaluate_case(CPU)


# ---- CPU tensors without the emulator: the plain torch expressions of packnet_sfm.utils.depth
@pytest.mark.parametrize('method', ['mean', 'max', 'min'])
def test_post_process_cpu_tensor_path(method):
    from packnet_sfm.hip import _lib
    from packnet_sfm.utils import depth as D
    assert _lib.REQUIRE_CUDA
    C.pp_reference_case(CPU, method, D.post_process_inv_depth)
    inv, inv_f = C.pp_inputs()
    C.rel_close(D.fuse_inv_depth(inv, inv_f, method), {'mean': 0.5 * (inv + inv_f), 'max': torch.max(inv, inv_f), 'min': torch.min(inv, inv_f)}[method],
                0.0, 'fuse_inv_depth')
    with pytest.raises(ValueError):
        D.post_process_inv_depth(inv, inv_f, 'median')


def test_evaluate_depth_cpu_tensor_path():
    from packnet_sfm.hip import _lib
    assert _lib.REQUIRE_CUDA
    C.evaluate_case(CPU)


def test_names_resolve_without_a_reference_checkout():
    from packnet_sfm.utils import depth as D
    for name in ('post_process_inv_depth', 'fuse_inv_depth', 'evaluate_depth', 'crop_window'):
        assert name in vars(D), name
