"""CPU: the depth-input kernels (csrc/depth_input.h) compiled for the host and run on the emulator, and the transforms over them
(packnet_sfm/datasets/device_transforms.py), through the same wrappers and against the same expectations as on the GPU
(tests/depth_input_cases.py).  The bar is bit-exact everywhere."""
import pytest
import torch

import depth_input_cases as C

CPU = torch.device('cpu')


@pytest.mark.parametrize('name', C.PRESERVE_CASES)
def test_depth_resize_preserve_emulated(emulated_kernels, name):
    """torch.equal to the reference's own resize_depth_preserve (tests/golden/depth_input.pt)."""
    C.preserve_case(CPU, name)


@pytest.mark.parametrize('name', C.PRESERVE_CASES)
def test_restatement_matches_golden(name):
    """The numpy restatement of tests/depth_input_cases.py equals the reference on every case: that licenses it as the expectation
    of the full-size and transform cases."""
    C.restatement_case(name)


@pytest.mark.parametrize('name', C.NEAREST_CASES)
def test_depth_resize_nearest_emulated(emulated_kernels, name):
    """Against the numpy restatement of the rule in include/pnsfm.h.  OpenCV itself (cv2.resize INTER_NEAREST, what the reference
    calls) is NOT available here: the rule is a restatement and is not pinned against the real library."""
    C.nearest_case(CPU, name)


def test_depth_resize_window_errors_emulated(emulated_kernels):
    C.window_errors_case(CPU)


@pytest.mark.parametrize('shape', [(2, 19, 64), (1, 5, 7)])
def test_totensor8_emulated(emulated_kernels, shape):
    C.totensor_case(CPU, *shape)


@pytest.mark.parametrize('case', C.TRAIN_CASES)
def test_train_transform_with_depth_emulated(emulated_kernels, case):
    C.train_case(CPU, *case)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('borders', [(), (5, 32, 3, 64)])
@pytest.mark.parametrize('mode', ['validation', 'test'])
def test_eval_transform_emulated(emulated_kernels, mode, borders, dtype):
    C.eval_case(CPU, mode, borders, dtype)


def test_get_device_transforms():
    C.get_transforms_case()
