"""GPU: the depth-input kernels (csrc/depth_input.h) and the transforms over them on the MI355X -- the cases of
tests/depth_input_cases.py, plus KITTI-size runs and run-to-run reproducibility."""
import numpy as np
import pytest
import torch

import depth_input_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', C.PRESERVE_CASES)
def test_depth_resize_preserve(name):
    """torch.equal to the reference's own resize_depth_preserve (tests/golden/depth_input.pt)."""
    C.preserve_case(_dev(), name)


@pytest.mark.parametrize('name', C.NEAREST_CASES)
def test_depth_resize_nearest(name):
    """Against the numpy restatement of the rule in include/pnsfm.h.  OpenCV itself (cv2.resize INTER_NEAREST, what the reference
    calls) is NOT available here: the rule is a restatement and is not pinned against the real library."""
    C.nearest_case(_dev(), name)


def test_depth_resize_window_errors():
    C.window_errors_case(_dev())


@pytest.mark.parametrize('shape', [(2, 19, 64), (1, 5, 7)])
def test_totensor8(shape):
    C.totensor_case(_dev(), *shape)


@pytest.mark.parametrize('case', C.TRAIN_CASES)
def test_train_transform_with_depth(case):
    C.train_case(_dev(), *case)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('borders', [(), (5, 32, 3, 64)])
@pytest.mark.parametrize('mode', ['validation', 'test'])
def test_eval_transform(mode, borders, dtype):
    C.eval_case(_dev(), mode, borders, dtype)


def test_depth_resize_preserve_kitti_size():
    """B = 4, 375x1242 -> 192x640, 5 % valid pixels, against the restatement (itself equal to the reference on every small case:
    test_restatement_matches_golden); the same call twice gives the same bits."""
    from packnet_sfm.hip import ops
    maps = C.depth_maps(4, 375, 1242, 0.05, 61)
    d = torch.from_numpy(maps).to(_dev())
    a = ops.depth_resize_preserve(d, (192, 640))
    b = ops.depth_resize_preserve(d, (192, 640))
    assert torch.equal(a, b)
    exp = torch.from_numpy(np.stack([C.resize_preserve_np(m, (192, 640)) for m in maps]))[:, None]
    assert torch.equal(a.cpu(), exp)


def test_validation_transform_kitti_size_half():
    """The validation transform at KITTI size in fp16 (B = 4, 375x1242 -> 192x640, 5 % valid pixels); the Lanczos expectation from PIL
    is checked on the first and last frame."""
    C.eval_case(_dev(), 'validation', (), torch.float16, B=4, H=375, W=1242, shape=(192, 640), density=0.05, check_frames=(0, 3))
