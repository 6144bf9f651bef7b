"""GPU (MI355X): every forward / backward-data decision of the shipped tuning database keeps its launch configuration.

csrc/tuned_gfx950.db is replayed line by line: a launch of the line's own shape (zero tensors -- the configuration depends on the
shape alone) with autotuning on and the shipped database loaded, then the eight ints of pnsfm_conv2d_last_config
(variant, NT, MT, taps per stage, K-split, tile mode, blocks, LDS bytes) are compared with tests/golden/tuned_configs.json.  The
fixture was recorded by replay_database() below on the build of the commit BEFORE the launch policy of conv2d.hip was reorganised
(decision codec, one dispatch, WgradPlan), so a line that decodes, falls back or tiles differently afterwards fails here.
Weight-gradient lines (kinds x2) are not part of this test: tests/test_gpu_wgrad_ladder.py replays them against what each line names."""
import ctypes
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'tuned_configs.json')


def replay_database(ops, lib):
    """Launch every forward / backward-data line once; {line text: the eight ints of pnsfm_conv2d_last_config}."""
    from packnet_sfm.hip import tune
    lines = tune.database_lines()
    tune.unpin()                            # the library defaults; drops the pins earlier tests of this process may have left
    # (in this order: the first query of a process reads the environment and loads the database)
    assert ops.tune_shipped_entries() == len(lines), 'the shipped database is not what this process tunes from'
    lib.pnsfm_set_autotune(1)
    got = {}
    for text, (kind, B, K, M, H, W, ks, _cfg, _split) in lines:
        direction, S, _bx3, several = tune.kind_fields(kind)
        if direction == tune.WGRAD:
            continue
        assert (direction, S) in ((0, 1), (1, 1), (0, 2)) and not several and kind < 200, 'cannot replay kind %d: %s' % (kind, text)
        # the launch forms the line's key only under the arithmetic the line was tuned for (split-bf16 from 16 K-channels on)
        assert (kind >= 100) == (K >= 16 and lib.pnsfm_get_conv_math() == 1), 'cannot replay under this arithmetic: %s' % text
        x = torch.zeros(B, K, H * S, W * S, device=DEV)
        if direction == tune.BACKWARD_DATA:         # K = channels of dy, M = channels of dx
            wp = torch.zeros(ops.conv2d_packed_sizes(M, K, ks)[1], device=DEV)
            y = ops.conv2d_backward_data(x, wp, M, ks)
        else:
            wp = torch.zeros(ops.conv2d_packed_sizes(K, M, ks)[0], device=DEV)
            y = ops.conv2d_forward_strided(x, wp, None, M, ks, 2) if S == 2 else ops.conv2d_forward(x, wp, None, M, ks)
        assert tuple(y.shape) == (B, M, H, W), text
        out = (ctypes.c_int * 8)()
        assert lib.pnsfm_conv2d_last_config(out) == 0
        assert text not in got, 'duplicate database line: %s' % text
        got[text] = list(out)
        del x, wp, y
    torch.cuda.synchronize()
    return got


def test_shipped_decisions_keep_their_launch_configuration():
    assert torch.cuda.is_available(), 'this test needs an MI355X'
    from packnet_sfm.hip import _lib, ops, tune
    lib = _lib.get()
    assert lib.pnsfm_build_target() == b'gfx950' and _lib.REQUIRE_CUDA
    with open(GOLDEN) as f:
        want = json.load(f)
    got = replay_database(ops, lib)
    expected_lines = [text for text, vals in tune.database_lines() if vals[0] % 10 != 2]
    assert expected_lines and sorted(got) == sorted(expected_lines)         # every forward / backward-data line was replayed
    assert sorted(want) == sorted(expected_lines), 'tests/golden/tuned_configs.json does not list the database\'s lines'
    wrong = {text: (got[text], want[text]) for text in expected_lines if got[text] != want[text]}
    assert not wrong, 'launch configuration changed (got, recorded): %r' % wrong
