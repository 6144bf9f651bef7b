"""GPU (MI355X): every weight-gradient kernel build a tuning decision can launch, at kernel level.

  (a) the cases of tests/wgrad_cases.py -- one or more per instantiation of conv2d_wgrad3_kernel (58 reachable) and
      conv2d_wgrad4_kernel (16), multi-source launches and the generic f32 kernel at stride 2 -- pinned (packnet_sfm.hip.tune),
      against float64 at the project's bound (16 * 2^-24 of sum |dY||X|), with the build that ran read back through
      pnsfm_conv2d_last_config, NaN guards around the gradient slots, a bit-identical second launch and the un-split launch next to
      the split one.  The host emulator runs the same table (tests/test_kernels_emulated.py), one fiber at a time: a missing barrier
      around the LDS reduction of the pixel shares, a register-budget build that behaves differently, the MFMA lane layout and the
      buffer-load range checks only show here.
  (b) every weight-gradient line of the shipped tuning database (csrc/tuned_gfx950.db, kinds 12, 22, 112, 1112) replayed at its own
      shape: the build that launches is the one the line names -- no fall-back, no re-route -- and has a case in (a)."""
import pytest
import torch

import wgrad_cases as WC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from packnet_sfm.hip import _lib
    assert _lib.get().pnsfm_build_target() == b'gfx950'
    assert _lib.REQUIRE_CUDA


def test_table_covers_every_reachable_build():
    """The builds the table's cases name are exactly the 58 + 16 the two dispatch ladders can launch (listed in
    wgrad_cases.expected_builds from enqueue_wgrad3 / enqueue_wgrad4); test_wgrad_ladder_case proves each name through the read-back."""
    WC.check_table()


@pytest.mark.parametrize('case', WC.CASES, ids=WC.CASE_IDS)
def test_wgrad_ladder_case(case):
    WC.run_case(DEV, case)


def _wgrad3_WM(Cout, want):
    most = 4 if Cout > 96 else (2 if Cout > 32 else 1)
    return want if want in (1, 2, 4) and want < most else most


def test_shipped_wgrad_decisions_launch_as_written():
    """Replay of the database's weight-gradient lines (zero tensors of the line's shape, autotuner on, shipped database loaded): the
    kernel family, NT / WM / OCC (wgrad3) or WCI / TG / TR (nine taps) and the pixel splits of the launch are the line's, and every
    build reached has a case in tests/wgrad_cases.py."""
    from packnet_sfm.hip import _lib, ops, tune
    lib = _lib.get()
    lines = tune.database_lines()
    tune.unpin()                            # the library defaults; drops the pins earlier tests of this process may have left
    assert ops.tune_shipped_entries() == len(lines), 'the shipped database is not what this process tunes from'
    assert lib.pnsfm_get_conv_math() == 1
    lib.pnsfm_set_autotune(1)
    table = {c['build'] for c in WC.CASES}
    wrong, reached, n = [], {}, 0
    for text, (kind, B, Cin, Cout, HW, W, ks, split, v1) in lines:
        if kind % 10 != 2:
            continue
        assert kind in (12, 22, 112, 1112), 'cannot replay kind %d: %s' % (kind, text)
        n += 1
        S = 2 if kind == 22 else 1
        if ks == 1 and S == 1:              # the key of a 1x1 layer holds the tiling width (32) in place of W
            assert W == 32, text
            H, Wd = (HW // 32, 32) if HW % 32 == 0 else (1, HW)
        else:
            assert HW % W == 0, text
            H, Wd = HW // W, W
        dy = torch.zeros(B, Cout, H, Wd, device=DEV)
        if kind == 1112:                    # (the key does not hold the sources' channel counts: any 32-aligned cut forms it)
            C0 = (Cin - 1) // 32 * 32
            xs = [torch.zeros(B, C0, H, Wd, device=DEV), torch.zeros(B, Cin - C0, H, Wd, device=DEV)]
            dw, db = ops.conv2d_backward_weight_cat(xs, dy, ks)
        elif S == 2:
            xs = [torch.zeros(B, Cin, 2 * H, 2 * Wd, device=DEV)]
            dw, db = ops.conv2d_backward_weight_strided(xs[0], dy, ks, 2)
        else:
            xs = [torch.zeros(B, Cin, H, Wd, device=DEV)]
            dw, db = ops.conv2d_backward_weight(xs[0], dy, ks)
        last = tune.last_config()
        cfg, build = last.raw, last.build
        d = tune.WgradDecision.decode(split, v1)._asdict()
        if d['kernel'] == 2:
            ok = build[0] == 103 and build[1] == ks and (build[2], build[3], build[6]) == (d['NT'], _wgrad3_WM(Cout, d['wm'] & 7), 3 if d['wm'] & 8 else 2)
        elif d['kernel'] == 3:
            ok = (build[0] == 104 and build[1] == (1 if d['WCI'] == 1 else 2) and (d['TG'] == 0 or build[2] == d['TG'])
                  and (d['TR'] == 0 or build[3] == d['TR']))
        elif d['kernel'] == 1:
            ok = build[0] == 102
        else:
            ok = build[0] == (105 if (Cin == 3 and ks == 5 and S == 1) else 100)
        if ok:
            ok = cfg[4] == WC.clamped_split(WC.launched_tiles(cfg, B, H, Wd, ks), split)
        if not ok:
            wrong.append((text, d, cfg))
        if build[0] in (103, 104):
            reached.setdefault(build, text)
        del xs, dy, dw, db
    torch.cuda.synchronize()
    assert n == sum(1 for _t, v in lines if v[0] % 10 == 2) and n > 100
    assert not wrong, 'lines that do not launch as written (line, decoded, last_config): %r' % wrong
    missing = {b: t for b, t in reached.items() if b not in table}
    assert not missing, 'builds the database launches that tests/wgrad_cases.py has no case for: %r' % missing
    print('replayed %d weight-gradient lines; %d distinct split-bf16 builds: %s' % (n, len(reached), sorted(reached)))
