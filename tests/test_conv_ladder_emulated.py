"""The emulated twin of tests/test_gpu_conv_ladder.py: the table of tests/conv_fwd_cases.py on the host-emulated kernels -- the
read-back of every launch, the small-integer data and the single-product probes, bit for bit against float64.  (P3 alone leaves the
piece products (2,0) and (0,2) unwatched here -- a kernel without one of them passed this file -- so P1 and P2 take turns with it.)

CPU-suite time: a launch costs 0.1 - 7 s here (a whole case with both directions and both data sets 1 - 30 s), so the table is
thinned by one rotating rule over a case's place i in it (emulated_plan):
  * a case runs ONE direction, its directions[i % 2] (a one-direction case: that one), and ONE data set, by i % 6: the integers
    (0, 1, 3), P3 (2), P1 (4), P2 (5);
  * of the costly cases -- 5x5 / 7x7 layers of 20 or 40 channels and the `many` launches, which repeat the builds of cheaper
    cases on more pixels -- every other one (i % 2 == 0) runs;
  * a build with fewer than seven cases of its own (the stem's, variant 6's and the f32 kernels' middle tiles, the ping-pong builds the LDS forces) runs all four data
    sets in each of them (the f32 kernels, which have no piece products to tell the probes apart: the integers and P3).
Neighbours in the table differ in tile form, kernel size or extra, so a build meets both directions and both data sets, and no build
is dropped: test_emulated_plan_drops_no_build.  The GPU half runs every case, direction and data set."""
import pytest

import conv_fwd_cases as CF


def test_conv_ladder_table_is_sound():
    CF.check_table()


_PER_BUILD = {}
for _c in CF.CASES:
    _PER_BUILD[CF.kernel_of(_c)] = _PER_BUILD.get(CF.kernel_of(_c), 0) + 1


def emulated_plan(i, case):
    """(direction, data set) of case i on the emulator, or None where the rule leaves the case to the GPU."""
    if (case['many'] or (case['ks'] >= 5 and case['K'] >= 20)) and i % 2 == 1:
        return None
    dirs = case['dirs']
    if _PER_BUILD[CF.kernel_of(case)] < 7:
        return dirs[i % len(dirs)], (('int', 'p1', 'p2', 'p3') if case['build'][0] >= 3 else ('int', 'p3'))
    return dirs[i % len(dirs)], (('int', 'int', 'p3', 'int', 'p1', 'p2')[i % 6],)


_PLAN = [(i, emulated_plan(i, c)) for i, c in enumerate(CF.CASES)]
_RUN = [(i, p) for i, p in _PLAN if p is not None]


def test_emulated_plan_drops_no_build():
    """Under the rotating rule every reachable build still runs the integer data, every split-bf16 build (every tile of the
    ping-pong kernel) also each of the three probes, every family every kernel size, and both directions occur for every kernel."""
    reach, _ = CF.expected_builds()
    ran = {CF.kernel_of(CF.CASES[i]) for i, p in _RUN if 'int' in p[1]}
    assert ran == reach, sorted(reach - ran)
    for probe in ('p1', 'p2', 'p3'):
        probed = {CF.kernel_of(CF.CASES[i]) for i, p in _RUN if probe in p[1]}
        assert {k for k in reach if k[0] in ('bx3-2', 'bx3-3', '1x1')} <= probed, (probe, sorted(reach - probed))
        assert {k[:3] for k in reach if k[0] == 'pp'} == {k[:3] for k in probed if k[0] == 'pp'}, probe
    for fam in CF.FAMILIES:
        sizes = {'stem': {5}, 'v8': {1}}.get(fam, {1, 3, 5, 7})
        assert {CF.CASES[i]['ks'] for i, _p in _RUN if CF.CASES[i]['family'] == fam} == sizes, fam
    for kern in {k[0] for k in reach}:
        assert {p[0] for i, p in _RUN if CF.kernel_of(CF.CASES[i])[0] == kern} == {'f', 'b'}, kern


@pytest.mark.parametrize('i', [i for i, _p in _RUN], ids=[CF.CASE_IDS[i] for i, _p in _RUN])
def test_conv_ladder_case_emulated(emulated_kernels, i):
    case = CF.CASES[i]
    d, steps = emulated_plan(i, case)
    CF.run_case('cpu', case, steps=steps, dirs=d)
