"""Cases of csrc/groupnorm.hip shared by the emulated CPU tests (tests/test_groupnorm_emulated.py) and the GPU tests
(tests/test_gpu_groupnorm.py).  The kernels are called through ops.groupnorm_act_forward / ops.groupnorm_act_backward (so that mean
and rstd are seen), once per form through hip.functional.groupnorm_act, and through ops.groupnorm_act_forward_h16, and compared PER
ELEMENT with float64 torch: F.group_norm of x (+ res) with identity / ELU / ReLU behind it, gradients from autograd on that, mean and
rstd of every (sample, group) from the same float64 data.  Every input is a float32 tensor converted exactly.  No comparison has
an outlier allowance.  The layout is that of tests/sup_head_pose_cases.py.

Measures.  y, dx: |got - ref| / (|ref| + rms of ref over the (sample, group) slab) -- under a max-normalised measure the small
groups are free.  rstd: relative.  mean: of |mean| + std of the slab.  dgamma, dbeta: of the sum of |terms| of that channel
(|dz xhat|, |dz| over samples and pixels, float64).  A second launch must return the bits of the first.
ReLU and ELU route on the sign of z = v sc + sh (sc = rstd gamma, sh = beta - mean sc): an element is left out of the y and dx
comparison when |z64| <= 8 eps32 (|v sc| + |sh|), from the oracle ALONE; a channel with gamma = 0 is never left out (sc = 0 and
sh = beta in the kernels too: z is exact).  The share is asserted before anything is compared: 0.1 % under ELU (which is C1
at 0: a flipped element moves nothing else), and NONE under ReLU (one flipped element moves dbeta by a whole dy), in the exact-z
cases and below 100 elements.  GN_SEEDS holds the seeds, chosen on the CPU from the oracle alone, at which that holds.

Routes.  gn_fused_ok, gn_fused_threads, gn_fused_parts, the NV dispatch, the TPC rule and gn_geom of csrc/groupnorm.hip are
restated below (fused_route, two_launch_route), and every case carries the route it is meant to hit, asserted before it runs:
form; T, NV, S, TPC for the one-launch form; T, rows, nchunk for the two-launch form.  A retuned rule fails there and does not move
a case off its edge.  ONE_LAUNCH and TWO_LAUNCH list the shapes with what each hits; a shape that allows both forms runs both.
Values: VALUE_SHAPES (both forms, S = 1 and S = 4, scalar chunks) run the conditioning classes (mean, std) = (10, 1), (100, 1),
(1, 0.01) beside the (0.3, 2) of every other case (the residual carries half of the offset), one case with one group exactly
constant (var = 0, rstd = 1 / sqrt(eps)) and the exact-z cases: channels with gamma = 0 and beta in EXACT_BETAS, where kernel and
oracle both have z = beta exactly.  That pins gn_expm1_neg at its polynomial / exponential switch (-0.25 and its two neighbours),
at saturation, and act_grad (through dbeta, dgamma, dx).  There y is compared absolutely for z <= 0 (ELU's negative branch and its
derivative are bounded by 1; dbeta and dgamma of those channels are normalised by sum |dy|, sum |dy xhat|) and relatively for
z > 0; ReLU at beta = +-0 must give y = 0 and dgamma = dbeta = 0 exactly, as torch does.  The one-launch kernels change paths where
|mean| = GNF_CENTRE = 4 std (raw squares and v rstd - mean rstd within, centred squares and (v - mean) rstd beyond): the classes
(3.5, 1) and (4.5, 1) run on either side, and every slab's side is asserted from the oracle.

GPU only (GPU_ONLY): (1,16,512,1024) and (1,16,359,361) (nchunk = PNSFM_GN_MAX_SPLIT = 64, vector and scalar: the workspace is used
to its last slot; 50 s each on the emulator), and the shapes with twelve or sixteen slabs of 1024-thread workgroups, 5-10 s each
there: (1,16,128,512), (1,16,4,16385), (1,112,4,439), (1,80,24,160), (3,16,64,64).  All of them passed on the emulator once, when
this table was written.  What they hit stays on the emulator at fewer slabs: S = 4 with a one-float4 last part at (1,28,4,439)
G = 4 (n4 = 3073 again), NV = 8 with an empty part at (1,17,4,241) G = 1, the non-interleaved gnf_slab_part at both.  Everything
else runs on both.

fp16 forward: H16_CASES, the NV / S / fallback edges through tests/half_cases.groupnorm_case (assert_close16 with its `extra`, a
bit-identical second call), the route asserted first.

Tolerances.  Per quantity and conditioning class: the SAME oracle functions in float32 torch on the CPU over the same inputs, their
largest error against float64 in the comparison's own measure over the class's cases (`python tests/groupnorm_cases.py` prints
them), times four -- another summation order, FMA contraction, the device's exp and division -- and not below 4 x 2^-24, so that
an exactly rounding float32 torch does not make a bound unsatisfiable.  Never taken from the kernels."""
import functools
import math

import torch
import torch.nn.functional as F

from loss_cases import EPS32, SMALL, _Ref, _key, _sid, _sync, _to, ids  # noqa: F401

EPS = 1e-5
ACT_ID, ACT_ELU, ACT_RELU = 0, 1, 2
ACT_NAMES = {ACT_ID: 'id', ACT_ELU: 'elu', ACT_RELU: 'relu'}
GNF_MAXCPG, GN_MAX_SPLIT = 128, 64          # csrc/groupnorm.hip, include/pnsfm.h
ELU_CAP = 0.001
FLOOR = 4.0 * 2.0 ** -24

# (mean, std) of x + res per conditioning class; 'const' and 'exact' draw from 'std', and so does 'tiny': the slabs of fewer than 16
# elements (dx lives in what n - 2 dimensions the two projections leave: at n = 3 float32 torch is 40 times further off than at n >= 64)
CLASSES = dict(std=(0.3, 2.0), off10=(10.0, 1.0), off100=(100.0, 1.0), near=(1.0, 0.01), const=(0.3, 2.0), exact=(0.3, 2.0), tiny=(0.3, 2.0),
               under=(3.5, 1.0), over=(4.5, 1.0))
_CLASS_KEY = ('const', 'exact', 'near', 'off10', 'off100', 'std', 'tiny', 'under', 'over')        # position = the class's part of a seed
GNF_CENTRE = 4.0                 # csrc/groupnorm.hip: the one-launch kernels centre a slab whose |mean| exceeds this many std
EXACT_BETAS = (0.0, -0.0, -1e-7, float(torch.nextafter(torch.tensor(-0.25), torch.tensor(-math.inf))), -0.25,
               float(torch.nextafter(torch.tensor(-0.25), torch.tensor(math.inf))), -1.0, -20.0, -88.0, -104.0, 3.0)

# The measured float32-torch baselines (one thread), per class and quantity; the tolerance is max(4 x baseline, 4 x 2^-24) (tol()).
# `yz`: y on the exact-z channels, absolute for z <= 0 and relative for z > 0.
GN_BASE = {
    'std': dict(y=1.98e-07, dx=1.97e-07, mean=2.72e-08, rstd=1.2e-07, dgamma=1.46e-07, dbeta=6.08e-08),
    'tiny': dict(y=5.26e-07, dx=8.96e-05, mean=5.8e-08, rstd=1.21e-07, dgamma=4.97e-07, dbeta=4.99e-08),
    'off10': dict(y=3e-06, dx=1.92e-06, mean=1.25e-07, rstd=2.17e-07, dgamma=4.71e-07, dbeta=1.07e-07),
    'off100': dict(y=2.45e-05, dx=1.56e-05, mean=1.07e-07, rstd=1.36e-06, dgamma=3.9e-06, dbeta=4.39e-07),
    'near': dict(y=2.86e-05, dx=1.65e-05, mean=1.21e-07, rstd=1.07e-06, dgamma=5.18e-06, dbeta=4.04e-07),
    # (the constant group: sh = beta - mean sc with sc = gamma / sqrt(eps) = 316 gamma is rounded at 400 and z = beta is of order 0.3)
    'const': dict(y=3.05e-05, dx=1.11e-05, mean=2.35e-08, rstd=8.97e-08, dgamma=7.17e-06, dbeta=5.01e-07),
    # (3.5, 1) and (4.5, 1): either side of GNF_CENTRE, where the one-launch kernels change from raw to centred sums
    'under': dict(y=7.96e-07, dx=5.56e-07, mean=7.53e-08, rstd=1.2e-07, dgamma=1.73e-07, dbeta=2.43e-08),
    'over': dict(y=1.46e-06, dx=9.1e-07, mean=1.2e-07, rstd=1.33e-07, dgamma=1.82e-07, dbeta=3.81e-08),
    'exact': dict(y=1.45e-07, dx=1.67e-07, mean=1.76e-08, rstd=9.25e-08, dgamma=3.52e-08, dbeta=2.08e-08, yz=9.15e-09),
}
QUANTITIES = ('y', 'dx', 'mean', 'rstd', 'dgamma', 'dbeta')


def tol(cls, q):
    return max(4.0 * GN_BASE[cls][q], FLOOR)


# ------------------------------------------------------------------------------------------------ the launchers' rules, restated
def _cdiv(a, b):
    return -(-a // b)


def fused_route(B, C, HW, G):
    """What pnsfm_groupnorm_act_forward / _backward choose with the one-launch form on: None where gn_fused_ok refuses, else
    T (gn_fused_threads), NV (the template the forward dispatches: 1, 2, 4, 8, 16), S (gn_fused_parts), TPC (threads per channel of
    the backward's parameter blocks) and n4, nslab."""
    cpg = C // G
    if HW % 4 != 0 or cpg > GNF_MAXCPG:
        return None
    n4 = cpg * (HW // 4)
    if n4 > 16 * 1024:
        return None
    T = 1024 if n4 > 2048 else 256
    nv = _cdiv(n4, T)
    S = 4 if (T == 1024 and nv >= 4) else 1
    NV = next(v for v in (1, 2, 4, 8, 16) if nv <= v)
    TPC = 64
    while TPC < T and B * (HW // 4) > 8 * TPC:
        TPC <<= 1
    return dict(form='one', T=T, NV=NV, S=S, TPC=TPC, n4=n4, nslab=B * G)


def two_launch_route(B, C, HW, G):
    """gn_geom(B * C, HW, HW % 4 == 0, PNSFM_GN_MAX_SPLIT): lanes per row, rows per workgroup, chunks per row, and the last chunk's
    elements."""
    vec = HW % 4 == 0
    units = HW // 4 if vec else HW
    T = 256
    while T > 1 and units < 4 * T:
        T >>= 1
    rows = 256 // T
    want = min(max(_cdiv(1024, _cdiv(B * C, rows)), 1), GN_MAX_SPLIT)
    per_pass = (4 if vec else 1) * T
    chunk = max(_cdiv(_cdiv(HW, want), per_pass) * per_pass, 8 * per_pass)
    if chunk >= HW:
        chunk = HW
    nchunk = _cdiv(HW, chunk)
    return dict(form='two', vec=vec, T=T, rows=rows, nchunk=nchunk, last=HW - (nchunk - 1) * chunk)


def route_of(shape, G, fused):
    B, C, H, W = shape
    r = fused_route(B, C, H * W, G) if fused else None
    return r if r is not None else two_launch_route(B, C, H * W, G)


def bwd_parts(n4, T, S):
    """float4 each part of a slab writes in the one-launch backward (gn_fused_bwd_kernel: `per`, `lo`, `hi`)"""
    per = _cdiv(_cdiv(n4, S), T) * T
    return [max(0, min(n4, (p + 1) * per) - p * per) for p in range(S)]


# ------------------------------------------------------------------------------------------------ the tables
# (shape, G, the route the one-launch form must take (None: it refuses and the two-launch form runs), what the shape hits)
ONE_LAUNCH = [
    ((3, 16, 2, 2), 16, dict(T=256, NV=1, S=1, TPC=64, n4=1), 'one live lane'),
    ((1, 16, 16, 64), 16, dict(T=256, NV=1, S=1, TPC=64, n4=256), 'NV = 1, full'),
    ((1, 16, 4, 257), 16, dict(T=256, NV=2, S=1, TPC=64, n4=257), 'NV = 2, one-element tail'),
    ((2, 48, 12, 57), 16, dict(T=256, NV=4, S=1, TPC=64, n4=513), 'NV = 4; HW4 = 171 < T: the carry in ch / pos; cpg = 3: surplus parameter rows'),
    ((1, 16, 32, 256), 16, dict(T=256, NV=8, S=1, TPC=256, n4=2048), 'last T = 256'),
    ((1, 48, 4, 683), 16, dict(T=1024, NV=4, S=1, TPC=128, n4=2049), 'first T = 1024; NV = 4, S = 1'),
    ((1, 16, 96, 128), 16, dict(T=1024, NV=4, S=1, TPC=512, n4=3072), 'last S = 1'),
    ((1, 112, 4, 439), 16, dict(T=1024, NV=4, S=4, TPC=64, n4=3073), 'first S = 4; the last backward part holds one float4'),
    ((1, 17, 4, 241), 1, dict(T=1024, NV=8, S=4, TPC=64, n4=4097, nslab=1), 'NV = 8, S = 4; backward part 2 one float4, part 3 empty; one slab'),
    ((3, 16, 64, 64), 4, dict(T=1024, NV=4, S=4, TPC=512, n4=4096, nslab=12), 'nslab = 12: the non-interleaved gnf_slab_part with S = 4'),
    ((1, 80, 24, 160), 16, dict(T=1024, NV=8, S=4, TPC=128, n4=4800), 'nv = 5 in NV = 8'),
    ((1, 128, 4, 4), 1, dict(T=256, NV=2, S=1, TPC=64, n4=512), 'cpg = GNF_MAXCPG'),
    ((1, 129, 4, 4), 1, None, 'cpg = GNF_MAXCPG + 1: falls to the two-launch form'),
    ((1, 16, 128, 512), 16, dict(T=1024, NV=16, S=4, TPC=1024, n4=16384), 'NV = 16, S = 4: the largest slab'),
    ((1, 16, 4, 16385), 16, None, 'n4 = 16385: falls to the two-launch form'),
    # the backward's parameter blocks: TPC = 128 and 256 = T (CPB = 1) of a 256-thread workgroup, 128, 512 (row sums through LDS)
    # and 1024 = T of a 1024-thread one
    ((9, 4, 16, 16), 4, dict(T=256, NV=1, S=1, TPC=128, n4=64), 'TPC = 128 of T = 256'),
    ((17, 4, 16, 16), 4, dict(T=256, NV=1, S=1, TPC=256, n4=64), 'TPC = T = 256: CPB = 1'),
    ((1, 8, 4, 516), 2, dict(T=1024, NV=4, S=1, TPC=128, n4=2064), 'TPC = 128 of T = 1024'),
    ((4, 8, 4, 516), 2, dict(T=1024, NV=4, S=1, TPC=512, n4=2064), 'TPC = 512: LDS row sum over 8 waves'),
    ((8, 8, 4, 516), 2, dict(T=1024, NV=4, S=1, TPC=1024, n4=2064), 'TPC = T = 1024: CPB = 1'),
]
# (shape, G, the two-launch route, what it hits)
TWO_LAUNCH = [
    ((3, 48, 1, 1), 16, dict(vec=False, T=1, rows=256, nchunk=1), 'HW = 1: one lane per row, 256 rows, 112 surplus rows'),
    ((3, 48, 5, 7), 16, dict(vec=False, T=8, rows=32, nchunk=1), 'scalar loads; B C = 144 is no multiple of 32 rows'),
    ((1, 16, 45, 47), 16, dict(vec=False, T=256, rows=1, nchunk=2, last=67), 'scalar with chunks: the second holds 67 elements'),
    ((1, 16, 3, 2732), 16, dict(vec=True, T=256, rows=1, nchunk=2, last=4), 'vector with chunks: the second holds one float4'),
    ((1, 3, 24, 88), 3, dict(vec=True, T=128, rows=2, nchunk=1), 'T = 128 rows (LDS row sum); B C = 3 is no multiple of 2 rows'),
    ((2, 16, 32, 128), 16, dict(vec=True, T=256, rows=1, nchunk=1), 'T = 256 rows'),
    ((1, 16, 512, 1024), 16, dict(vec=True, T=256, rows=1, nchunk=64, last=8192), 'nchunk = PNSFM_GN_MAX_SPLIT, vector'),
    ((1, 16, 359, 361), 16, dict(vec=False, T=256, rows=1, nchunk=64, last=575), 'nchunk = PNSFM_GN_MAX_SPLIT, scalar'),
]
FALLBACK_ROUTES = {(1, 129, 4, 4): dict(vec=True, T=1, rows=256, nchunk=1), (1, 16, 4, 16385): dict(vec=True, T=256, rows=1, nchunk=9, last=4)}
GPU_ONLY = {(1, 16, 128, 512), (1, 16, 512, 1024), (1, 16, 359, 361), (1, 16, 4, 16385), (1, 112, 4, 439), (1, 80, 24, 160), (3, 16, 64, 64)}
# shapes of the value cases: (shape, G): one-launch S = 1 with one float4 per thread and with the ch / pos carry, one-launch S = 4
# (n4 = 3073 again, on four slabs of seven channels), two-launch scalar with chunks
VALUE_SHAPES = [((2, 32, 8, 16), 16), ((2, 48, 12, 57), 16), ((1, 28, 4, 439), 4), ((1, 16, 45, 47), 16)]
EXACT_SHAPES = [((2, 48, 12, 57), 16), ((1, 28, 4, 439), 4)]
# seeds chosen on the CPU, from the oracle alone, so that every case meets its cap (check_case): (shape, G, act, res, cls) -> seed
GN_SEEDS = {((1, 16, 32, 256), 16, 2, True, 'std'): 1, ((2, 32, 8, 16), 16, 1, True, 'over'): 6, ((2, 32, 8, 16), 16, 1, True, 'under'): 2}


def _case(shape, G, act, res, cls, fused, expect, note=''):
    form = 'one' if (fused and expect is not None and expect.get('form', 'one') == 'one') else 'two'
    return dict(id='gn-%s-g%d-%s-%s-%s-%s' % (_sid(shape), G, ACT_NAMES[act], 'res' if res else 'nores', cls, form + ('' if fused else '-forced')),
                shape=shape, G=G, act=act, res=res, cls=cls, fused=fused, expect=expect, note=note)


def _both_forms(shape, G, act, res, cls, one, two, note=''):
    """the case under fused = 1 (route `one`, or `two` where the one-launch form refuses) and under fused = 0 (route `two`)"""
    first = dict(one, form='one') if one is not None else dict(two, form='two')
    return [_case(shape, G, act, res, cls, 1, first, note), _case(shape, G, act, res, cls, 0, dict(two, form='two'), note)]


def _two_of(shape, G):
    B, C, H, W = shape
    r = two_launch_route(B, C, H * W, G)
    return {k: r[k] for k in ('vec', 'T', 'rows', 'nchunk', 'last')}


def _cls_of(shape, G):
    return 'tiny' if shape[1] // G * shape[2] * shape[3] < 16 else 'std'


_ACTS = ((ACT_ELU, True), (ACT_RELU, False), (ACT_ID, True), (ACT_ELU, False), (ACT_RELU, True), (ACT_ID, False))
ROUTE_CASES = []
for _i, (_s, _g, _r, _note) in enumerate(ONE_LAUNCH):
    _a, _res = _ACTS[_i % len(_ACTS)]
    if _r is None:          # the one-launch form refuses: fused = 1 and fused = 0 take the same kernels, one run
        ROUTE_CASES.append(_case(_s, _g, _a, _res, 'std', 1, dict(FALLBACK_ROUTES[_s], form='two'), _note))
    else:                   # (the forced two-launch route of a one-launch shape is whatever gn_geom gives: restated, not tabled)
        ROUTE_CASES += _both_forms(_s, _g, _a, _res, _cls_of(_s, _g), _r, _two_of(_s, _g), _note)
for _i, (_s, _g, _r, _note) in enumerate(TWO_LAUNCH):
    _a, _res = _ACTS[(_i + 1) % len(_ACTS)]
    if _s in GPU_ONLY:
        _a = ACT_ELU        # (ReLU allows no masked element: not at 8 M elements)
    ROUTE_CASES.append(_case(_s, _g, _a, _res, _cls_of(_s, _g), 0, dict(_r, form='two'), _note))
    if _s == (1, 16, 3, 2732):                      # n4 = 2049: with the one-launch form on it is the first T = 1024 slab again
        ROUTE_CASES.append(_case(_s, _g, _a, _res, 'std', 1, dict(form='one', T=1024, NV=4, S=1, TPC=512, n4=2049), _note))
VALUE_CASES = []
for _s, _g in VALUE_SHAPES:
    for _cls, _a in (('off10', ACT_ELU), ('off100', ACT_ELU), ('off100', ACT_ID), ('near', ACT_ELU), ('near', ACT_ID), ('under', ACT_ELU),
                     ('over', ACT_ELU)):
        VALUE_CASES += _both_forms(_s, _g, _a, True, _cls, fused_route(_s[0], _s[1], _s[2] * _s[3], _g), _two_of(_s, _g))
    VALUE_CASES += _both_forms(_s, _g, ACT_ELU, True, 'const', fused_route(_s[0], _s[1], _s[2] * _s[3], _g), _two_of(_s, _g))
for _s, _g in EXACT_SHAPES:
    for _a in (ACT_ELU, ACT_RELU):
        VALUE_CASES += _both_forms(_s, _g, _a, False, 'exact', fused_route(_s[0], _s[1], _s[2] * _s[3], _g), _two_of(_s, _g))
# a shape that the one-launch form refuses runs the same kernels under both settings: keep one
VALUE_CASES = [c for c in VALUE_CASES if not (c['fused'] == 0 and fused_route(c['shape'][0], c['shape'][1], c['shape'][2] * c['shape'][3], c['G']) is None)]
CASES = ROUTE_CASES + VALUE_CASES
CASES_EMU = [c for c in CASES if c['shape'] not in GPU_ONLY]
# hip.functional.groupnorm_act with a residual, one case per form
FUNCTIONAL_CASES = [_case((2, 48, 12, 57), 16, ACT_ELU, True, 'std', 1, dict(form='one', T=256, NV=4, S=1, TPC=64, n4=513)),
                    _case((2, 48, 12, 57), 16, ACT_ELU, True, 'std', 0, dict(_two_of((2, 48, 12, 57), 16), form='two'))]
# fp16 forward: (shape, G, fused, act, res, the route)
H16_CASES = [dict(id='gn16-%s-g%d-%s-%s-%s' % (_sid(s), g, ACT_NAMES[a], 'res' if r else 'nores', 'one' if e.get('form') == 'one' else 'two'),
                  shape=s, G=g, fused=f, act=a, res=r, expect=e)
             for s, g, f, a, r, e in [
                 ((3, 16, 2, 2), 16, 1, ACT_ELU, True, dict(form='one', T=256, NV=1, S=1)),
                 ((1, 16, 4, 257), 16, 1, ACT_ID, False, dict(form='one', T=256, NV=2, S=1)),
                 ((2, 48, 12, 57), 16, 1, ACT_ELU, True, dict(form='one', T=256, NV=4, S=1)),
                 ((1, 16, 32, 256), 16, 1, ACT_ELU, False, dict(form='one', T=256, NV=8, S=1)),
                 ((1, 48, 4, 683), 16, 1, ACT_ID, True, dict(form='one', T=1024, NV=4, S=1)),
                 ((1, 28, 4, 439), 4, 1, ACT_ELU, True, dict(form='one', T=1024, NV=4, S=4)),
                 ((1, 17, 4, 241), 1, 1, ACT_ELU, False, dict(form='one', T=1024, NV=8, S=4, nslab=1)),
                 ((3, 16, 64, 64), 4, 1, ACT_ELU, True, dict(form='one', T=1024, NV=4, S=4, nslab=12)),
                 ((1, 128, 4, 4), 1, 1, ACT_ELU, True, dict(form='one', T=256, NV=2, S=1)),
                 ((1, 129, 4, 4), 1, 1, ACT_ELU, True, dict(form='two', vec=True, T=1, rows=256, nchunk=1)),
                 ((1, 16, 3, 2732), 16, 0, ACT_ELU, True, dict(form='two', vec=True, T=256, rows=1, nchunk=2, last=4)),
                 ((1, 16, 45, 47), 16, 0, ACT_ID, True, dict(form='two', vec=False, T=256, rows=1, nchunk=2, last=67)),
             ]]
for _cases in (CASES, FUNCTIONAL_CASES, H16_CASES):
    assert len({c['id'] for c in _cases}) == len(_cases), [c['id'] for c in _cases]


def check_route(case):
    """The route the launchers' restated rules give this case is the one the table says."""
    got = route_of(case['shape'], case['G'], case['fused'])
    for k, v in case['expect'].items():
        assert got.get(k) == v, '%s: the rules give %s = %r, the table says %r (%r)' % (case['id'], k, got.get(k), v, got)
    return got


# ------------------------------------------------------------------------------------------------ inputs and the oracle
def exact_channels(C):
    """channel -> beta of the exact-z channels: spread over the groups, never the first channel of the tensor alone"""
    step = max(1, C // len(EXACT_BETAS))
    return {(1 + i * step) % C: b for i, b in enumerate(EXACT_BETAS)}


@functools.lru_cache(maxsize=4)
def gn_inputs(shape, G, act, res, cls):
    """float32 x, res (or None), gamma, beta, dy.  x + res has the class's mean and std; res carries half of the offset."""
    B, C, H, W = shape
    mean, std = CLASSES[cls]
    g = torch.Generator().manual_seed(_key(shape, G, act, int(res), _CLASS_KEY.index(cls), GN_SEEDS.get((shape, G, act, res, cls), 0)))

    def rn(*size):
        return torch.randn(*size, generator=g, dtype=torch.float64)

    if res:
        x, r = (0.5 * mean + 0.8 * std * rn(B, C, H, W)).float(), (0.5 * mean + 0.6 * std * rn(B, C, H, W)).float()
    else:
        x, r = (mean + std * rn(B, C, H, W)).float(), None
    gamma, beta = (1.0 + 0.3 * rn(C)).float(), (0.3 * rn(C)).float()
    dy = rn(B, C, H, W).float()
    if cls == 'const':              # the last group of sample 0: x + res = 1.25 exactly
        cpg = C // G
        x[0, C - cpg:] = 0.75 if res else 1.25
        if res:
            r[0, C - cpg:] = 0.5
    if cls == 'exact':
        for c, b in exact_channels(C).items():
            gamma[c], beta[c] = 0.0, b
    return x, r, gamma, beta, dy


def _act(z, act):
    return F.elu(z) if act == ACT_ELU else F.relu(z) if act == ACT_RELU else z


def oracle(x, res, gamma, beta, dy, G, act):
    """y, dx (= d res), dgamma, dbeta, mean, rstd in the dtype of the inputs (float64: the oracle; float32: the baseline, whose mean
    and rstd are the ones torch's own group norm returns)."""
    B, C = x.shape[:2]
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    v = x + res if res is not None else x
    y = _act(F.group_norm(v, G, gamma, beta, EPS), act)
    y.backward(dy)
    vd = v.detach()
    if vd.dtype == torch.float64:
        s = vd.reshape(B, G, -1)
        mean = s.mean(2)
        rstd = 1.0 / torch.sqrt(((s - mean[:, :, None]) ** 2).mean(2) + EPS)
    else:
        _, mean, rstd = torch.native_group_norm(vd, gamma.detach(), beta.detach(), B, C, vd[0, 0].numel(), G, EPS)
    return y.detach(), x.grad, gamma.grad, beta.grad, mean.reshape(B, G), rstd.reshape(B, G)


def _slab(t, G):
    return t.reshape(t.shape[0], G, -1)


def _slab_rms(t, G):
    return _slab(t, G).pow(2).mean(2).sqrt().repeat_interleave(t.shape[1] // G, 1)[:, :, None, None].expand_as(t)


@functools.lru_cache(maxsize=2)
def reference(shape, G, act, res, cls):
    """The float64 oracle of one (shape, G, act, res, class): shared by both forms, the functional case and both devices."""
    B, C, H, W = shape
    cpg = C // G
    r = _Ref()
    r.inputs = gn_inputs(shape, G, act, res, cls)
    x, rs, gamma, beta, dy = (t.double() if t is not None else None for t in r.inputs)
    r.y, r.dx, r.dgamma, r.dbeta, r.mean, r.rstd = oracle(x, rs, gamma, beta, dy, G, act)
    v = x + rs if rs is not None else x
    r.std = _slab(v, G).std(2, unbiased=False)
    ch = lambda t: t.repeat_interleave(cpg, 1)[:, :, None, None]          # noqa: E731  [B, G] -> [B, C, 1, 1]
    xhat = (v - ch(r.mean)) * ch(r.rstd)
    sc = ch(r.rstd) * gamma[None, :, None, None]
    sh = beta[None, :, None, None] - ch(r.mean) * sc
    r.z = v * sc + sh
    exact = torch.zeros(C, dtype=torch.bool)
    if cls == 'exact':
        exact[list(exact_channels(C))] = True
        assert bool((r.z[:, exact] == beta[exact][None, :, None, None]).all())
    r.exact = exact
    if act == ACT_ID:
        r.excluded = torch.zeros_like(r.z, dtype=torch.bool)
        slope = torch.ones_like(r.z)
    else:
        r.excluded = (r.z.abs() <= 8.0 * EPS32 * ((v * sc).abs() + sh.abs())) & (gamma != 0)[None, :, None, None]
        slope = torch.where(r.z > 0, torch.ones_like(r.z), torch.exp(r.z) if act == ACT_ELU else torch.zeros_like(r.z))
    slope[:, exact] = 1.0           # the exact-z channels: dbeta, dgamma absolutely, in units of sum |dy|, sum |dy xhat|
    dz = dy * slope
    r.n_dbeta, r.n_dgamma = dz.abs().sum((0, 2, 3)), (dz * xhat).abs().sum((0, 2, 3))
    r.n_y, r.n_dx = r.y.abs() + _slab_rms(r.y, G), r.dx.abs() + _slab_rms(r.dx, G)
    return r


def check_case(case):
    """What a case promises, from the oracle alone: its route, its class, and the cap on the excluded share."""
    shape, G, act, res, cls = (case[k] for k in ('shape', 'G', 'act', 'res', 'cls'))
    route = check_route(case)
    if route['form'] == 'one' and route['S'] == 4 and 'one float4' in case['note']:
        assert 1 in bwd_parts(route['n4'], route['T'], 4), case['id']
    r = reference(shape, G, act, res, cls)
    n, nex = r.z.numel(), int(r.excluded.sum())
    cap = ELU_CAP if (act == ACT_ELU and cls != 'exact' and n >= SMALL) else 0.0
    assert nex <= cap * n, '%s: the oracle alone excludes %d of %d elements (cap %g)' % (case['id'], nex, n, cap)
    mean, std = CLASSES[cls]
    if shape[2] * shape[3] * (shape[1] // G) >= 512 and cls != 'const':
        assert bool(((r.mean - mean).abs() <= 0.25 * std).all()) and bool(((r.std / std - 1).abs() <= 0.25).all())
    if cls in ('under', 'over'):    # every slab on its side of the threshold between raw and centred sums, with room for fp32
        side = r.mean.abs() * r.rstd
        assert bool((side < 0.95 * GNF_CENTRE).all()) if cls == 'under' else bool((side > 1.05 * GNF_CENTRE).all()), case['id']
    if cls == 'const':
        assert float(r.std[0, G - 1]) == 0.0 and abs(float(r.rstd[0, G - 1]) * math.sqrt(EPS) - 1.0) < 1e-12
    return nex / n


def errors(got, r, G, cls):
    """{quantity: per-element error in the comparison's measure}; y and dx carry 0 on the excluded elements."""
    y, dx, dgamma, dbeta, mean, rstd = (t.detach().double().cpu() for t in got)
    keep = ~r.excluded
    e = dict(y=torch.where(keep, (y - r.y).abs() / r.n_y, torch.zeros_like(r.y)),
             dx=torch.where(keep, (dx - r.dx).abs() / r.n_dx, torch.zeros_like(r.dx)),
             mean=(mean.reshape(r.mean.shape) - r.mean).abs() / (r.mean.abs() + r.std),
             rstd=(rstd.reshape(r.rstd.shape) / r.rstd - 1.0).abs(),
             dgamma=(dgamma - r.dgamma).abs() / r.n_dgamma, dbeta=(dbeta - r.dbeta).abs() / r.n_dbeta)
    for q in ('y', 'dx', 'dgamma', 'dbeta'):        # a normaliser of exactly 0 (every term is exactly 0) asks for exactly 0
        num = {'y': y, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta}[q]
        den = {'y': r.n_y, 'dx': r.n_dx, 'dgamma': r.n_dgamma, 'dbeta': r.n_dbeta}[q]
        e[q] = torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)), e[q])
    if cls == 'exact':              # y on the exact-z channels: absolute for z <= 0 (bounded by 1), relative for z > 0
        yz, rz = y[:, r.exact], r.y[:, r.exact]
        e['yz'] = (yz - rz).abs() / torch.where(r.z[:, r.exact] > 0, rz.abs(), torch.ones_like(rz))
    return e


class _Form(object):
    """`with _Form(lib, fused):` -- pnsfm_set_gn_fused for the block; the previous setting comes back on exit."""

    def __init__(self, fused):
        from packnet_sfm.hip import _lib
        self.lib, self.fused = _lib.get(), fused

    def __enter__(self):
        self.prev = self.lib.pnsfm_set_gn_fused(self.fused)

    def __exit__(self, *exc):
        self.lib.pnsfm_set_gn_fused(self.prev)


def _report(case, e, baseline):
    worst = {q: float(v[torch.isfinite(v)].max()) if baseline else float(v.max()) for q, v in e.items()}
    print('%s%s: %s' % (case['id'], ' [float32 torch]' if baseline else '', '  '.join('%s %.3g' % (q, worst[q]) for q in sorted(worst))))
    return worst


def _assert_errors(case, e, r):
    cls = case['cls']
    for q, v in e.items():
        assert bool(torch.isfinite(v).all()), '%s: %s not finite or not exactly 0 where the reference allows nothing else' % (case['id'], q)
        bad = v > tol(cls, q)
        assert not bool(bad.any()), '%s: %d %s values past %.3g (worst %.3g), first %s' % (
            case['id'], int(bad.sum()), q, tol(cls, q), float(v.max()), bad.nonzero()[0].tolist())


def run_case(device, case, baseline=False):
    """One case through ops.groupnorm_act_forward / _backward, twice (bit-identical), against the oracle.  baseline: the oracle in
    float32 torch in place of the kernels; returns {quantity: worst error}."""
    from packnet_sfm.hip import ops
    shape, G, act, res, cls = (case[k] for k in ('shape', 'G', 'act', 'res', 'cls'))
    check_case(case)
    r = reference(shape, G, act, res, cls)
    x, rs, gamma, beta, dy = r.inputs
    if baseline:
        y, dx, dgamma, dbeta, mean, rstd = oracle(x, rs, gamma, beta, dy, G, act)
        return _report(case, errors((y, dx, dgamma, dbeta, mean, rstd), r, G, cls), True)
    d = [t.to(device) if t is not None else None for t in (x, rs, gamma, beta, dy)]
    with _Form(case['fused']):
        runs = []
        for _ in range(2):
            y, mean, rstd = ops.groupnorm_act_forward(d[0], d[1], d[2], d[3], G, EPS, act)
            dx, dgamma, dbeta = ops.groupnorm_act_backward(d[4], d[0], d[1], d[2], d[3], mean, rstd, G, act)
            _sync(device)
            runs.append(tuple(t.clone() for t in (y, dx, dgamma, dbeta, mean, rstd)))
    assert runs[0][0].shape == x.shape and runs[0][1].shape == x.shape and tuple(runs[0][4].shape) == (shape[0] * G,)
    for a, b, q in zip(runs[0], runs[1], ('y', 'dx', 'dgamma', 'dbeta', 'mean', 'rstd')):
        assert torch.equal(a, b), '%s: a second launch returns another %s' % (case['id'], q)
    e = errors(runs[0], r, G, cls)
    worst = _report(case, e, False)
    _assert_errors(case, e, r)
    if cls == 'exact' and act == ACT_RELU:          # beta = +-0: y, dgamma and dbeta exactly 0, as torch gives them
        y, _, dgamma, dbeta = (t.cpu() for t in runs[0][:4])
        for c, b in exact_channels(shape[1]).items():
            if b <= 0:
                assert bool((y[:, c] == 0).all()) and float(dgamma[c]) == 0.0 and float(dbeta[c]) == 0.0, '%s: channel %d (beta %r)' % (case['id'], c, b)
                assert bool((r.y[:, c] == 0).all()) and float(r.dgamma[c]) == 0.0 and float(r.dbeta[c]) == 0.0
    return worst


def run_functional(device, case):
    """hip.functional.groupnorm_act with a residual: output and every gradient against the oracle, and the residual's gradient is
    what GroupNormActFn.backward is written to return -- the gradient of x itself (d(x + res) / dres = 1)."""
    from packnet_sfm.hip import functional as HF
    shape, G, act, cls = case['shape'], case['G'], case['act'], case['cls']
    check_case(case)
    r = reference(shape, G, act, True, cls)
    x, rs, gamma, beta = (t.clone().to(device).requires_grad_(True) for t in r.inputs[:4])       # (clones: the reference is shared)
    with _Form(case['fused']):
        y = HF.groupnorm_act(x, gamma, beta, G, EPS, act, res=rs)
        y.backward(r.inputs[4].to(device))
        _sync(device)
    assert torch.equal(x.grad, rs.grad), case['id'] + ': the gradient of the residual is not the gradient of x'
    e = errors((y, x.grad, gamma.grad, beta.grad, r.mean, r.rstd), r, G, cls)
    _report(case, e, False)
    _assert_errors(case, e, r)


def run_h16(device, case):
    """ops.groupnorm_act_forward_h16 at a routing edge: half_cases.groupnorm_case (one fp16 ulp of the float64 value + its `extra`,
    a bit-identical second call)."""
    import half_cases as HC
    check_route(case)
    B, C, H, W = case['shape']
    HC.groupnorm_case(device, B, C, H, W, G=case['G'], res=case['res'], act=case['act'], seed=_key(case['shape'], 5) % 10007, fused=case['fused'])


# ------------------------------------------------------------------------------------------------ the float32-torch baselines
def measure_baselines():
    """Largest error of the oracle in float32 torch against float64, per class and quantity, over the compared elements of all the
    class's cases: the numbers beside the tolerances above."""
    out = {}
    for c in CASES:
        if c['fused'] == 0 and any(o['fused'] == 1 and all(o[k] == c[k] for k in ('shape', 'G', 'act', 'res', 'cls')) for o in CASES):
            continue                # the same inputs as the fused = 1 case
        w = run_case('cpu', c, baseline=True)
        for q, v in w.items():
            out.setdefault(c['cls'], {})[q] = max(out.get(c['cls'], {}).get(q, 0.0), v)
    for cls in sorted(out):
        print("    '%s': dict(%s)," % (cls, ', '.join('%s=%.3g' % (q, out[cls][q]) for q in QUANTITIES + (('yz',) if 'yz' in out[cls] else ()))))
        for q, v in out[cls].items():
            print('%-8s %-7s baseline %.3g   committed %.3g   tolerance %.3g' % (cls, q, v, GN_BASE[cls].get(q, float('nan')), tol(cls, q)))
    return out


def choose_seeds():
    """The smallest seed per (shape, G, act, res, class) at which check_case holds: prints the GN_SEEDS table."""
    for c in CASES:
        key = tuple(c[k] for k in ('shape', 'G', 'act', 'res', 'cls'))
        for seed in range(64):
            GN_SEEDS[key] = seed
            gn_inputs.cache_clear()
            reference.cache_clear()
            try:
                check_case(c)
                break
            except AssertionError:
                continue
        else:
            raise AssertionError('no seed for %s' % c['id'])
        if GN_SEEDS[key] == 0:
            del GN_SEEDS[key]
    print('GN_SEEDS = {%s}' % ', '.join('%r: %d' % kv for kv in sorted(GN_SEEDS.items())))


if __name__ == '__main__':
    import sys
    torch.set_num_threads(1)
    if sys.argv[1:] == ['seeds']:
        choose_seeds()
    else:
        measure_baselines()
