"""Depth-output cases (csrc/depth_output.h: colour-mapped inverse depth, 16-bit depth values; utils.depth.viz_inv_depth_u8 /
depth_png16) shared by the emulated CPU tests (tests/test_depth_output_emulated.py) and the GPU tests (tests/test_gpu_depth_output.py).

Inputs come from depth_eval_cases.uniform (an integer hash), so they are the same numbers on every machine and need no storage.  The
reference's own viz_inv_depth on them, reduced to colour-table indices by exact row match, is in tests/golden/viz.pt (written by
tools/make_viz_golden.py, which imports the input builders below) together with the 256 x 3 float64 plasma table, the made-up 10-row
table of case 8 and a bit-pattern checksum of every input.  Kernel tests pass the table from the fixture: they need neither
matplotlib nor a reference checkout.

EVERY comparison is exact (torch.equal / bit patterns); there is no tolerance in this feature.

  case  shape and inputs                                            what it catches
  1     1x1 and 1x2, percentile 95 and 100                          rank k+1 clamped to n-1; gamma = 0
  2     3x7 and 37x53, percentiles 0, 50, 95, 99.5                   odd sizes; both branches of the interpolation (asserted)
  3     19x27, values rounded to 1/16                               long runs of ties across the two ranks
  4     37x53, about 30 % zeros, filter_zeros on and off            n from the device count
  5     batch 2 of 96x320, images with different value ranges       several workgroups per image, per-image normalisers
  6     case 5's data, caller-supplied normaliser 0.7               the select skipped
  7     case 2's 37x53 map stored as fp16                           expected: the fp32 result on .float()
  8     case 4's data with a made-up 10-row table                   index = trunc(x N) and the N -> N-1 rule off the 256 path

Cases 1-8 compare `index` with the fixture and `out` with rint(table * 255)[index]; the normaliser with np.percentile on the host, bit
for bit (case 6: with float32(0.7))."""
import collections
import contextlib
import functools

import numpy as np
import pytest
import torch

import parity_cases as P
from depth_eval_cases import checksum, uniform
from packnet_sfm.hip import _lib
from packnet_sfm.hip import functional as HF
from packnet_sfm.hip import ops
from packnet_sfm.utils import depth as D

Sub = collections.namedtuple('Sub', 'key case input percentile filter_zeros normalizer table')


def _map(shape, seed, lo=0.02, hi=0.5):
    return (lo + (hi - lo) * uniform(shape, seed)).float()


@functools.lru_cache(maxsize=None)
def viz_input(name):
    """[B,1,H,W] inverse-depth maps on the CPU ('half': fp16)."""
    if name == '1x1':
        return _map((1, 1, 1, 1), 101)
    if name == '1x2':
        return _map((1, 1, 1, 2), 102)
    if name == '3x7':
        return _map((1, 1, 3, 7), 103)
    if name == '37x53':
        return _map((1, 1, 37, 53), 104)
    if name == 'ties':                      # 33 distinct values over 513 pixels
        return (torch.round(2.0 * uniform((1, 1, 19, 27), 105) * 16) / 16).float()
    if name == 'zeros':
        m = _map((1, 1, 37, 53), 106)
        m[uniform((1, 1, 37, 53), 107) < 0.3] = 0
        return m
    if name == 'batch':
        return torch.cat([_map((1, 1, 96, 320), 108), _map((1, 1, 96, 320), 109, 0.5, 3.0)])
    if name == 'half':
        return viz_input('37x53').half()
    raise KeyError(name)


INPUTS = ('1x1', '1x2', '3x7', '37x53', 'ties', 'zeros', 'batch', 'half')


def table10():
    """A made-up 10-row colour table, float64 in [0, 1] on a 1/64 grid; rows distinct (asserted by the fixture tool)."""
    return (torch.round(uniform((10, 3), 110) * 64) / 64).numpy()


def _subs():
    out = []
    for nm in ('1x1', '1x2'):
        out += [Sub('c1_%s_p%g' % (nm, p), 1, nm, p, False, None, 'plasma') for p in (95, 100)]
    for nm in ('3x7', '37x53'):
        out += [Sub('c2_%s_p%g' % (nm, p), 2, nm, p, False, None, 'plasma') for p in (0, 50, 95, 99.5)]
    out += [Sub('c3_p%g' % p, 3, 'ties', p, False, None, 'plasma') for p in (50, 95)]
    out += [Sub('c4_fz%d' % fz, 4, 'zeros', 95, bool(fz), None, 'plasma') for fz in (0, 1)]
    out.append(Sub('c5', 5, 'batch', 95, False, None, 'plasma'))
    out.append(Sub('c6', 6, 'batch', 95, False, 0.7, 'plasma'))
    out += [Sub('c7_p%g' % p, 7, 'half', p, False, None, 'plasma') for p in (0, 50, 95, 99.5)]
    out += [Sub('c8_fz%d' % fz, 8, 'zeros', 95, bool(fz), None, 'table10') for fz in (0, 1)]
    return out


SUBS = _subs()
SUB_KEYS = [s.key for s in SUBS]
BY_KEY = {s.key: s for s in SUBS}


def fixture():
    return P.golden('viz')


def table(name):
    """The float64 [N,3] table `name` of the fixture."""
    fx = fixture()
    t = fx[name].numpy()
    if name == 'table10':
        assert np.array_equal(t, table10())
    return t


def lut8_of(tab):
    return torch.from_numpy(np.rint(np.asarray(tab, np.float64) * 255).astype(np.uint8))


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def virtual_index(n, percentile):
    """np.percentile's float32 virtual index for n values (numpy 2.2, method 'linear')."""
    f = np.float32
    q = f(percentile) / f(100)
    return f(n - 1) * q


def host_normalizers(sub, inv):
    x = inv.float().numpy()[:, 0]
    if sub.normalizer is not None:
        return np.full((x.shape[0],), sub.normalizer, np.float32)
    return np.array([np.percentile(m[m > 0] if sub.filter_zeros else m, sub.percentile) for m in x], np.float32)


def viz_case(dev, key):
    sub, fx = BY_KEY[key], fixture()
    inv = viz_input(sub.input)
    assert checksum(inv) == fx['checksums'][sub.input], 'input %r differs from the one the fixture was recorded on' % sub.input
    tab = table(sub.table)
    lut8 = lut8_of(tab)
    assert torch.equal(D.colormap_lut8(tab, 'cpu'), lut8)
    out, index, norms = HF.viz_inv_depth_u8(inv.to(dev), lut8.to(dev), normalizer=sub.normalizer, percentile=sub.percentile,
                                            filter_zeros=sub.filter_zeros, details=True)
    B, _, H, W = inv.shape
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, 3) and index.dtype == torch.uint8 and tuple(index.shape) == (B, H, W)
    assert norms.dtype == torch.float32 and tuple(norms.shape) == (B,) and out.device == index.device == norms.device
    want = fx['index'][key]
    bad = (index.cpu() != want)
    assert not bool(bad.any()), '%s: %d of %d table indices differ from the reference (first at %s: %d, expected %d)' % (
        key, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), int(index.cpu()[bad][0]), int(want[bad][0]))
    assert torch.equal(out.cpu(), lut8[want.long()]), key + ': out != rint(table * 255)[index]'
    got, host = norms.cpu().numpy(), host_normalizers(sub, inv)
    assert np.array_equal(bits(got), bits(host)), '%s: normalisers %s, np.percentile %s' % (key, got.tolist(), host.tolist())
    plain = HF.viz_inv_depth_u8(inv.to(dev), lut8.to(dev), normalizer=sub.normalizer, percentile=sub.percentile, filter_zeros=sub.filter_zeros)
    assert torch.equal(plain, out), key + ': details=False'
    if sub.case == 7:                                   # fp16 storage == the fp32 kernels on the .float() copy
        o32, i32, n32 = HF.viz_inv_depth_u8(inv.float().to(dev), lut8.to(dev), percentile=sub.percentile, details=True)
        assert torch.equal(o32, out) and torch.equal(i32, index) and torch.equal(n32, norms), key
    if sub.case == 5:
        assert got[0] != got[1] and int(want[0].max()) == 255 and int(want[1].max()) == 255, 'case 5 wants per-image normalisers'
    return out, index, norms


def all_zero_case(dev):
    """filter_zeros on an all-zero image (second image of the batch: no leakage from the first): normaliser 0, every index 0."""
    inv = torch.cat([viz_input('3x7'), torch.zeros((1, 1, 3, 7))])
    lut8 = lut8_of(table('plasma'))
    out, index, norms = HF.viz_inv_depth_u8(inv.to(dev), lut8.to(dev), filter_zeros=True, details=True)
    assert float(norms[1]) == 0.0 and float(norms[0]) > 0.0
    assert not bool(index[1].any()) and bool(index[0].any())
    assert torch.equal(out[1].cpu(), lut8[0].expand(3, 7, 3))


def panel_inputs():
    u8 = (uniform((2, 8, 20, 3), 120) * 256).to(torch.uint8)
    u8.view(-1)[:4] = torch.tensor([0, 255, 1, 254], dtype=torch.uint8)
    return u8, _map((2, 1, 8, 20), 121)


def panel_case(dev, dtype):
    u8, inv = panel_inputs()
    rgb = (u8.permute(0, 3, 1, 2).float() / 255).to(dtype).contiguous()
    lut8 = lut8_of(table('plasma')).to(dev)
    for bgr in (False, True):
        out = HF.viz_inv_depth_u8(inv.to(dev), lut8, rgb=rgb.to(dev), bgr=bgr)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 16, 20, 3)
        assert torch.equal(out[:, :8].cpu(), u8.flip(3) if bgr else u8), 'frame half, bgr=%s %s' % (bgr, dtype)
        alone = HF.viz_inv_depth_u8(inv.to(dev), lut8, bgr=bgr)
        assert torch.equal(out[:, 8:], alone), 'picture half, bgr=%s %s' % (bgr, dtype)
        if bgr:
            assert torch.equal(alone, HF.viz_inv_depth_u8(inv.to(dev), lut8).flip(3))


def png16_input(dtype):
    m = _map((1, 1, 5, 9), 130, 0.001, 0.9)
    m.view(-1)[:5] = torch.tensor([0.0, 1e-7, 1 / 256, 1 / 255.99, 2.0])
    return m.to(dtype)


def png16_expected(inv):
    return (1 / inv.float().clamp(min=1e-6) * 256).int().clamp(max=65535)


def png16_case(dev, dtype, fn=None):
    inv = png16_input(dtype)
    out = (fn or HF.depth_png16)(inv.to(dev))
    assert out.dtype == torch.uint16 and tuple(out.shape) == tuple(inv.shape)
    want = png16_expected(inv)
    assert int(want.max()) == 65535 and int(want.min()) < 256          # saturation and sub-metre values are both in the map
    assert torch.equal(out.cpu().to(torch.int32), want), (out.cpu().to(torch.int32) - want).abs().max()
    return out


@contextlib.contextmanager
def product_loader_rules():
    """Inside: CPU tensors take the CPU-tensor path of packnet_sfm.utils.depth even while the emulator is loaded."""
    saved = _lib.REQUIRE_CUDA
    _lib.REQUIRE_CUDA = True
    try:
        yield
    finally:
        _lib.REQUIRE_CUDA = saved


def host_path(fn, *tensors, **kw):
    with product_loader_rules():
        return fn(*[t.cpu() if torch.is_tensor(t) else t for t in tensors], **kw)


def same(a, b):
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b)) and len(a) == len(b)


def public_case(dev):
    """utils.depth functions on device (or emulated) tensors == on CPU tensors == the fixture, case 4's data."""
    inv, tab = viz_input('zeros'), table('plasma')
    u8 = (uniform((1, 37, 53, 3), 122) * 256).to(torch.uint8)
    rgb = (u8.permute(0, 3, 1, 2).float() / 255).contiguous()
    for fz in (False, True):
        kw = dict(colormap=tab, filter_zeros=fz, details=True)
        got = D.viz_inv_depth_u8(inv.to(dev), **kw)
        assert same(got, host_path(D.viz_inv_depth_u8, inv, **kw)), 'filter_zeros=%s' % fz
        assert torch.equal(got[1].cpu(), fixture()['index']['c4_fz%d' % fz])
        kw.update(rgb=rgb, bgr=True, percentile=50)
        assert same(D.viz_inv_depth_u8(inv.to(dev), **dict(kw, rgb=rgb.to(dev))), host_path(D.viz_inv_depth_u8, inv, **kw))
        kw.update(normalizer=0.3)
        assert same(D.viz_inv_depth_u8(inv.to(dev), **dict(kw, rgb=rgb.to(dev))), host_path(D.viz_inv_depth_u8, inv, **kw))
    kw8 = dict(colormap=torch.from_numpy(table('table10')), filter_zeros=True, details=True)
    got = D.viz_inv_depth_u8(inv.to(dev), **kw8)
    assert same(got, host_path(D.viz_inv_depth_u8, inv, **kw8)) and torch.equal(got[1].cpu(), fixture()['index']['c8_fz1'])
    for dtype in (torch.float32, torch.float16):
        a = png16_case(dev, dtype, D.depth_png16)
        assert torch.equal(a.cpu().to(torch.int32), host_path(D.depth_png16, png16_input(dtype)).to(torch.int32))


def errors_case(dev):
    _, inv = panel_inputs()
    u8, _ = panel_inputs()
    rgb = (u8.permute(0, 3, 1, 2).float() / 255).contiguous().to(dev)
    inv = inv.to(dev)
    lut8 = lut8_of(table('plasma')).to(dev)
    with pytest.raises(RuntimeError):                   # mismatched rgb shape
        HF.viz_inv_depth_u8(inv, lut8, rgb=rgb[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        D.viz_inv_depth_u8(inv, rgb=rgb[:1], colormap=table('plasma'))
    for n in (0, 257):                                  # table with N = 0 or N = 257
        with pytest.raises(RuntimeError):
            HF.viz_inv_depth_u8(inv, torch.zeros((n, 3), dtype=torch.uint8, device=dev))
        with pytest.raises(ValueError):
            D.viz_inv_depth_u8(inv, colormap=np.zeros((n, 3)))
    for p in (101, -1):                                 # numpy's rule
        with pytest.raises(ValueError):
            HF.viz_inv_depth_u8(inv, lut8, percentile=p)
        with pytest.raises(ValueError):
            D.viz_inv_depth_u8(inv, colormap=table('plasma'), percentile=p)
    with pytest.raises(RuntimeError, match='2\\^24'):    # H W above 2^24: the shape alone, nothing is allocated
        ops.viz_inv_depth_check(1, 4097, 4096, 256, 95)
    ops.viz_inv_depth_check(1, 4096, 4096, 256, 95)
    lib = _lib.get()                                    # ... and the library's own error code, before it touches a pointer
    rc = lib.pnsfm_viz_inv_depth(None, 0, None, 0, None, 256, None, None, None, 1, 4097, 4096, 95.0, 0, 0, 0.0, 0, None)
    assert rc != 0 and b'2^24' in lib.pnsfm_last_error()
    rc = lib.pnsfm_viz_inv_depth(None, 0, None, 0, None, 256, None, None, None, 1, 8, 8, 101.0, 0, 0, 0.0, 0, None)
    assert rc != 0 and b'percentile' in lib.pnsfm_last_error()
    with pytest.raises(NotImplementedError):            # forward only
        HF.viz_inv_depth_u8(inv.clone().requires_grad_(True), lut8)
