"""The Python face of the conv tuning ABI: pnsfm_tune_key / pnsfm_tune_set / pnsfm_conv2d_last_config (include/pnsfm.h).

Tests and the lab tools under tools/ pin launch configurations the un-tuned heuristics would not pick and read back what ran.
The KEY of a launch always comes from the library (key(): the function the launch itself calls), never from arithmetic here; the
two ints of a DECISION are laid out by the codec table of csrc/conv2d.hip (ConvDecision / WgradDecision), of which the two classes
below are the one Python copy, field for field.
"""
import collections
import contextlib
import ctypes
import os

from . import _lib, ops

FORWARD, BACKWARD_DATA, WGRAD = 0, 1, 2
SHIPPED_DB = os.path.join(_lib._CSRC, 'tuned_gfx950.db')


def key(kind, B, Cin, Cout, H, W, ks, stride=1, sources=1, lib=None):
    """The 7-int key under which the launch looks its decision up, under the arithmetic mode in force.  kind: FORWARD, BACKWARD_DATA
    or WGRAD; H, W: the OUTPUT map (y / dY); Cin, Cout: K and M of the launch (backward-data: K = channels of dY); sources: 1..3 input
    tensors.  Raises HipError for a shape the launch would refuse.  lib: a library handle of the caller's own (the trace builds of
    tools/) instead of the loaded one."""
    out = (ctypes.c_int * 7)()
    _lib.check((lib or _lib.get()).pnsfm_tune_key(kind, B, Cin, Cout, H, W, ks, stride, sources, out), 'tune_key')
    return tuple(out)


def key_rows(kind, B, Cin, Cout, H, Hi, W, ks, lib=None):
    """The key of a row-window launch (ops.conv2d_*_rows): B the whole batch of strips, H the rows the launch tiles (y / dx / dY),
    Hi the rows of the map it reads (x / dY / x).  Differs from key() of the same shape in key[0] (+ 10000 * Hi)."""
    out = (ctypes.c_int * 7)()
    _lib.check((lib or _lib.get()).pnsfm_tune_key_rows(kind, B, Cin, Cout, H, Hi, W, ks, out), 'tune_key_rows')
    return tuple(out)


class ConvDecision(collections.namedtuple('ConvDecision', 'NT variant narrow_m tile_mode split')):
    """Forward / backward-data: NT 1 | 2 32-pixel tiles per wave; variant 0..8 the kernel; narrow_m 1: 32-row M tiles where 64 would
    fit; tile_mode 0 | 1 | 2 | 3 classic tiles, 16-wide rectangles, row bands, short-map rectangles (maps of < 4 rows); split: K-split."""
    __slots__ = ()

    def __new__(cls, NT=1, variant=0, narrow_m=0, tile_mode=0, split=1):
        return super().__new__(cls, NT, variant, narrow_m, tile_mode, split)

    def encode(self):
        return (self.NT | (self.variant << 4) | (self.narrow_m << 8) | (self.tile_mode << 9), self.split)

    @classmethod
    def decode(cls, v0, v1):
        return cls(v0 & 15, (v0 >> 4) & 15, (v0 >> 8) & 1, (v0 >> 9) & 3, v1)


class WgradDecision(collections.namedtuple('WgradDecision', 'kernel split NT wm WCI TG TR')):
    """Weight gradient: kernel 0 generic f32 (the stem's own where it applies), 1 tap-major, 2 split-bf16 (NT 1 | 2 ci tiles per wave;
    wm: co tiles per workgroup, 0 the most, + 8 the three-workgroups build), 3 nine-taps (WCI 1 | 2 ci tiles per workgroup; TG, TR:
    tile width in 8-pixel groups / rows, 0 the library's choice); split: pixel split.  Fields of another kernel are not encoded."""
    __slots__ = ()

    def __new__(cls, kernel=0, split=1, NT=1, wm=0, WCI=2, TG=0, TR=0):
        return super().__new__(cls, kernel, split, NT, wm, WCI, TG, TR)

    def encode(self):
        if self.kernel == 2:
            return (self.split, 2 | (self.NT << 4) | (self.wm << 6))
        if self.kernel == 3:
            return (self.split, 3 | ((self.WCI | (self.TG << 4) | (self.TR << 8)) << 4))
        return (self.split, self.kernel)

    @classmethod
    def decode(cls, v0, v1):
        kernel = v1 & 15
        if kernel == 2:
            return cls(2, v0, NT=2 if ((v1 >> 4) & 3) == 2 else 1, wm=(v1 >> 6) & 15)
        if kernel == 3:
            return cls(3, v0, WCI=(v1 >> 4) & 15, TG=(v1 >> 8) & 15, TR=(v1 >> 12) & 15)
        return cls(kernel, v0)


def kind_fields(kind):
    """key[0] of a database line -> (FORWARD | BACKWARD_DATA | WGRAD, stride, split-bf16 arithmetic, several input tensors).
    (A row-window launch adds 10000 * Hi: rows_of.)"""
    return kind % 10, kind // 10 % 10, kind // 100 % 10 == 1, kind // 1000 % 10 == 1


def rows_of(kind):
    """Rows of the map a row-window launch reads (key_rows), 0 for every other launch."""
    return kind // 10000


def decode(kind, v0, v1):
    """The decision of a database line / a pnsfm_tune_set call from the key's kind (x2: weight gradient)."""
    return (WgradDecision if kind % 10 == WGRAD else ConvDecision).decode(v0, v1)


def pin(key7, decision, lib=None):
    """pnsfm_tune_set: the launches of key7 run `decision` until unpin() (or any call of the two pnsfm_set_*_variant setters)."""
    v0, v1 = decision.encode()
    _lib.check((lib or _lib.get()).pnsfm_tune_set((ctypes.c_int * 7)(*key7), v0, v1), 'tune_set')


def unpin():
    """Drop every pin and restore the library's un-tuned default kernels (the calls of conftest.py's `emulated_kernels`)."""
    lib = _lib.get()
    lib.pnsfm_set_conv_variant(0)
    lib.pnsfm_set_conv_variant(3)
    lib.pnsfm_set_wgrad_variant(-1)


@contextlib.contextmanager
def pinned(*pins):
    """`with pinned((key, decision), ...):` -- the launches inside run the pinned decisions.  On exit, also on an exception, ALL
    pins are dropped and the un-tuned defaults restored (unpin): not nestable, and a pnsfm_set_conv_variant / pnsfm_set_wgrad_variant
    call inside the block drops the pins too (switch an un-tuned default BEFORE entering)."""
    try:
        for k, d in pins:
            pin(k, d)
        yield
    finally:
        unpin()


class LastConfig(dict):
    """pnsfm_conv2d_last_config by name.  `raw`: the eight ints; `build`: the kernel build a weight-gradient launch ran --
    (103, KS, NT, WM, TC, masked, OCC) | (104, WCI, TG, TR, masked) | (100, stride, MT, tile mode) | (102,) | (105, MT) -- and
    (variant, MT, NT, G) after a forward / backward-data launch (G: taps per weight stage, 0 for the f32 kernels).
    Every layout has variant (the code 100..105 after a weight-gradient launch), split, blocks, lds; forward / backward-data adds
    NT, MT, G, tm; 100 stride, MT, PT, tm; 103 NT, WM, TC, OCC, masked, KS; 104 WCI, TG, TR, masked; 105 MT."""

    def __init__(self, c):
        code = c[0]
        super().__init__(variant=code, split=c[4], blocks=c[6], lds=c[7])
        self.raw = list(c)
        self.build = (code,)
        if code == 100:
            self.update(stride=c[1], MT=c[2], PT=c[3], tm=c[5])
            self.build = (100, c[1], c[2], c[5])
        elif code == 103:
            self.update(NT=c[1], WM=c[2], TC=c[3], OCC=c[5] & 15, masked=(c[5] >> 4) & 1, KS=c[5] >> 8)
            self.build = (103, c[5] >> 8, c[1], c[2], c[3], (c[5] >> 4) & 1, c[5] & 15)
        elif code == 104:
            self.update(WCI=c[1], TG=c[2], TR=c[3], masked=(c[5] >> 4) & 1)
            self.build = (104, c[1], c[2], c[3], (c[5] >> 4) & 1)
        elif code == 105:
            self.update(MT=c[2])
            self.build = (105, c[2])
        elif code < 100:
            self.update(NT=c[1], MT=c[2], G=c[3], tm=c[5])
            self.build = (code, c[2], c[1], c[3])


def last_config():
    """What the calling thread's most recent conv launch ran (ops.conv2d_last_config), by name."""
    return LastConfig(ops.conv2d_last_config())


def database_lines(path=SHIPPED_DB):
    """[(line text, [kind, B, K, M, H, W, ks, v0, v1])] of every data line of a tuning database, in file order."""
    out = []
    with open(path) as f:
        for raw in f:
            text = ' '.join(raw.split())
            if not text or text.startswith('#'):
                continue
            vals = [int(t) for t in text.split()]
            assert len(vals) == 9, 'malformed database line: %r' % raw
            out.append((text, vals))
    return out
