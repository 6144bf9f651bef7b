"""Write tests/golden/depth_input.pt: the REFERENCE's resize_depth_preserve / crop_depth outputs for PRESERVE_CASES of
tests/depth_input_cases.py.

    python tools/make_depth_input_golden.py

Runs on the CPU where a reference checkout is present; loads it through oracle._refstubs (imports only, nothing is copied).  The
fixture holds data only: per case the reference's output as fp32 [N,1,H,W] (its float64 array holds fp32 values, so the cast is exact
-- asserted), for the windowed case also the reference's crop_depth, and a bit-pattern checksum of each input, which the tests rebuild
from the same integer hash."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import depth_input_cases as C
    inputs = {name: C.preserve_inputs(name) for name in C.PRESERVE_CASES}
    from oracle import _refstubs
    _refstubs.install()
    import PIL.Image
    if not hasattr(PIL.Image, 'ANTIALIAS'):          # removed in Pillow 10; a default argument of the reference's resize_image
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
    assert not any(n == 'packnet_sfm' or n.startswith('packnet_sfm.') for n in sys.modules), 'the project package is already imported'
    from packnet_sfm.datasets import augmentations as RA
    assert RA.__file__.startswith(_refstubs.REFERENCE), RA.__file__
    fx = {'preserve': {}, 'crop': {}, 'checksums': {}}
    for name, (maps, window, shape) in inputs.items():
        fx['checksums'][name] = C.checksum(maps)
        outs = []
        for m in maps:
            if window is not None:
                y0, x0, h, w = window
                m = RA.crop_depth(m, (x0, y0, x0 + w, y0 + h))          # (left, top, right, bottom)
                fx['crop'][name] = torch.from_numpy(np.ascontiguousarray(m))[None]
            r = RA.resize_depth_preserve(m, shape)
            assert r.shape == tuple(shape) + (1,) and np.array_equal(r.astype(np.float32).astype(r.dtype), r), name
            outs.append(r[:, :, 0].astype(np.float32))
        fx['preserve'][name] = torch.from_numpy(np.stack(outs))[:, None]
        print(name, tuple(fx['preserve'][name].shape), 'non-zero cells:', int((fx['preserve'][name] != 0).sum()))
    out = os.path.join(ROOT, 'tests', 'golden', 'depth_input.pt')
    torch.save(fx, out)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
