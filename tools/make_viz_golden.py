"""Write tests/golden/viz.pt: the REFERENCE's viz_inv_depth for the depth-output cases of tests/depth_output_cases.py.

    python tools/make_viz_golden.py

Runs on the CPU where a reference checkout is present; loads it through oracle._refstubs (imports only, nothing is copied).  The
fixture holds data only: matplotlib's 256 x 3 float64 plasma table, the made-up 10-row table of case 8, per case the reference's own
output reduced to colour-table indices (uint8 [B,H,W]; the reduction is by EXACT row match, and the tables' rows are distinct --
asserted here) and a bit-pattern checksum of each input, which the tests rebuild from the same integer hash."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'packnet-sfm_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def to_indices(picture, table):
    """[H,W,3] float64 colours -> uint8 [H,W] rows of `table`; every pixel must equal exactly one row."""
    match = (picture[:, :, None, :] == table[None, None]).all(-1)
    assert (match.sum(-1) == 1).all(), 'a pixel of the reference output matches no row, or several rows, of the colour table'
    return torch.from_numpy(match.argmax(-1).astype(np.uint8))


def main():
    import depth_output_cases as C               # our package first: the input builders live next to the tests
    inputs = {name: C.viz_input(name) for name in C.INPUTS}
    table10 = C.table10()
    for name in [n for n in sys.modules if n == 'packnet_sfm' or n.startswith('packnet_sfm.')]:
        del sys.modules[name]                    # ... then the reference's package of the same name
    sys.path.remove(os.path.join(ROOT, 'packnet-sfm_amd'))
    from oracle import _refstubs
    _refstubs.install()
    import matplotlib
    from matplotlib.colors import ListedColormap
    from packnet_sfm.utils import depth as RD
    assert RD.__file__.startswith(_refstubs.REFERENCE), RD.__file__
    plasma = matplotlib.colormaps['plasma']
    tables = {'plasma': plasma(np.arange(plasma.N))[:, :3].astype(np.float64), 'table10': table10.astype(np.float64)}
    assert tables['plasma'].shape == (256, 3)
    for name, t in tables.items():
        assert len({row.tobytes() for row in t}) == len(t), '%s: rows are not distinct' % name
        assert len({row.tobytes() for row in np.rint(t * 255)}) == len(t), '%s: byte rows are not distinct' % name
    matplotlib.colormaps.register(ListedColormap(table10, name='pnsfm_table10'))
    names = {'plasma': 'plasma', 'table10': 'pnsfm_table10'}
    fx = {'plasma': torch.from_numpy(tables['plasma']), 'table10': torch.from_numpy(tables['table10']), 'index': {},
          'checksums': {name: C.checksum(t) for name, t in inputs.items()}, 'numpy': np.__version__, 'matplotlib': matplotlib.__version__}
    for sub in C.SUBS:
        inv = inputs[sub.input]
        rows = []
        for b in range(inv.shape[0]):
            pic = RD.viz_inv_depth(inv[b].float().clone(), normalizer=sub.normalizer, percentile=sub.percentile,
                                   colormap=names[sub.table], filter_zeros=sub.filter_zeros)      # the function divides its input in place
            assert pic.shape == tuple(inv.shape[2:]) + (3,) and pic.dtype == np.float64
            rows.append(to_indices(pic, tables[sub.table]))
        fx['index'][sub.key] = torch.stack(rows)
        print(sub.key, tuple(fx['index'][sub.key].shape), 'indices', int(fx['index'][sub.key].min()), '..', int(fx['index'][sub.key].max()))
    out = os.path.join(ROOT, 'tests', 'golden', 'viz.pt')
    torch.save(fx, out)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
