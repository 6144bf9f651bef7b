"""Write tests/golden/eval.pt: the REFERENCE's outputs for the depth-evaluation cases of tests/depth_eval_cases.py.

    python tools/make_eval_golden.py

Runs on the CPU where a reference checkout is present; loads it through oracle._refstubs (imports only, nothing is copied).  The
fixture holds data only: the post-process inputs ([2,1,8,64]) with the reference's post_process_inv_depth for mean / max / min, the
reference's compute_depth_metrics for metric cases 2-5 (case 1 is tests/golden/slim.pt['host']['metrics']) and a bit-pattern checksum
of each case's inputs, which the tests rebuild from the same integer hash."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'packnet-sfm_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    import depth_eval_cases as C                 # our package first: the input builders use packnet_sfm.utils.depth
    inputs = {case: C.metric_inputs(case) for case in (2, 3, 4, 5)}
    pp_in = C.pp_inputs()
    for name in [n for n in sys.modules if n == 'packnet_sfm' or n.startswith('packnet_sfm.')]:
        del sys.modules[name]                    # ... then the reference's package of the same name
    sys.path.remove(os.path.join(ROOT, 'packnet-sfm_amd'))
    from oracle import _refstubs
    _refstubs.install()
    from packnet_sfm.utils import depth as RD
    assert RD.__file__.startswith(_refstubs.REFERENCE), RD.__file__
    fx = {'post_process': {'inv_depth': pp_in[0], 'inv_depth_flipped': pp_in[1],
                           'out': {m: RD.post_process_inv_depth(pp_in[0], pp_in[1], method=m) for m in ('mean', 'max', 'min')}},
          'metrics': {}, 'checksums': {}}
    for case, (gt, pred, configs) in inputs.items():
        fx['checksums'][case] = C.checksum(gt, pred)
        for ugs in (False, True):
            fx['metrics'][(case, ugs)] = RD.compute_depth_metrics(configs[0], gt.float(), pred.float(), ugs)
            print(case, ugs, fx['metrics'][(case, ugs)].tolist())
    out = os.path.join(ROOT, 'tests', 'golden', 'eval.pt')
    torch.save(fx, out)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
