"""Drop-in boundary (packnet_sfm/_merge.py) against a stand-in checkout written by this test.

`PYTHONPATH=<repo>/packnet-sfm_amd:<checkout>` must give ONE `packnet_sfm` package: modules this repository re-implements
resolve here, modules only the checkout has resolve there, a shadowing module serves the names it does not define from the
checkout's file of the same path, and `import horovod.torch` lands on the RCCL facade.  The stand-in holds a few lines of
this test's own, laid out like a packnet_sfm checkout.  CPU, no kernels launched; each scenario is a fresh interpreter so
that sys.path order, not this pytest process's import state, decides.
"""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'packnet-sfm_amd')

STAND_IN = {
    'packnet_sfm/__init__.py': '',
    'packnet_sfm/utils/__init__.py': '',
    'packnet_sfm/utils/load.py': '''
        import importlib
        def load_class(name, paths):
            return getattr(importlib.import_module(paths[0] + '.' + name), name)
    ''',
    'packnet_sfm/utils/depth.py': '''
        def viz_inv_depth(x):
            return 'stand-in viz_inv_depth'
        def inv2depth(x):
            return 'stand-in inv2depth'
    ''',
    'packnet_sfm/networks/__init__.py': '',
    'packnet_sfm/networks/depth/__init__.py': '',
    'packnet_sfm/networks/depth/PackNet01.py': '''
        class PackNet01:
            stand_in = True
    ''',
}


def _checkout(tmp_path):
    for rel, src in STAND_IN.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    return str(tmp_path)


def _run(code, pythonpath):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath), PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, 'child failed:\nSTDOUT:\n%s\nSTDERR:\n%s' % (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_merged_package_resolves_each_module_in_the_right_tree(tmp_path):
    ref = _checkout(tmp_path)
    out = _run('''
        import packnet_sfm.utils.load as L, packnet_sfm.networks.depth.PackNet01 as PN, packnet_sfm.utils.depth as D
        print('load', L.__file__); print('ours', PN.__file__); print('ours', D.__file__)
        cls = L.load_class('PackNet01', ['packnet_sfm.networks.depth'])
        print('plugin', cls.__module__, hasattr(cls, 'stand_in'))
        # a name the shadowing module does not define comes from the checkout's file; a name it defines stays ours
        from packnet_sfm.utils.depth import viz_inv_depth, inv2depth
        print('fallback', viz_inv_depth.__module__, viz_inv_depth(0).replace(' ', '_'), inv2depth.__module__)
    ''', [PKG, ref])
    lines = [l.split(' ', 1) for l in out.strip().splitlines()]
    got = {k: v for k, v in lines if k != 'ours'}
    assert got['load'].startswith(ref)
    ours = [v for k, v in lines if k == 'ours']
    assert len(ours) == 2 and all(p.startswith(PKG) for p in ours), ours
    assert got['plugin'] == 'packnet_sfm.networks.depth.PackNet01 False'
    fb = got['fallback'].split()
    assert fb == ['packnet_sfm.utils.depth.__reference__', 'stand-in_viz_inv_depth', 'packnet_sfm.utils.depth'], fb


def test_without_a_checkout_the_fallback_names_what_is_missing():
    out = _run('''
        import packnet_sfm.utils.depth as D
        try:
            D.viz_inv_depth
        except AttributeError as e:
            print('missing', e)
    ''', [PKG])
    assert out.startswith('missing') and 'no reference checkout' in out, out


def test_horovod_imports_resolve_to_the_rccl_facade(tmp_path):
    out = _run('''
        import torch
        import horovod.torch as hvd
        import packnet_sfm.rccl.hvd as facade
        for name in ('init', 'rank', 'size', 'local_rank', 'allreduce', 'broadcast_parameters', 'DistributedOptimizer', 'Compression'):
            assert getattr(hvd, name) is getattr(facade, name), name
        assert hvd.Compression.none is None
        hvd.init()
        assert hvd.rank() == 0 and hvd.size() == 1
        print('OK')
    ''', [PKG, _checkout(tmp_path)])
    assert out.strip().splitlines()[-1] == 'OK'
