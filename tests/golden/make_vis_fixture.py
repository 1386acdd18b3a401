#!/usr/bin/env python3
"""Records tests/golden/ref_vis_cases.npz: what the reference's own internal/vis.py -- imported UNMODIFIED -- returns in
float64 on the small test planes of tests/vis_ref.py, plus those planes and matplotlib's turbo table.  The reference needs
jax; three stand-ins are installed before the import, none of which touches its arithmetic:
    jax.numpy                    -> numpy
    jax.scipy.signal.convolve2d  -> scipy.signal.convolve2d (the `precision` keyword dropped)
    matplotlib.cm.get_cmap       -> matplotlib.colormaps.__getitem__ (matplotlib 3.9 removed get_cmap)
tests/test_vis_host.py holds the float64 restatement (tests/vis_ref.py) to these numbers; the GPU tests are held to the
restatement.  Data only: inputs, outputs, a colour table.

    python tests/golden/make_vis_fixture.py REFERENCE_ROOT [OUT.npz]      (no GPU; needs scipy and matplotlib)"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import vis_ref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ref_vis_cases.npz')
SMALL = ('p1x1', 'p1x7', 'p7x1', 'p3x3', 'p37x53', 'nan_acc0', 'nan_noacc', 'const')
NEAR_FAR = (0.5, 45.0)


def import_reference_vis(ref_root):
    import matplotlib
    import matplotlib.cm
    import scipy.signal
    jax = types.ModuleType('jax')
    jax.numpy = np
    jax.lax = types.SimpleNamespace(Precision=types.SimpleNamespace(HIGHEST=None))
    jsp = types.ModuleType('jax.scipy')
    jsp.signal = types.SimpleNamespace(convolve2d=lambda z, f, mode='full', precision=None: scipy.signal.convolve2d(z, f, mode=mode))
    jax.scipy = jsp
    sys.modules.update({'jax': jax, 'jax.numpy': np, 'jax.scipy': jsp})
    if not hasattr(matplotlib.cm, 'get_cmap'):
        matplotlib.cm.get_cmap = matplotlib.colormaps.__getitem__
    spec = importlib.util.spec_from_file_location('reference_vis', os.path.join(ref_root, 'internal', 'vis.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(ref_root):
    import matplotlib
    V = import_reference_vis(ref_root)
    out = {'turbo': np.asarray(matplotlib.colormaps['turbo'](np.arange(256))[:, :3], np.float64)}
    h = np.linspace(-1.5, 2.5, 41)
    out['sinebow_h'], out['sinebow'] = h, V.sinebow(h)
    with np.errstate(all='ignore'):
        for name in SMALL:
            depth, acc = vis_ref.case(name)
            out[name + '/depth'] = depth
            if acc is not None:
                out[name + '/acc'] = acc
            d = depth[0].astype(np.float64)
            a = None if acc is None else acc[0].astype(np.float64)
            out[name + '/normals_raw'] = V.depth_to_normals(d)
            out[name + '/normals'] = V.visualize_normals(d, a)
            out[name + '/depth_mod'] = V.visualize_depth(d, a, modulus=0.1)
            out[name + '/depth_given'] = V.visualize_depth(d, a, near=NEAR_FAR[0], far=NEAR_FAR[1])
            out[name + '/depth_auto'] = V.visualize_depth(d, a)
            if name == 'p3x3':
                out[name + '/normals_s2'] = V.visualize_normals(d, a, scaling=2.0)
                suite = V.visualize_suite(d, a)
                for k in suite:
                    out[name + '/suite_' + k] = suite[k]
            if name == 'p37x53':
                out[name + '/depth_flipped_identity'] = V.visualize_depth(d, a, near=30.0, far=5.0, curve_fn=lambda x: x)
                out[name + '/depth_inverse'] = V.visualize_depth(d, a, curve_fn=lambda x: 1 / (x + np.finfo(np.float32).eps))
                out[name + '/depth_ignore'] = V.visualize_depth(d, a, ignore_frac=0.05)
                out[name + '/depth_far_only'] = V.visualize_depth(d, a, near=0, far=45.0)
    return out


if __name__ == '__main__':
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    np.savez_compressed(path, **record(sys.argv[1]))
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
