#!/usr/bin/env python3
"""Records tests/golden/gen_batch_rig0.npz: what raygen.generate_batch (durf_gen_batch) returns, bit for bit, on the seeded
three-camera rig of tests/test_gpu_data.py -- the full images in order (ray_idx = None) and a random batch of 777 pixel
indices.  Recorded ONCE on an MI355X from the commit BEFORE the pinhole body of k_gen_batch was factored out into
csrc/pinhole.h (now csrc/camera.h; the device function k_camera_rays shares with it): tests/test_gpu_trajectory.py holds every later build
to these bits, so "durf_gen_batch stays bit-identical" is checked against the old kernel and not against itself.

    python tests/golden/make_gen_batch_fixture.py [OUT.npz]        (needs the GPU; do not re-record to make a test pass)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from durf_amd import raygen  # noqa: E402
from tests import test_gpu_data as TD  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'gen_batch_rig0.npz')
FIELDS = ('origins', 'directions', 'viewdirs', 'radii', 'lossmult', 'near', 'far')
NEAR, FAR, SEED_RIG, SEED_IDX, N_IDX = 0.0, 40.0, 0, 1, 777


def rig_and_indices():
    h, w, focal, pp, c2w, images, depth, sky = TD._rig(SEED_RIG)
    idx = np.random.default_rng(SEED_IDX).integers(0, int((h * w).sum()), N_IDX).astype(np.int32)
    return (h, w, focal, pp, c2w, images, depth, sky), idx


def run(dev):
    """-> {name: ndarray} of both calls (the test runs this too and compares)"""
    (h, w, focal, pp, c2w, images, depth, sky), idx = rig_and_indices()
    ts = raygen.TimestepData(c2w, focal, pp, h, w, images, depth, sky, device=dev)
    out = {}
    for tag, ri in (('full', None), ('batch', torch.tensor(idx, device=dev))):
        rays, px, dp, sk = raygen.generate_batch(ts, ri, NEAR, FAR)
        for name in FIELDS:
            out['%s_%s' % (tag, name)] = getattr(rays, name).cpu().numpy()
        out[tag + '_pixels'], out[tag + '_depth'], out[tag + '_sky'] = px.cpu().numpy(), dp.cpu().numpy(), sk.cpu().numpy()
    return out


if __name__ == '__main__':
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **run(torch.device('cuda:0')))
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
