"""Step time of dynamics=False training with box-pose optimisation versus frozen poses (4096 x 128 x 2, K = 3 by default):
python tools/time_static_pose.py [--rays 4096] [--samples 128] [--K 3] [--steps 20] [--warmup 5] [--precision bf16]
Prints one JSON line per mode: median / mean ms per train_step from HIP events (the same batch every step)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from durf_amd import obbpose_model, synthetic, train_boxpose, utils  # noqa: E402
from tests import helpers as H  # noqa: E402


def run(pose_opt, a):
    dev = torch.device('cuda:0')
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.dynamics = False\nMipNerfModel.mlp_precision = "%s"\n'
                    'MipNerfModel.no_pose_opt = %s\nMipNerfModel.no_yaw_opt = %s\nConfig.tv_loss_mult = 0.01\n'
                    % (a.samples, a.precision, not pose_opt, not pose_opt))
    config = utils.configured(utils.Config)
    b = synthetic.make_batch(a.rays, a.K, seed=7, noise_boxes=0.05)
    db = H.device_batch(b, dev)
    model, variables = obbpose_model.construct_mipnerf(7, db, device=dev)
    state = train_boxpose.create_train_state(variables)
    prev = db['init'][0:1] + 0.01
    times = []
    for i in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        state, stats, _, _ = train_boxpose.train_step(model, config, i, state, db, 5e-4, 3.0, 10.0, prev)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    print(json.dumps(dict(mode='pose_opt' if pose_opt else 'frozen', rays=a.rays, samples=a.samples, K=a.K,
                          precision=a.precision, ms_median=times[len(times) // 2], ms_mean=sum(times) / len(times),
                          loss=float(stats.loss))), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rays', type=int, default=4096)
    p.add_argument('--samples', type=int, default=128)
    p.add_argument('--K', type=int, default=3)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--precision', default='bf16')
    p.add_argument('--only', choices=['pose_opt', 'frozen'], default=None)
    a = p.parse_args()
    for pose_opt in (False, True):
        if a.only is None or a.only == ('pose_opt' if pose_opt else 'frozen'):
            run(pose_opt, a)


if __name__ == '__main__':
    main()
