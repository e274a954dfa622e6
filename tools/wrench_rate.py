"""rp_step's time with the per-env wrench table (profiles/wrench_rate.txt): ms per step at N = 4096 on the headline id, with the zero
table and, with --push, a non-zero force and torque on every body of every env (arm links up to 3 N / 0.3 N m, the other bodies up to 0.3 N / 0.003 N m).
Device events around --steps steps, --repeats times after a warm-up; prints one line per repeat and the median.  Runs on a tree without set_wrench too
(then --push is refused): the job that alternates old and new builds runs this same file in both.
usage: python tools/wrench_rate.py [env_id] [--n N] [--steps K] [--repeats R] [--push]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roboticsplayroompybullet_amd import VecPlayEnv  # noqa: E402

LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('env_id', nargs='?', default='UR5PlayAbsRPY1Obj-v0')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--push', action='store_true', help='a non-zero wrench on every body of every env')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    env = VecPlayEnv(args.env_id, args.n, seed=0)
    if args.push:
        if not hasattr(env, 'set_wrench'):
            sys.exit('this build has no wrench table')
        names = env.wrench_names
        g = torch.Generator().manual_seed(1)
        w = 2 * torch.rand((args.n, len(names), 6), generator=g) - 1
        w = torch.where(w.abs() < 1e-3, torch.full_like(w, 1e-3), w)
        mag = torch.tensor([[3.0] * 3 + [0.3] * 3 if nm.startswith('link') else [0.3] * 3 + [0.003] * 3 for nm in names])
        env.set_wrench((w * mag).to(dev))
    env.reset()
    rng = np.random.default_rng(0)
    a = torch.tensor(LO + (HI - LO) * rng.random((args.warmup + args.steps, args.n, 7)), dtype=torch.float32, device=dev)
    for i in range(args.warmup):
        env.step(a[i])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for r in range(args.repeats):
        torch.cuda.synchronize()
        t0.record()
        for i in range(args.steps):
            env.step(a[args.warmup + i])
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / args.steps)
    tag = args.label or ('push' if args.push else 'zero')
    print('%-10s %s N=%d  ms/step per repeat: %s  median %.4f  spread %.4f' % (tag, args.env_id, args.n, ' '.join('%.4f' % x for x in ms),
                                                                      float(np.median(ms)), max(ms) - min(ms)))
    env.close()


if __name__ == '__main__':
    main()
