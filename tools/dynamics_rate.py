"""rp_step's time with the per-env dynamics table (profiles/dynamics_rate.txt): ms per step at N = 4096 on the headline id, with the baked
values and, with --random, every env's friction and masses drawn anew (baked x U[0.25, 4]).  Device events around --steps steps, --repeats times after a
warm-up; prints one line per repeat and the median.  Runs on a tree without set_dynamics too (then --random is refused): the job that alternates old and
new builds runs this same file in both.
usage: python tools/dynamics_rate.py [env_id] [--n N] [--steps K] [--repeats R] [--random]"""
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
    ap.add_argument('--random', action='store_true', help='every env gets its own friction and masses')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    env = VecPlayEnv(args.env_id, args.n, seed=0)
    if args.random:
        if not hasattr(env, 'set_dynamics'):
            sys.exit('this build has no per-env dynamics')
        g = torch.Generator().manual_seed(1)
        d = env.get_dynamics()
        env.set_dynamics(**{k: (v.cpu() * (0.25 + 3.75 * torch.rand(v.shape, generator=g))).to(dev) for k, v in d.items()})
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
    tag = args.label or ('random' if args.random else 'baked')
    print('%-10s %s N=%d  ms/step per repeat: %s  median %.4f  spread %.4f' % (tag, args.env_id, args.n, ' '.join('%.4f' % x for x in ms),
                                                                      float(np.median(ms)), max(ms) - min(ms)))
    env.close()


if __name__ == '__main__':
    main()
