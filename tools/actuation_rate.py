"""rp_step's time with the per-env actuation table (profiles/actuation_rate.txt): ms per step at N = 4096 on the headline id, with the default
table ((0, 0, -9.8), gains 1, strengths 1) and, with --random, every env's own row (gravity tilted by up to 3 m/s^2 in x and y and scaled by up to 2 in z, gains
0.5 .. 1.5, strengths 0.3 .. 1.2): a different workload.  Device events around --steps steps, --repeats times after a warm-up; prints one line per repeat,
the median and, with --timers, the per-launch timers of the last steps.  Runs on a tree without set_actuation too (then --random is refused): the job that
alternates old and new builds runs this same file in both.
usage: python tools/actuation_rate.py [env_id] [--n N] [--steps K] [--repeats R] [--random] [--timers]"""
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
    ap.add_argument('--random', action='store_true', help="every env its own gravity, motor gains and motor strengths")
    ap.add_argument('--timers', action='store_true', help='print the per-launch timers of the last 64 steps')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    env = VecPlayEnv(args.env_id, args.n, seed=0)
    if args.random:
        if not hasattr(env, 'set_actuation'):
            sys.exit('this build has no actuation table')
        na = len(env.actuation_names['motor'])
        g = torch.Generator().manual_seed(1)
        grav = torch.tensor([0.0, 0.0, -9.8]) + torch.tensor([3.0, 3.0, 2.0]) * (2 * torch.rand((args.n, 3), generator=g) - 1)
        env.set_actuation(gravity=grav.to(dev), motor_gain=(0.5 + torch.rand((args.n, na), generator=g)).to(dev),
                          motor_strength=(0.3 + 0.9 * torch.rand((args.n, na), generator=g)).to(dev))
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
    tag = args.label or ('random' if args.random else 'default')
    print('%-10s %s N=%d  ms/step per repeat: %s  median %.4f  spread %.4f' % (tag, args.env_id, args.n, ' '.join('%.4f' % x for x in ms),
                                                                      float(np.median(ms)), max(ms) - min(ms)))
    if args.timers:
        env.enable_timers(64)
        for i in range(64):
            env.step(a[args.warmup + i % args.steps])
        torch.cuda.synchronize()
        print('%-10s per-launch timers: %s' % (tag, ' '.join('%s=%.4g' % kv for kv in env.timers().items())))
    env.close()


if __name__ == '__main__':
    main()
