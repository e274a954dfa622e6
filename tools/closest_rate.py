"""What closest_points costs (rp_closest_points; DESIGN.md section 4, profiles/closest_points_rate.txt): collider pairs per second on the headline id at N = 4096 with the
arm-against-scene pair list - every arm-link collider against every collider that is not the arm's, one group per link - with and without max_distance = 0.05.
The envs are first stepped with seeded random actions so that the arms are not all in one pose.  Device events around --calls back-to-back calls after a warm-up,
--repeats times; the median.  A call is two launches (k_collider_poses_rows, k_closest_points); the poses' share is measured by a call with one pair.
usage: python tools/closest_rate.py [env_id] [--n N] [--calls C] [--repeats R] [--steps S] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roboticsplayroompybullet_amd import VecPlayEnv  # noqa: E402

LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])


def timed(fn, calls, repeats, warmup=3):
    """milliseconds per call of `calls` back-to-back calls of fn, `repeats` times"""
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / calls)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('env_id', nargs='?', default='UR5PlayAbsRPY1Obj-v0')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    env = VecPlayEnv(args.env_id, args.n, seed=1)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(args.steps):
        env.step(torch.tensor(LO + (HI - LO) * rng.random((args.n, 7)), dtype=torch.float32, device=env.device))
    names = env.collider_names
    arm = [c for c, nm in enumerate(names) if nm.startswith('link')]
    scene = [c for c in range(len(names)) if c not in arm]
    pairs = torch.cat([env.collider_pairs(a, scene, group=g) for g, a in enumerate(arm)])
    k, groups = int(pairs.shape[0]), len(arm)
    out = env.closest_points(pairs, n_groups=groups)      # (the output tensors are made once: the timed calls allocate nothing)
    lines = ['closest_points on %s, N = %d: %d arm-link colliders x %d scene colliders = %d pairs per env, %d groups (%s)'
             % (args.env_id, args.n, len(arm), len(scene), k, groups, env.lib.rp_version().decode())]
    one = statistics.median(timed(lambda: env.closest_points(pairs[:1], out=None), args.calls, args.repeats))
    lines.append('  one pair per env (the pose pass and a launch):      %8.3f ms per call' % one)
    for label, cut in (('no cut', None), ('max_distance = 0.05', 0.05)):
        ms = timed(lambda: env.closest_points(pairs, max_distance=cut, n_groups=groups, out=out), args.calls, args.repeats)
        med = statistics.median(ms)
        st = out['status']
        far = float(((st & 3) == 2).float().mean())
        capped = int(((st & 4) != 0).sum())
        lines.append('  %-22s %8.3f ms per call (min %.3f, max %.3f of %d x %d calls): %.3e pairs/s; FAR %.1f %%, CAPPED %d, overlapping %.2f %%'
                     % (label + ':', med, min(ms), max(ms), args.repeats, args.calls, args.n * k / (med * 1e-3), 100 * far, capped,
                        100 * float(((st & 3) == 1).float().mean())))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
