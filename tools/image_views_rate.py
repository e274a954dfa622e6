"""What two camera views per env inside the batched step cost on the GPU box (DESIGN.md "Several views per env", profiles/image_views_rate.txt): N = 4096 of
UR5PlayAbsRPY1Obj-v0 after 50 random steps, view 1 the fixed camera at 84 x 84 rgb, view 2 the gripper camera at 64 x 64 rgb + depth, one process per variant:

  obs+render          (a) the route before rp_set_image_views: set_image_obs for view 1, then per step `step` and render_layers for view 2 into preallocated tensors
                      - a second pose table and a second launch chain per step.  Uses nothing this feature added, so the same file times an older tree (--tree).
  views               (b) set_image_views, both views: one k_collider_poses and one k_render_views per pass
  views-per-view      (c) ... with rp_debug_image_views_merge(h, 0): one k_collider_poses, then a k_render_layers launch per view
  autoreset           (d) autoreset=True, max_episode_steps=200, counters staggered e % 200 (about N / 200 envs end in every step), both views with terminal frames:
                      the terminal pass over the ended envs, then the observation pass
  autoreset-per-view  (e) ... with the merge switched off

ms per step from device events around enough back-to-back steps for --window ms, warmed up, three timings, their median.  Each process appends its lines to --out;
`--summarize raw.txt` turns the lines of a job that ran every variant twice, alternated, into the table.  The bar a difference has to clear is the spread of (a) on
the older tree: the larger of the gap between its two processes and of the spread of the three timings inside a process.
usage: python tools/image_views_rate.py --variant views [--tree DIR] [--label NAME] [--out FILE] [--window 300] [--n 4096]
       python tools/image_views_rate.py --summarize FILE"""
import argparse
import collections
import os
import sys

import numpy as np

GID = 'UR5PlayAbsRPY1Obj-v0'
LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])
VARIANTS = ('obs+render', 'views', 'views-per-view', 'autoreset', 'autoreset-per-view')
LIMIT = 200
SHAPE = 'fixed 84 x 84 rgb + gripper 64 x 64 rgb, depth'


def summarize(path):
    rows = collections.OrderedDict()          # label -> [(median, spread, note)] per process
    for ln in open(path):
        p = ln.rstrip('\n').split('\t')
        if len(p) == 6 and p[0] == 'RATE':
            rows.setdefault(p[1], []).append((float(p[3]), float(p[4]), p[5]))
    labels = list(rows)
    base = labels[0]
    b = rows[base]
    bar = max(max(m for m, _, _ in b) - min(m for m, _, _ in b), max(s for _, s, _ in b))
    mean = {lb: float(np.mean([m for m, _, _ in rows[lb]])) for lb in labels}
    out = ['## N = 4096, %s' % SHAPE,
           '%-34s %s | mean     | spread inside a process' % ('ms per step', ' '.join('%9s' % ('run %d' % (i + 1)) for i in range(len(b))))]
    for lb in labels:
        out.append('%-34s %s | %8.4f | %s' % (lb, ' '.join('%9.4f' % m for m, _, _ in rows[lb]), mean[lb], ' '.join('%.4f' % s for _, s, _ in rows[lb])))
    out.append('the bar (the spread of %s: the gap between its processes, or the largest spread inside one): %.4f ms' % (base, bar))

    def against(x, y):
        if x in mean and y in mean:
            d = mean[x] - mean[y]
            out.append('%-22s - %-34s %+.4f ms (%+.2f %%): %s' % (x, y, d, 100 * d / mean[y], 'inside the bar' if abs(d) <= bar else ('faster' if d < 0 else 'slower') + ' by more than the bar'))
    for y in labels:
        if y.startswith('obs+render'):
            against('views', y)
    against('views', 'views-per-view')
    against('autoreset', 'autoreset-per-view')
    print('\n'.join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', choices=VARIANTS)
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the tree whose package is timed')
    ap.add_argument('--label', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--window', type=float, default=300.0, help='milliseconds of back-to-back steps per timing')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    sys.path.insert(0, args.tree)
    import torch
    from roboticsplayroompybullet_amd import VecPlayEnv, _lib
    label = args.label or args.variant
    n = args.n
    auto = args.variant.startswith('autoreset')
    env = VecPlayEnv(GID, n, seed=11, **(dict(autoreset=True, max_episode_steps=LIMIT) if auto else {}))
    env.reset()
    rng = np.random.default_rng(0)
    acts = [torch.tensor(LO + (HI - LO) * rng.random((n, 7)), dtype=torch.float32, device=env.device) for _ in range(50)]
    for a in acts:
        env.step(a)
    if auto:
        env.episode_steps = torch.arange(n, dtype=torch.int32) % LIMIT
    torch.cuda.synchronize()
    lines = ['# %s: tools/image_views_rate.py --variant %s on %s, %s (%s), N = %d' % (label, args.variant, torch.cuda.get_device_name(0), _lib.load().rp_version().decode(),
                                                                                      os.path.basename(os.path.abspath(args.tree)), n)]
    state = {'i': 0}
    fixed = dict(width=84, height=84, layers=('rgb',))
    wrist = dict(width=64, height=64, layers=('rgb', 'depth'), camera=env.camera(gripper=True))

    def ms(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    if args.variant == 'obs+render':
        env.set_image_obs(**fixed)
        out = {'rgb': torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=env.device), 'depth': torch.empty((n, 64, 64), dtype=torch.float32, device=env.device)}

        def fn():
            env.step(acts[state['i'] % 50])
            env.render_layers(out=out, **wrist)
            state['i'] += 1
    else:
        if args.variant.endswith('per-view'):
            env._call('rp_debug_image_views_merge', 0)
        env.set_image_views({'img': fixed, 'wrist': wrist})

        def fn():
            env.step(acts[state['i'] % 50])
            state['i'] += 1
    fn()
    reps = max(5, int(np.ceil(args.window / max(ms(fn, 5), 1e-3))))
    ts = [ms(fn, reps) for _ in range(3)]
    lines.append('RATE\t%s\t%s\t%.4f\t%.4f\t%d steps per timing: %s' % (label, SHAPE, float(np.median(ts)), max(ts) - min(ts), reps, ' '.join('%.4f' % t for t in ts)))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    env.close()


if __name__ == '__main__':
    main()
