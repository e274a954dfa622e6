"""What camera images inside the batched step cost on the GPU box (DESIGN.md "Images written by the step", profiles/image_obs_rate.txt): N = 4096 of
UR5PlayAbsRPY1Obj-v0 after 50 random steps, 64 x 64 and 84 x 84, rgb alone and all three layers, one process per variant:

  step+render        (a) the route before rp_set_image_obs: step, then render_layers into preallocated tensors - a second library call per step.  Uses nothing this
                     feature added, so the same file times an older tree: run it with that tree first on sys.path (--tree).
  image-obs          (b) step with set_image_obs: the same two kernels launched from inside rp_step
  autoreset          (c) autoreset=True, max_episode_steps=200, counters staggered e % 200 (about N / 200 envs end in every step), image observations WITHOUT
                     terminal frames (final_* NULL at the ABI)
  autoreset+final    (c) ... with terminal frames: the terminal pass's two launches over all N envs, of which the ended envs' blocks do work

ms per step from device events around enough back-to-back steps for --window ms, every shape warmed up, three timings, their median.  Each process appends its lines
to --out; `--summarize raw.txt` turns the lines of a job that ran every variant twice, alternated, into the table.  The bar a difference has to clear is the spread of
(a) on the older tree: the larger of the gap between its two processes and of the spread of the three timings inside a process.
usage: python tools/image_obs_rate.py --variant image-obs [--tree DIR] [--label NAME] [--out FILE] [--window 300] [--n 4096]
       python tools/image_obs_rate.py --summarize FILE"""
import argparse
import collections
import os
import sys

import numpy as np

GID = 'UR5PlayAbsRPY1Obj-v0'
LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])
VARIANTS = ('step+render', 'image-obs', 'autoreset', 'autoreset+final')
SHAPES = ((64, 64, ('rgb',)), (64, 64, ('rgb', 'depth', 'segmentation')), (84, 84, ('rgb',)), (84, 84, ('rgb', 'depth', 'segmentation')))
LIMIT = 200


def summarize(path):
    rows = collections.OrderedDict()          # (label, shape) -> [(median, spread)] per process
    for ln in open(path):
        p = ln.rstrip('\n').split('\t')
        if len(p) == 6 and p[0] == 'RATE':
            rows.setdefault((p[1], p[2]), []).append((float(p[3]), float(p[4]), p[5]))
    labels = list(collections.OrderedDict((k[0], None) for k in rows))
    shapes = list(collections.OrderedDict((k[1], None) for k in rows))
    base = labels[0]
    out = []
    for sh in shapes:
        out.append('## %s' % sh)
        out.append('%-28s %s | mean     | - %s (means)' % ('ms per step', ' '.join('%9s' % ('run %d' % (i + 1)) for i in range(len(rows[(base, sh)]))), base))
        b = rows[(base, sh)]
        bmean = float(np.mean([m for m, _, _ in b]))
        bar = max(max(m for m, _, _ in b) - min(m for m, _, _ in b), max(s for _, s, _ in b))
        for lb in labels:
            r = rows.get((lb, sh))
            if not r:
                continue
            mean = float(np.mean([m for m, _, _ in r]))
            out.append('%-28s %s | %8.4f | %+.4f ms (%+.2f %%)' % (lb, ' '.join('%9.4f' % m for m, _, _ in r), mean, mean - bmean, 100 * (mean - bmean) / bmean))
        out.append('the bar (the spread of %s): %.4f ms' % (base, bar))
        out.append('')
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
    lines = ['# %s: tools/image_obs_rate.py --variant %s on %s, %s (%s), N = %d' % (label, args.variant, torch.cuda.get_device_name(0), _lib.load().rp_version().decode(),
                                                                                    os.path.basename(os.path.abspath(args.tree)), n)]
    state = {'i': 0}

    def ms(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    for w, h, layers in SHAPES:
        if args.variant == 'step+render':
            out = {'rgb': torch.empty((n, h, w, 3), dtype=torch.uint8, device=env.device), 'depth': torch.empty((n, h, w), dtype=torch.float32, device=env.device),
                   'segmentation': torch.empty((n, h, w), dtype=torch.int32, device=env.device)}

            def fn():
                env.step(acts[state['i'] % 50])
                env.render_layers(width=w, height=h, layers=layers, out=out)
                state['i'] += 1
        else:
            env.set_image_obs(width=w, height=h, layers=layers)
            if args.variant == 'autoreset':          # the same output tensors, no terminal frames
                p = [env.image_obs[k].data_ptr() if k in env.image_obs else None for k in ('rgb', 'depth', 'segmentation')]
                env._call('rp_set_image_obs', None, None, 0.01, 10.0, 0, w, h, *p, None, None, None)

            def fn():
                env.step(acts[state['i'] % 50])
                state['i'] += 1
        fn()
        reps = max(5, int(np.ceil(args.window / max(ms(fn, 5), 1e-3))))
        ts = [ms(fn, reps) for _ in range(3)]
        shape = 'N = %d, %d x %d, %s' % (n, w, h, ' + '.join(layers))
        lines.append('RATE\t%s\t%s\t%.4f\t%.4f\t%d steps per timing: %s' % (label, shape, float(np.median(ts)), max(ts) - min(ts), reps, ' '.join('%.4f' % t for t in ts)))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    env.close()


if __name__ == '__main__':
    main()
