"""What a point cloud per env inside the batched step costs on the GPU box (DESIGN.md "Point clouds from the camera views", profiles/image_points_rate.txt): N = 4096 of
UR5PlayAbsRPY1Obj-v0 after 50 random steps, autoreset=True with max_episode_steps=200 and counters staggered e % 200 (about N / 200 envs end in every step), one
84 x 84 view of the fixed camera with depth (metres) + segmentation and terminal frames, one process per variant:

  plain    the view alone: per step the terminal pass over the ended envs and the observation pass, two launches each
  points   ... with a 1024-point world-frame cloud attached (set_image_points(1024)): one more k_point_cloud launch behind each pass

ms per autoreset step from device events around enough back-to-back steps for --window ms, warmed up, three timings, their median; env-steps/s = N / that.  The points
process also times k_point_cloud itself: render_points (k_collider_poses, k_render_layers, k_point_cloud) against render_layers (the first two) for all N envs at the same
size into preallocated tensors, back to back on one stream - the difference per call is the kernel's time per launch, launch gap included.  Each process appends its
lines to --out; `--summarize raw.txt` turns the lines of a job that ran both variants twice, alternated, into the table.  No threshold: both rates and their ratio.
usage: python tools/image_points_rate.py --variant points [--out FILE] [--window 300] [--n 4096]
       python tools/image_points_rate.py --summarize FILE"""
import argparse
import collections
import ctypes as C
import os
import sys

import numpy as np

GID = 'UR5PlayAbsRPY1Obj-v0'
LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])
VARIANTS = ('plain', 'points')
LIMIT = 200
SIZE, POINTS = 84, 1024
SHAPE = 'autoreset step, one %d x %d view (depth + segmentation, terminal frames), cloud of %d points' % (SIZE, SIZE, POINTS)


def summarize(path):
    rows, kern = collections.OrderedDict(), []
    for ln in open(path):
        p = ln.rstrip('\n').split('\t')
        if len(p) == 5 and p[0] == 'RATE':
            rows.setdefault(p[1], []).append((float(p[2]), float(p[3]), p[4]))
        if len(p) == 4 and p[0] == 'KERNEL':
            kern.append((float(p[1]), float(p[2]), float(p[3])))
    n = 4096
    mean = {lb: float(np.mean([m for m, _, _ in r])) for lb, r in rows.items()}
    out = ['## N = %d, %s' % (n, SHAPE),
           '%-8s %s | mean ms  | env-steps/s | spread inside a process' % ('', ' '.join('%9s' % ('run %d' % (i + 1)) for i in range(max(len(r) for r in rows.values()))))]
    for lb, r in rows.items():
        out.append('%-8s %s | %8.4f | %11.0f | %s' % (lb, ' '.join('%9.4f' % m for m, _, _ in r), mean[lb], 1e3 * n / mean[lb], ' '.join('%.4f' % s for _, s, _ in r)))
    if 'plain' in mean and 'points' in mean:
        out.append('points / plain: %.4f of the env-steps/s (%+.4f ms per step)' % (mean['plain'] / mean['points'], mean['points'] - mean['plain']))
    for lay, pts, d in kern:
        out.append('k_point_cloud per launch, N = %d: render_points %.4f ms - render_layers %.4f ms = %.4f ms' % (n, pts, lay, d))
    print('\n'.join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', choices=VARIANTS)
    ap.add_argument('--out', default=None)
    ap.add_argument('--window', type=float, default=300.0, help='milliseconds of back-to-back steps per timing')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from roboticsplayroompybullet_amd import VecPlayEnv, _lib
    n = args.n
    env = VecPlayEnv(GID, n, seed=11, autoreset=True, max_episode_steps=LIMIT)
    env.reset()
    rng = np.random.default_rng(0)
    acts = [torch.tensor(LO + (HI - LO) * rng.random((n, 7)), dtype=torch.float32, device=env.device) for _ in range(50)]
    for a in acts:
        env.step(a)
    env.episode_steps = torch.arange(n, dtype=torch.int32) % LIMIT
    torch.cuda.synchronize()
    lines = ['# %s: tools/image_points_rate.py --variant %s on %s, %s, N = %d' % (args.variant, args.variant, torch.cuda.get_device_name(0),
                                                                                 _lib.load().rp_version().decode(), n)]
    state = {'i': 0}
    view = dict(width=SIZE, height=SIZE, layers=('depth', 'segmentation'), depth='metres')
    env.set_image_obs(**view)
    if args.variant == 'points':
        env.set_image_points(POINTS)

    def ms(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    def fn():
        env.step(acts[state['i'] % 50])
        state['i'] += 1
    fn()
    reps = max(5, int(np.ceil(args.window / max(ms(fn, 5), 1e-3))))
    ts = [ms(fn, reps) for _ in range(3)]
    lines.append('RATE\t%s\t%.4f\t%.4f\t%d steps per timing: %s' % (args.variant, float(np.median(ts)), max(ts) - min(ts), reps, ' '.join('%.4f' % t for t in ts)))
    if args.variant == 'points':
        dev = env.device
        depth, seg = torch.empty((n, SIZE, SIZE), dtype=torch.float32, device=dev), torch.empty((n, SIZE, SIZE), dtype=torch.int32, device=dev)
        xyz, pseg, cnt = env._points_tensors(n, POINTS, False).values()
        spec = _lib.RpPointsSpec(POINTS, _lib.POINTS_WORLD, 0.0, 0)
        out = {'depth': depth, 'segmentation': seg}

        def layers():
            env.render_layers(out=out, **view)

        def points():
            env._call('rp_render_points', None, None, SIZE, SIZE, 0, n, C.byref(spec), None, depth.data_ptr(), seg.data_ptr(), xyz.data_ptr(), pseg.data_ptr(), None,
                      cnt.data_ptr(), env._stream())
        layers(), points()
        reps = max(5, int(np.ceil(args.window / max(ms(points, 5), 1e-3))))
        lay = float(np.median([ms(layers, reps) for _ in range(3)]))
        pts = float(np.median([ms(points, reps) for _ in range(3)]))
        lines.append('KERNEL\t%.4f\t%.4f\t%.4f' % (lay, pts, pts - lay))
    print('\n'.join(lines), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    env.close()


if __name__ == '__main__':
    main()
