"""What an image of a STORED state row costs on the GPU box (DESIGN.md "Images of stored state rows", profiles/render_states_rate.txt): rp_render_layers on a handle
of N = 4096 envs of UR5PlayAbsRPY1Obj-v0 after 50 random steps against rp_render_states of the same 4096 rows (get_state()), drawn by the same handle, in three forms -
the rows as they lie (identity), through a random index (a permutation of the rows: the same work, gathered), and with solid goals (every env's desired goal, the
sub-goal's words overwritten before the one pass) - at 64 x 64 and 84 x 84, colour only and all three layers.  A further form, the index 0 .. N - 1 written out, is
the identity's images in the identity's order through the gather's code path: it tells a cost of the path from an effect of the order.  Each call is a pose kernel +
a draw kernel either way (k_collider_poses + k_render_layers, k_collider_poses_rows + k_render_states); the same tiles are drawn by the same device function, so the
expectation is a ratio of 1 within render_layers' own round-to-round spread, which the tool measures in the same process and holds every ratio against (twice the
spread is the bar).  Device events around enough back-to-back calls for --window ms per timing, every shape warmed up, three timings per variant and round (their
median counts), the variants alternated over three rounds, each round starting one variant further on, so that no variant always runs behind the same one.  Before
anything is timed the identity form's bytes, and the gathered form's, are compared with render_layers' at the size timed.
usage: python tools/render_states_rate.py [--out profiles/render_states_rate.txt] [--window 300] [--n 4096]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from render_rate import gpu_ms, stepped_env  # noqa: E402

VARIANTS = ('render_layers', 'render_states identity', 'render_states index = 0 .. N - 1', 'render_states random index', 'render_states solid goals')
ALL = ('rgb', 'depth', 'segmentation')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'render_states_rate.txt'))
    ap.add_argument('--window', type=float, default=300.0, help='milliseconds of back-to-back calls per timing')
    ap.add_argument('--n', type=int, default=4096)
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    n = args.n
    env = stepped_env(n)
    say('# tools/render_states_rate.py on %s, one process.  %s, N = %d after 50 random steps; ms per call = the pose kernel + the draw kernel; device events around'
        % (torch.cuda.get_device_name(0), env.env_id, n))
    say('# >= %d ms of back-to-back calls per timing, every shape warmed up, median of three timings per variant and round, variants alternated over three rounds' % args.window)
    say('# (round r starts at variant r).')
    states = env.get_state()
    goal = env.calc_state()['desired_goal'].clone()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(device=env.device, dtype=torch.int32)
    ident = torch.arange(n, dtype=torch.int32, device=env.device)
    verdict = []
    for w, h in ((64, 64), (84, 84)):
        for which in (('rgb',), ALL):
            out = {'rgb': torch.empty((n, h, w, 3), dtype=torch.uint8, device=env.device), 'depth': torch.empty((n, h, w), dtype=torch.float32, device=env.device),
                   'segmentation': torch.empty((n, h, w), dtype=torch.int32, device=env.device)}
            kw = dict(width=w, height=h, layers=which, out=out)
            fns = {VARIANTS[0]: lambda: env.render_layers(**kw), VARIANTS[1]: lambda: env.render_states(states, **kw),
                   VARIANTS[2]: lambda: env.render_states(states, index=ident, **kw), VARIANTS[3]: lambda: env.render_states(states, index=perm, **kw),
                   VARIANTS[4]: lambda: env.render_states(states, goal=goal, goal_mode='solid', **kw)}
            # the identity form writes render_layers' bytes at the size timed (faster and different is not faster)
            want = {k: v.clone() for k, v in env.render_layers(width=w, height=h, layers=which).items()}
            fns[VARIANTS[1]]()
            torch.cuda.synchronize()
            for k in which:
                assert torch.equal(out[k], want[k]), 'render_states differs from render_layers (%s, %d x %d)' % (k, w, h)
            fns[VARIANTS[3]]()
            torch.cuda.synchronize()
            for k in which:
                assert torch.equal(out[k], want[k][perm.long()]), 'the gathered images differ from render_layers (%s, %d x %d)' % (k, w, h)
            reps = {}
            for v in VARIANTS:          # warm-up, and the number of calls that fill the window
                fns[v]()
                reps[v] = max(5, int(np.ceil(args.window / max(gpu_ms(fns[v], 5), 1e-3))))
            med = {v: [] for v in VARIANTS}
            say()
            say('## N = %d, %d x %d, %s' % (n, w, h, ' + '.join(which)))
            for rnd in range(3):
                for v in VARIANTS[rnd:] + VARIANTS[:rnd]:
                    ts = [gpu_ms(fns[v], reps[v]) for _ in range(3)]
                    med[v].append(float(np.median(ts)))
                    say('round %d  %-34s %5d calls per timing  ms per call: %s  median %.4f' % (rnd + 1, v, reps[v], ' '.join('%.4f' % t for t in ts), med[v][-1]))
            m = {v: float(np.median(med[v])) for v in VARIANTS}
            spread = {v: max(med[v]) - min(med[v]) for v in VARIANTS}
            for v in VARIANTS:
                say('%-34s median of the three medians %.4f ms  (they spread by %.4f ms, %.2f %%)  %.3f M images/s' % (v, m[v], spread[v], 100 * spread[v] / m[v], n / m[v] / 1e3))
            base = VARIANTS[0]
            for v in VARIANTS[1:]:
                ratio = m[v] / m[base]
                beyond = abs(m[v] - m[base]) > 2 * spread[base]
                say('%s / render_layers: %.4f  (%+.4f ms; twice render_layers\' own spread: %.4f ms)%s' % (v, ratio, m[v] - m[base], 2 * spread[base], '  BEYOND' if beyond else ''))
                verdict.append((w, h, which, v, ratio, beyond))
    say()
    for w, h, which, v, ratio, beyond in verdict:
        say('%d x %d %-34s %-34s ratio %.4f: %s' % (w, h, ' + '.join(which), v, ratio, 'beyond twice the spread' if beyond else 'within twice the spread'))
    env.close()
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
