"""What an image costs on the GPU box (DESIGN.md "Camera layers", profiles/render_rate_one_kernel.txt): rp_render and rp_render_layers, which share one kernel
(k_render_layers, a 16 x 16 tile per block with its shortlist of records) - rp_render, rp_render_layers colour only with the shortlist, colour only with the shortlist
switched off (rp_debug_render_cull(h, 0)), all three layers with it - at the sizes a learner runs: N = 4096 at 64 x 64 and 84 x 84 (fixed and gripper camera), N = 64 at
200 x 200, UR5PlayAbsRPY1Obj-v0 after 50 random steps.  Every call is k_collider_poses + the render kernel; the 1 x 1 pixel line is what k_collider_poses and the two
launches cost alone.  Device events around enough back-to-back calls for --window ms per timing, every shape warmed up, three timings per variant and round (their median
counts), the variants alternated over three rounds; the spread of a variant's own three round medians is the bar a difference has to clear.  To compare two builds, run
the tool once per build in processes of their own, alternated, with RP_PLAYROOM_LIB naming the library to time (a library from before an entry point _lib binds
cannot be loaded that way: run that commit's own tree).  --visuals random: every handle gets a random per-env visuals table first (rp_set_visuals: colours, light and
background differ in every env), so the kernels read the table instead of their constants (profiles/visuals_rate.txt); the default, none, never makes the table.
usage: python tools/render_rate.py [--out profiles/render_rate_one_kernel.txt] [--window 300] [--n 4096] [--visuals none|random]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roboticsplayroompybullet_amd import VecPlayEnv  # noqa: E402

GID = 'UR5PlayAbsRPY1Obj-v0'
LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])
VARIANTS = ('rp_render', 'layers rgb', 'layers rgb, shortlist off', 'layers rgb + depth + segmentation')


def gpu_ms(fn, reps):
    """device time per call of fn (events around reps calls)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def stepped_env(n):
    env = VecPlayEnv(GID, n, seed=11)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(50):
        env.step(torch.tensor(LO + (HI - LO) * rng.random((n, 7)), dtype=torch.float32, device=env.device))
    torch.cuda.synchronize()
    return env


def random_visuals(env):
    """a seeded visuals row per env, built on the device: colours and background uniform in [0, 1), a unit direction in the upper half space, ambient in [0.2, 0.6),
    diffuse in [0.3, 0.8)"""
    gen = torch.Generator(device=env.device).manual_seed(5)
    n = env.num_envs
    u = lambda *shape: torch.rand(shape, generator=gen, device=env.device)          # noqa: E731
    d = u(n, 3) * torch.tensor([2.0, 2.0, 1.0], device=env.device) - torch.tensor([1.0, 1.0, -0.2], device=env.device)
    light = torch.cat([d / d.norm(dim=1, keepdim=True), 0.2 + 0.4 * u(n, 1), 0.3 + 0.5 * u(n, 1)], 1)
    env.set_visuals(colour=u(n, len(env.visual_names), 3), light=light, background=u(n, 3))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'render_rate_one_kernel.txt'))
    ap.add_argument('--window', type=float, default=300.0, help='milliseconds of back-to-back calls per timing')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--visuals', choices=('none', 'random'), default='none', help='random: a random per-env visuals table is set on every handle first')
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('# tools/render_rate.py on %s, one job.  %s after 50 random steps; ms per call = k_collider_poses + the render kernel; device events around >= %d ms of'
        % (torch.cuda.get_device_name(0), GID, args.window))
    say('# back-to-back calls per timing, every shape warmed up, median of three timings per variant and round, variants alternated over three rounds.')
    say('# visuals: %s' % ('a random table set on every handle (rp_set_visuals)' if args.visuals == 'random' else 'no table (the kernels\' constants)'))
    shapes = [(args.n, 64, 64, False), (args.n, 84, 84, False), (args.n, 84, 84, True), (64, 200, 200, False)]
    env = None
    verdict = []
    for n, w, h, gripper in shapes:
        if env is None or env.num_envs != n:          # one handle at a time
            if env is not None:
                env.close()
            env = stepped_env(n)
            if args.visuals == 'random':
                random_visuals(env)
        cam = env.camera(gripper=True) if gripper else None
        rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=env.device)
        out = {'rgb': rgb, 'depth': torch.empty((n, h, w), dtype=torch.float32, device=env.device),
               'segmentation': torch.empty((n, h, w), dtype=torch.int32, device=env.device)}

        def layers(which, on):
            def fn():
                env.lib.rp_debug_render_cull(env.h, on)
                env.render_layers(width=w, height=h, camera=cam, layers=which, out=out)
            return fn
        fns = {VARIANTS[0]: lambda: env.render('rgb_array', width=w, height=h, camera=cam, out=rgb), VARIANTS[1]: layers(('rgb',), 1), VARIANTS[2]: layers(('rgb',), 0),
               VARIANTS[3]: layers(('rgb', 'depth', 'segmentation'), 1)}
        # the layers' colour is rp_render's image at the size timed, with the shortlist and without it (faster and different is not faster)
        want = env.render('rgb_array', width=w, height=h, camera=cam).clone()
        for on in (1, 0):
            layers(('rgb',), on)()
            assert torch.equal(rgb, want), 'render_layers differs from rp_render (shortlist %d)' % on
        reps = {}
        for v in VARIANTS:          # warm-up, and the number of calls that fill the window
            fns[v]()
            reps[v] = max(5, int(np.ceil(args.window / max(gpu_ms(fns[v], 5), 1e-3))))
        med = {v: [] for v in VARIANTS}
        say()
        say('## N = %d, %d x %d, %s camera' % (n, w, h, 'gripper' if gripper else 'fixed'))
        for rnd in range(3):
            for v in VARIANTS:
                ts = [gpu_ms(fns[v], reps[v]) for _ in range(3)]
                med[v].append(float(np.median(ts)))
                say('round %d  %-36s %5d calls per timing  ms per call: %s  median %.4f' % (rnd + 1, v, reps[v], ' '.join('%.4f' % t for t in ts), med[v][-1]))
        env.lib.rp_debug_render_cull(env.h, 1)
        m = {v: float(np.median(med[v])) for v in VARIANTS}
        spread = {v: max(med[v]) - min(med[v]) for v in VARIANTS}
        for v in VARIANTS:
            say('%-36s median of the three medians %.4f ms  (they spread by %.4f ms, %.2f %%)  %.3f M images/s' % (v, m[v], spread[v], 100 * spread[v] / m[v], n / m[v] / 1e3))
        bar = max(spread[VARIANTS[1]], spread[VARIANTS[2]])
        say('shortlist on / off: %.3f  (%+.4f ms; the bar: %.4f ms)' % (m[VARIANTS[1]] / m[VARIANTS[2]], m[VARIANTS[1]] - m[VARIANTS[2]], bar))
        verdict.append((n, w, h, gripper, m[VARIANTS[2]] - m[VARIANTS[1]] > bar))
        if not gripper:
            one = torch.empty((n, 1, 1, 3), dtype=torch.uint8, device=env.device)
            fn = lambda: env.render('rgb_array', width=1, height=1, out=one)          # noqa: E731
            fn()
            say('rp_render at 1 x 1 pixel (k_collider_poses and the two launches alone): %.4f ms' % float(np.median([gpu_ms(fn, max(5, int(args.window / 4 / max(gpu_ms(fn, 5), 1e-3)))) for _ in range(3)])))
    say()
    for n, w, h, gripper, cull_pays in verdict:
        say('N = %d %d x %d%s: the shortlist %s the switch-off variant by more than the spread' % (n, w, h, ' gripper' if gripper else '', 'beats' if cull_pays else 'DOES NOT beat'))
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
