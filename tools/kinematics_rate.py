"""What rp_set_kinematics / rp_copy_envs cost (profiles/kinematics_rate.txt), on the headline id at N = 4096.
--mode step: ms per rp_step with the new calls unused - device events around --steps steps, --repeats times after a warm-up; one line per run.  Runs on a tree
without the calls too: the job that alternates the parent's build and this one runs this same file in both.
--mode calls: microseconds per call of set_kinematics (both halves, [N, .] device tensors), set_body (the block's position and linear velocity, device tensors)
and clone_envs (a random permutation on the device), each beside the only route a build without them has, timed in the same run: get_state, an edit of the
columns (or a gather of the rows) in torch, set_state.  Device events around --calls calls after a warm-up, --repeats times; the median per call.
usage: python tools/kinematics_rate.py [env_id] [--mode step|calls] [--n N] [--steps K] [--calls C] [--repeats R] [--label L]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roboticsplayroompybullet_amd import VecPlayEnv  # noqa: E402

LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])


def timed(fn, calls, repeats, warmup=10):
    """median over `repeats` of the device time of `calls` back-to-back calls of fn, in microseconds per call"""
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * t0.elapsed_time(t1) / calls)
    return us


def step_mode(env, args, dev):
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
    print('%-6s %s N=%d  ms/step per repeat: %s  median %.4f  spread %.4f' % (args.label or 'step', args.env_id, args.n, ' '.join('%.4f' % x for x in ms),
                                                                          float(np.median(ms)), max(ms) - min(ms)))


def calls_mode(env, args, dev):
    n = args.n
    lay = env.state_layout
    nfree = sum(1 for k in lay if k.startswith('free'))
    f0 = lay['free0'][0]
    # the blob route's view of the kinematics columns
    pos_i = list(range(*lay['q'])) + [lay['free%d' % f][0] + j for f in range(nfree) for j in range(7)] + list(range(*lay['jq']))
    vel_i = list(range(*lay['qd'])) + [lay['free%d' % f][0] + 7 + j for f in range(nfree) for j in range(6)] + list(range(*lay['jqd']))
    pos_i, vel_i = torch.tensor(pos_i, device=dev), torch.tensor(vel_i, device=dev)
    st = env.get_state()
    p, v = st[:, pos_i].clone(), st[:, vel_i].clone()
    xyz, lin = st[:, f0:f0 + 3].clone(), st[:, f0 + 7:f0 + 10].clone()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    perm32 = perm.to(torch.int32)

    def blob_set():
        s = env.get_state()
        s[:, pos_i] = p
        s[:, vel_i] = v
        env.set_state(s)

    def blob_body():
        s = env.get_state()
        s[:, f0:f0 + 3] = xyz
        s[:, f0 + 7:f0 + 10] = lin
        env.set_state(s)

    def blob_clone():
        env.set_state(env.get_state()[perm])

    routes = [('set_kinematics', 'get_state + column edit + set_state', blob_set), ('set_body', 'get_state + column edit + set_state', blob_body),
              ('clone_envs', 'get_state + gather + set_state', blob_clone)]
    new = {}
    if hasattr(env, 'set_kinematics'):
        new = {'set_kinematics': lambda: env.set_kinematics(pos=p, vel=v), 'set_body': lambda: env.set_body('block', pos=xyz, lin_vel=lin),
               'clone_envs': lambda: env.clone_envs(perm32)}
    print('%s N=%d, %d bytes per state row; microseconds per call, median of %d repeats of %d calls (all repeats in brackets)' %
          (args.env_id, n, env.lib.rp_state_bytes(env.h), args.repeats, args.calls))
    for name, what, blob in routes:
        us_b = timed(blob, args.calls, args.repeats)
        line = '%-15s blob route (%s) %8.1f us [%s]' % (name, what, float(np.median(us_b)), ' '.join('%.1f' % x for x in us_b))
        if name in new:
            us_n = timed(new[name], args.calls, args.repeats)
            line += '   new call %8.1f us [%s]   ratio %.2f' % (float(np.median(us_n)), ' '.join('%.1f' % x for x in us_n), np.median(us_b) / np.median(us_n))
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('env_id', nargs='?', default='UR5PlayAbsRPY1Obj-v0')
    ap.add_argument('--mode', choices=('step', 'calls'), default='step')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    env = VecPlayEnv(args.env_id, args.n, seed=0)
    env.reset()
    if args.mode == 'step':
        step_mode(env, args, dev)
    else:
        calls_mode(env, args, dev)
    torch.cuda.synchronize()
    env.close()


if __name__ == '__main__':
    main()
