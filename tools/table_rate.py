"""What the per-env parameter tables and the state-by-column calls cost (profiles/table_rate.txt), on the headline id at N = 4096.  Only VecPlayEnv's
public methods are used and every one is looked up with hasattr, so the job that alternates an older build and this one runs this same file in both trees.
--mode step: ms per rp_step with the table of --table as a fresh handle has it and, with --random, with every env's own row (dynamics: friction and masses scaled
by 0.25 .. 4; wrench: arm links up to 3 N / 0.3 N m, the other bodies up to 0.3 N / 0.003 N m; actuation: gravity tilted by up to 3 m/s^2 in x and y and changed by up
to 2 in z, gains 0.5 .. 1.5, strengths 0.3 .. 1.2; kinematics has no row to draw: its calls stay unused).  Device events around --steps steps, --repeats times after
a warm-up; one line per run, with --timers the per-launch timers of 64 more steps.
--mode calls: microseconds per set_* / get_* call of every table with [N, .] device tensors, and per set_body and clone_envs (a random permutation on the device); the
three state calls beside the only route a build without them has, timed in the same run: get_state, an edit of the columns (or a gather of the rows) in torch,
set_state.  Device events around --calls calls after a warm-up, --repeats times; the median per call.
usage: python tools/table_rate.py [env_id] [--mode step|calls] [--table T] [--random] [--timers] [--n N] [--steps K] [--calls C] [--repeats R] [--label L]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roboticsplayroompybullet_amd import VecPlayEnv  # noqa: E402

LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])
TABLES = ('dynamics', 'wrench', 'actuation', 'kinematics')


def randomise(env, table, n, dev):
    """every env its own row of `table`"""
    if table == 'kinematics':
        sys.exit('--random needs --table dynamics, wrench or actuation: the kinematics calls have no row to draw')
    if not hasattr(env, 'set_' + table):
        sys.exit('this build has no %s table' % table)
    g = torch.Generator().manual_seed(1)
    if table == 'dynamics':
        env.set_dynamics(**{k: (v.cpu() * (0.25 + 3.75 * torch.rand(v.shape, generator=g))).to(dev) for k, v in env.get_dynamics().items()})
    elif table == 'wrench':
        names = env.wrench_names
        w = 2 * torch.rand((n, len(names), 6), generator=g) - 1
        w = torch.where(w.abs() < 1e-3, torch.full_like(w, 1e-3), w)
        mag = torch.tensor([[3.0] * 3 + [0.3] * 3 if nm.startswith('link') else [0.3] * 3 + [0.003] * 3 for nm in names])
        env.set_wrench((w * mag).to(dev))
    else:
        na = len(env.actuation_names['motor'])
        grav = torch.tensor([0.0, 0.0, -9.8]) + torch.tensor([3.0, 3.0, 2.0]) * (2 * torch.rand((n, 3), generator=g) - 1)
        env.set_actuation(gravity=grav.to(dev), motor_gain=(0.5 + torch.rand((n, na), generator=g)).to(dev),
                          motor_strength=(0.3 + 0.9 * torch.rand((n, na), generator=g)).to(dev))


def timed(fn, calls, repeats, warmup=10):
    """the device time of `calls` back-to-back calls of fn, `repeats` times, in microseconds per call"""
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
    for k in range(args.warmup):
        env.step(a[k])
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
    tag = args.label or ('%s-%s' % (args.table, 'random' if args.random else 'default'))
    print('%-10s %s N=%d  ms/step per repeat: %s  median %.4f  spread %.4f' % (tag, args.env_id, args.n, ' '.join('%.4f' % x for x in ms),
                                                                      float(np.median(ms)), max(ms) - min(ms)))
    if args.timers:
        env.enable_timers(64)
        for k in range(64):
            env.step(a[args.warmup + k % args.steps])
        torch.cuda.synchronize()
        print('%-10s per-launch timers: %s' % (tag, ' '.join('%s=%.4g' % kv for kv in env.timers().items())))


def calls_mode(env, args, dev):
    n = args.n
    tag = (args.label + ' ') if args.label else ''
    print('%s%s N=%d, %d bytes per state row; microseconds per call, median of %d repeats of %d calls (all repeats in brackets)' %
          (tag, args.env_id, n, env.lib.rp_state_bytes(env.h), args.repeats, args.calls))

    def report(name, fn):
        us = timed(fn, args.calls, args.repeats)
        print('%s%-20s %8.1f us [%s]' % (tag, name, float(np.median(us)), ' '.join('%.1f' % x for x in us)))
        return float(np.median(us))

    # every table's get and set, the set with what the get returned as [N, .] device tensors
    for table in TABLES:
        if not hasattr(env, 'set_' + table):
            continue
        get, put = getattr(env, 'get_' + table), getattr(env, 'set_' + table)
        cur = get()
        report('get_' + table, get)
        report('set_' + table, (lambda: put(cur)) if table == 'wrench' else (lambda: put(**cur)))
    # the state calls beside the blob route
    lay = env.state_layout
    nfree = sum(1 for k in lay if k.startswith('free'))
    f0 = lay['free0'][0]
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

    # (blob_set: get_state + column edit + set_state, against set_kinematics(pos, vel) above; blob_body: the same for one body; blob_clone: get_state + gather + set_state)
    blob = {'set_kinematics': report('blob_set', blob_set), 'set_body': report('blob_body', blob_body),
            'clone_envs': report('blob_clone', lambda: env.set_state(env.get_state()[perm]))}
    if hasattr(env, 'set_body'):
        new = {'set_kinematics': report('set_kinematics(p,v)', lambda: env.set_kinematics(pos=p, vel=v)),
               'set_body': report('set_body', lambda: env.set_body('block', pos=xyz, lin_vel=lin)), 'clone_envs': report('clone_envs', lambda: env.clone_envs(perm32))}
        for k in blob:
            print('%s%-20s blob route / new call  ratio %.2f' % (tag, k, blob[k] / new[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('env_id', nargs='?', default='UR5PlayAbsRPY1Obj-v0')
    ap.add_argument('--mode', choices=('step', 'calls'), default='step')
    ap.add_argument('--table', choices=TABLES, default='kinematics')
    ap.add_argument('--random', action='store_true', help="step mode: every env its own row of --table")
    ap.add_argument('--timers', action='store_true', help='step mode: print the per-launch timers of 64 more steps')
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    env = VecPlayEnv(args.env_id, args.n, seed=0)
    if args.mode == 'step' and args.random:
        randomise(env, args.table, args.n, dev)
    env.reset()
    if args.mode == 'step':
        step_mode(env, args, dev)
    else:
        calls_mode(env, args, dev)
    torch.cuda.synchronize()
    env.close()


if __name__ == '__main__':
    main()
