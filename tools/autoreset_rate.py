"""rp_step_autoreset's cost on the GPU box (profiles/autoreset_rate.txt):
  1. reset latency for 1 / 16 / 64 / 256 ending envs of 4096: the autoreset step minus a step without ends, against rp_reset(mask) (host rounds);
     for one and for four envs per k_autoreset block (RP_AUTORESET_EPB, read at rp_create)
  2. env-steps/s at N = 4096 with staggered 250- and 50-step episodes: autoreset against the step + reset(mask) loop
  3. the autoreset step without ends against rp_step
--table M: the autoreset handles restart ended envs from a reset table of M random_start_table rows (rp_set_reset_table) instead of settling; section 1
  then compares the table against the settled autoreset (one env per block), section 2 adds the settled autoreset's rate (DESIGN.md,
  profiles/autoreset_table_rate.txt)
usage: python tools/autoreset_rate.py [env_id] [--steps K] [--table M]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roboticsplayroompybullet_amd import VecPlayEnv  # noqa: E402

LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])


def acts(n, steps, dev):
    rng = np.random.default_rng(0)
    return torch.tensor(LO + (HI - LO) * rng.random((steps, n, 7)), dtype=torch.float32, device=dev)


def gpu_ms(fn, reps):
    """device time per call of fn (events around reps calls)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('env_id', nargs='?', default='UR5PlayAbsRPY1Obj-v0')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--table', type=int, default=0, help='rows of a reset table (0: settle, as in ABI 0.5)')
    args = ap.parse_args()
    n, gid = args.n, args.env_id
    print('# %s, N = %d, %s%s' % (gid, n, torch.cuda.get_device_name(0), ', reset table of %d rows' % args.table if args.table else ''))
    dev = torch.device('cuda', 0)
    A = acts(n, args.steps, dev)
    table = None
    if args.table:
        maker = VecPlayEnv(gid, 8, seed=7)
        table = maker.random_start_table(args.table, 7)
        maker.close()

    def autoreset_env(seed, limit, use_table=True, **kw):
        return VecPlayEnv(gid, n, seed=seed, autoreset=True, max_episode_steps=limit, reset_table=table if use_table else None, **kw)

    # one handle at a time: a second handle's group streams share the process's hardware queues with the first one's and slow its steps down
    print('## 1. reset latency (ms): autoreset step - step without ends | rp_reset(mask), wall time incl. its host rounds')
    ks = (1, 16, 64, 256)
    masks = {}
    for k in ks:
        masks[k] = torch.zeros(n, dtype=torch.uint8, device=dev)
        masks[k][torch.randperm(n, generator=torch.Generator().manual_seed(k))[:k].to(dev)] = 1
    none = torch.zeros(n, dtype=torch.uint8, device=dev)
    res = {}
    # rows: ('table', 1) = the reset table; (None, epb) = settling with epb envs per k_autoreset block
    configs = (('table', 1), (None, 1)) if table is not None else ((None, 1), (None, 4))
    for use, epb in configs:
        os.environ['RP_AUTORESET_EPB'] = str(epb)
        ar = autoreset_env(1, 0, use_table=use is not None, end_on_fault=False)
        ar.reset()
        for _ in range(3):
            ar.step(A[0], end_mask=none)
        base = gpu_ms(lambda i: ar.step(A[i % args.steps], end_mask=none), 20)
        for k in ks:
            res[use, epb, k] = (gpu_ms(lambda i: ar.step(A[i % args.steps], end_mask=masks[k]), 10), base)
        ar.close()
    os.environ.pop('RP_AUTORESET_EPB')
    host = VecPlayEnv(gid, n, seed=1)
    host.reset()
    t_host = {k: wall_ms(lambda i: host.reset(mask=masks[k]), 5) for k in ks}
    host.close()
    for use, epb in configs:
        for k in ks:
            t_ar, base = res[use, epb, k]
            print('%s  k = %3d: autoreset step %7.2f ms (step alone %5.2f) -> reset %7.2f ms | rp_reset(mask) %7.2f ms'
                  % ('table' if use else 'epb %d' % epb, k, t_ar, base, t_ar - base, t_host[k]))

    print('## 2. env-steps/s, staggered episodes (%d steps)' % args.steps)
    for limit in (250, 50):
        t_set = {}
        for use in ((True, False) if table is not None else (False,)):
            ar = autoreset_env(2, limit, use_table=use, end_on_fault=False)
            ar.reset()
            ar.episode_steps = torch.arange(n, dtype=torch.int32) % limit
            t_set[use] = wall_ms(lambda i: ar.step(A[i % args.steps]), args.steps)
            ar.close()
        t_ar = t_set[table is not None]
        host = VecPlayEnv(gid, n, seed=2)
        host.reset()
        cnt = torch.arange(n, dtype=torch.int32, device=dev) % limit

        def host_step(i):
            nonlocal cnt
            host.step(A[i % args.steps])
            cnt = cnt + 1
            done = cnt >= limit
            if bool(done.any()):
                host.reset(mask=done)
                cnt = torch.where(done, torch.zeros_like(cnt), cnt)
        t_host = wall_ms(host_step, args.steps)
        host.close()
        settled = ''
        if table is not None:
            settled = ' | settling autoreset %6.3f ms/step = %6.3f M env-steps/s' % (t_set[False], n / t_set[False] / 1e3)
        print('limit %3d (~%d ends per step): autoreset%s %6.3f ms/step = %6.3f M env-steps/s%s | step + reset(mask) %7.3f ms/step = %6.3f M env-steps/s'
              % (limit, n // limit, ' (table)' if table is not None else '', t_ar, n / t_ar / 1e3, settled, t_host, n / t_host / 1e3))

    print('## 3. no ends: autoreset step vs rp_step (device time per step over %d steps, fresh handle each, alternating, 3 rounds)' % args.steps)
    r_ar, r_pl = [], []
    for _ in range(3):
        for auto, out in ((False, r_pl), (True, r_ar)):
            env = autoreset_env(3, 0) if auto else VecPlayEnv(gid, n, seed=3)
            env.reset()
            for i in range(5):
                env.step(A[i])
            out.append(gpu_ms(lambda i: env.step(A[i % args.steps]), args.steps))
            env.close()
    a, p = float(np.median(r_ar)), float(np.median(r_pl))
    print('rp_step %.4f ms, autoreset %.4f ms (medians; all: %s | %s): overhead %+.4f ms = %+.2f %%'
          % (p, a, ' '.join('%.4f' % v for v in r_pl), ' '.join('%.4f' % v for v in r_ar), a - p, 100 * (a - p) / p))


if __name__ == '__main__':
    main()
