#!/usr/bin/env python3
"""Checksums of the production step for tests/test_gpu_prep2_tail.py: md5 of rp_get_state (state records and contact-cache rows, every word) after every
step of a seeded rollout - N = 256 envs, 12 steps of distribution B (bench.py's action ranges) and then, from a fresh handle, 12 steps of distribution A
(a ~ U(action space)) - for the UR5 and the Panda one-object play ids (crowded_scenes' U and V).

Run once at the commit whose results are the reference (it was: the parent of the k_prep2 tail change), on the device:
    python tools/prep2_tail_goldens.py            # writes tests/golden/prep2_tail_checksums.json
The test recomputes run() and compares.  Nothing k_prep2 does may move a bit of either; the order of k_solve2's heavy list may differ from run to run and
the results do not depend on it."""
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

IDS = {'U': 'UR5PlayAbsRPY1Obj-v0', 'V': 'pandaPlayAbsRPY1Obj-v0'}
N, STEPS, SEED = 256, 12, 20250
B_LO = [-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0]      # bench.py's distribution B (both ids stand in the same scene)
B_HI = [0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0]
OUT = os.path.join(REPO, 'tests', 'golden', 'prep2_tail_checksums.json')


def actions(dist, high):
    """[STEPS, N, 7] on the host, from a CPU generator (the same numbers on every machine)"""
    g = torch.Generator(device='cpu').manual_seed(SEED + (1 if dist == 'A' else 0))
    u = torch.rand((STEPS, N, 7), generator=g)
    if dist == 'A':
        return (2 * u - 1) * high.cpu()
    lo, hi = torch.tensor(B_LO), torch.tensor(B_HI)
    return lo + (hi - lo) * u


def run(kind):
    """{'A': [md5 after step 1, ...], 'B': [...]} of id `kind`"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    out = {}
    for dist in ('B', 'A'):
        env = VecPlayEnv(IDS[kind], N, seed=SEED)
        env.reset()
        acts = actions(dist, env.action_high).to(env.device)
        sums = []
        for k in range(STEPS):
            env.step(acts[k])
            s = env.get_state()
            torch.cuda.synchronize()
            sums.append(hashlib.md5(s.cpu().contiguous().numpy().tobytes()).hexdigest())
        out[dist] = sums
        env.close()
    return out


if __name__ == '__main__':
    res = {'n_envs': N, 'steps': STEPS, 'seed': SEED, 'ids': IDS, 'md5': {k: run(k) for k in IDS}}
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)
