#!/usr/bin/env python3
"""Checksums of VecPlayEnv.render (rp_render / rp_render_ex) for test_rp_render_bits_of_the_parent in tests/test_gpu_render.py: per case the sha256 of get_state() -
which tells a differing scene from a differing picture - and the sha256 of the image bytes.  The cases are the shapes of tests/test_gpu_render_layers.py:

  sweep    UR5PlayAbsRPY1Obj-v0, 3 envs, seed 4, after reset() and again after 5 seeded random steps: the seven CAMERAS crossed with the four SIZES, and
           envs=(1, 3) at 70 x 45 (slot is not env)
  ghosts   a sub-goal on that handle (more than 64 records: two ballot rounds); pandaPlayAbsRPY1Obj-v0, 2 envs, seed 3: a ghost arm, a ghost arm with a sub-goal;
           pandaPlay-v0 (the wide build), 1 env, seed 2: bare and with a sub-goal; each at 200 x 200 and 70 x 45

Only the public Python surface is used, so the same script runs on any commit.  Run once at the commit whose images are the reference (it was: the parent of the
change that retired rp_render's own kernel of 256-pixel runs and moved it onto k_render_layers), on the device:
    python tools/render_goldens.py [tests/golden/render_parent_checksums.json] [--commit HASH]
The test recomputes run() and compares."""
import hashlib
import json
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

U, V, W2 = 'UR5PlayAbsRPY1Obj-v0', 'pandaPlayAbsRPY1Obj-v0', 'pandaPlay-v0'
SIZES = ((200, 200), (70, 45), (1, 1), (3, 130))          # (width, height)
GHOST_SIZES = ((200, 200), (70, 45))
CAMERAS = ('default', 'wide', 'gripper', 'fov170', 'fov1', 'close', 'away')
STEPS, ACTION_SEED = 5, 20251
OUT = os.path.join(REPO, 'tests', 'golden', 'render_parent_checksums.json')


def make_camera(env, name):
    """the cameras of tests/test_gpu_render_layers.py"""
    if name == 'default':
        return None
    if name == 'wide':
        return env.camera(distance=2.0, yaw=20.0, pitch=-40.0, fov=60.0, aspect=320 / 240)
    if name == 'gripper':
        return env.camera(gripper=True)
    blk = env.get_state()[0, 24:27].cpu().numpy().astype(float)
    edge = (blk + [0.0, -0.025, 0.025]).tolist()
    if name == 'fov170':
        return env.camera(target=edge, distance=0.6, fov=170.0)
    if name == 'fov1':
        return env.camera(target=edge, fov=1.0)
    if name == 'close':
        return env.camera(target=blk.tolist(), distance=0.09, yaw=40.0, pitch=-35.0)
    assert name == 'away'
    cam = env.camera()
    for k in range(3):
        cam.target[k] = 2.0 * cam.eye[k] - cam.target[k]
    return cam


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def run():
    """[{'case': name, 'state': sha256 of get_state(), 'image': sha256 of the image}, ...] in a fixed order"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    out = []

    def shot(env, name, **kw):
        out.append({'case': name, 'state': sha(env.get_state()), 'image': sha(env.render('rgb_array', **kw))})

    def sweep(env, stage):
        for cam in CAMERAS:
            c = make_camera(env, cam)
            for w, h in SIZES:
                shot(env, '%s %s %s %dx%d' % (U, stage, cam, w, h), width=w, height=h, camera=c)
        shot(env, '%s %s envs=(1, 3) 70x45' % (U, stage), width=70, height=45, envs=(1, 3))

    env = VecPlayEnv(U, 3, seed=4)
    obs = env.reset()
    sweep(env, 'reset')
    sg = obs['achieved_goal'].clone()
    sg[:, 0] += 0.12
    sg[:, 7] = -0.05
    for w, h in GHOST_SIZES:
        shot(env, '%s reset sub_goal %dx%d' % (U, w, h), width=w, height=h, sub_goal=sg)
    g = torch.Generator(device='cpu').manual_seed(ACTION_SEED)          # a ~ U(action space), the same numbers on every machine
    for _ in range(STEPS):
        env.step(((2 * torch.rand((3, 7), generator=g) - 1) * env.action_high.cpu()).to(env.device))
    sweep(env, 'stepped')
    env.close()

    panda = VecPlayEnv(V, 2, seed=3)
    pobs = panda.reset()
    ee = pobs['obs_quat'][:, 0:7]
    away = torch.cat([ee[:, 0:3] + torch.tensor([0.15, 0.0, 0.05], device=ee.device), ee[:, 3:7], torch.zeros((2, 1), device=ee.device)], 1)
    psg = pobs['achieved_goal'].clone()
    psg[:, 0] -= 0.1
    for w, h in GHOST_SIZES:
        shot(panda, '%s ghost_arm %dx%d' % (V, w, h), width=w, height=h, ghost_arm=away)
        shot(panda, '%s ghost_arm sub_goal %dx%d' % (V, w, h), width=w, height=h, ghost_arm=away, sub_goal=psg)
    panda.close()

    wide = VecPlayEnv(W2, 1, seed=2)
    wobs = wide.reset()
    wsg = wobs['achieved_goal'].clone()
    wsg[:, 0] += 0.1
    for w, h in GHOST_SIZES:
        shot(wide, '%s bare %dx%d' % (W2, w, h), width=w, height=h)
        shot(wide, '%s sub_goal %dx%d' % (W2, w, h), width=w, height=h, sub_goal=wsg)
    wide.close()
    return out


if __name__ == '__main__':
    args = sys.argv[1:]
    commit = None
    if '--commit' in args:
        k = args.index('--commit')
        commit = args[k + 1]
        del args[k:k + 2]
    if commit is None:
        commit = subprocess.run(['git', '-C', REPO, 'rev-parse', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    cases = run()
    res = {'commit': commit, 'steps': STEPS, 'action_seed': ACTION_SEED, 'cases': [c['case'] for c in cases], 'sha256': {c['case']: {'state': c['state'], 'image': c['image']} for c in cases}}
    path = args[0] if args else OUT
    with open(path, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path, len(cases), 'cases')
