"""The narrowphase at its shared caps, device against the CPU oracle (tests/crowded_scenes.py explains the caps and the scenes).

- One-kernel path, history-free: rp_debug_substep's contact list (k_debug_substep's collide()) against the fp32 oracle scene by scene - the same count, the
  same (ca, cb) sequence in the same order, points and distances within 5e-5, normals within 5e-4 - on the crowded scenes whose cap coverage
  tests/test_contact_caps.py asserts on the CPU, and against the fp64 oracle on the scenes where fp32 and fp64 agree on the pair list.
- Production path: the crowded scenes packed into one handle with empty caches, one rp_step holding the pose: the split, fused and chain pipelines give the
  same records and cache rows bit for bit, and each env's cache row is the fp32 oracle's after the same step within the lock-step's bounds
  (tests/test_gpu_dist_a.py).  pandaPlay-v0 runs the one-kernel path only.
- The contact fuzz (tools/contact_fuzz.py) as a test: shallow random scenes with equal pair lists, points and distances within 5e-5; deep ones with
  equal pair lists."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, 'oracle'), os.path.join(REPO, 'tools'), HERE) if p not in sys.path]
import cache_rows  # noqa: E402
import crowded_scenes as cs  # noqa: E402
from test_contact_caps import FLOORS, SCENES  # noqa: E402


def _record(o, kind):
    if kind == 'W':
        from test_gpu_parity import wide_record_from_oracle
        return wide_record_from_oracle(o)
    from gpu_debug import record_from_oracle
    return record_from_oracle(o)


def _device_list(env, o, kind, s):
    o.set_state(s)
    rec = _record(o, kind)
    o.set_state(s)
    env.set_state(torch.tensor(np.tile(rec, (2, 1))))
    dbg = env.debug_substep(0).numpy()
    n = int(dbg[0])
    return dbg[16:16 + 9 * n].reshape(n, 9).astype(np.float64)


def _gap(a, b):
    """points and distances [m], normals weighted by 0.1 (5e-5 on points = 5e-4 on normals): test_gpu_gjk_contacts.py's weighting"""
    if not len(a):
        return 0.0
    return max(float(np.abs(a[:, 2:5] - b[:, 2:5]).max()), float(np.abs(a[:, 8] - b[:, 8]).max()), 0.1 * float(np.abs(a[:, 5:8] - b[:, 5:8]).max()))


def _same_pairs(a, b):
    return len(a) == len(b) and np.array_equal(a[:, :2], b[:, :2])


@pytest.mark.parametrize('kind', ['U', 'V', 'P', 'W'])
def test_one_kernel_path_at_the_caps(kind):
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    scenes = [sc for sc in cs.generate(kind, SCENES, seed=0) if not sc['deep']]
    env = VecPlayEnv(cs.IDS[kind], 2, seed=7)
    o32 = OracleEnv(cs.IDS[kind], seed=7, f32=True)
    o64 = OracleEnv(cs.IDS[kind], seed=7)
    o32.reset()
    o64.reset()
    bad, bad_caps, worst, agree64, bad64, worst64 = [], {}, 0.0, 0, 0, 0.0
    for i, sc in enumerate(scenes):
        gc = _device_list(env, o32, kind, sc['state'])
        oc = sc['contacts']
        ok = _same_pairs(gc, oc) and _gap(gc, oc) <= 5e-5
        if ok:
            worst = max(worst, _gap(gc, oc))
        else:
            bad.append(i)
            for c in sc['crossed']:
                bad_caps[c] = bad_caps.get(c, 0) + 1
            if len(bad) <= 3:
                print('%s scene %d (crosses %s, counts %s): device %d contacts, oracle %d' % (kind, i, sorted(sc['crossed']), sc['counts'], len(gc), len(oc)))
                print(np.round(gc, 5)); print(np.round(oc, 5))
        o64.set_state(sc['state'])
        oc64 = o64.contacts()
        o64.set_state(sc['state'])
        if _same_pairs(oc64, oc) and _gap(oc64, oc) <= 1e-5:      # (where the two oracles agree - on a tied hull vertex they may pick other points)
            agree64 += 1
            if not (_same_pairs(gc, oc64) and _gap(gc, oc64) <= 5e-5):
                bad64 += 1
            else:
                worst64 = max(worst64, _gap(gc, oc64))
    cov = cs.coverage(scenes)
    print('%s: %d shallow crowded scenes, scenes that cross each cap %s; %d with another list on the device (by cap crossed: %s), worst gap of the rest %.1e; '
          'fp64 oracle: same pair list as fp32 on %d, %d of them with another list on the device, worst gap %.1e'
          % (kind, len(scenes), cov, len(bad), bad_caps, worst, agree64, bad64, worst64))
    for cap, floor in FLOORS[kind].items():
        assert cov[cap] >= floor, (cap, cov[cap])
    assert agree64 >= 0.9 * len(scenes)
    assert bad == [] and bad64 == 0


@pytest.mark.parametrize('kind', ['U', 'V', 'P'])
def test_production_path_at_the_caps(kind):
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    from gpu_debug import record_from_oracle
    scenes = [sc for sc in cs.generate(kind, SCENES, seed=0) if not sc['deep']]
    n = len(scenes)
    o = OracleEnv(cs.IDS[kind], seed=7, f32=True)
    o64 = OracleEnv(cs.IDS[kind], seed=7)                 # the twin: how far rounding alone moves the arm in one step from these scenes
    o.reset()
    o64.reset()
    na = o.n_arm
    recs, acts, rows_o, arm_o, arm_tw = [], [], [], [], []
    for sc in scenes:
        o.set_state(sc['state'])
        recs.append(record_from_oracle(o))
        o.set_state(sc['state'])
        a = cs.hold_action(o)
        acts.append(a)
        o.step(a)
        rows_o.append(o.get_cache_row())
        arm_o.append(o.get_state()[:na].copy())
        o64.set_state(sc['state'])
        o64.step(a)
        arm_tw.append(float(np.abs(o64.get_state()[:na] - arm_o[-1]).max()))
    recs, acts = torch.tensor(np.stack(recs)), torch.tensor(np.stack(acts), dtype=torch.float32)
    env = VecPlayEnv(cs.IDS[kind], n, seed=7)
    REC = 128
    out = {}
    for mode in (0, 1, 2):
        env.set_fused(mode)
        env.set_state(recs)
        env.step(acts)
        torch.cuda.synchronize()
        out[mode] = env.get_state().cpu()
    for mode in (1, 2):
        eq = (out[0].view(torch.int32) == out[mode].view(torch.int32)).all(dim=1)
        assert bool(eq.all()), '%s: split pipeline != %s (records and cache rows): first differing env %d' % (kind, ('fused', 'chain')[mode - 1], int(torch.nonzero(~eq)[0]))
    st = out[0].numpy()
    same = np.zeros(n, bool)
    d_arm = np.zeros(n)
    status = np.ascontiguousarray(st[:, 118]).view(np.int32)
    for e in range(n):
        rd, ro = st[e, REC:], rows_o[e]
        same[e] = cache_rows.manifolds(rd) == cache_rows.manifolds(ro) and cache_rows.gjk_tags(rd) == cache_rows.gjk_tags(ro)
        d_arm[e] = float(np.abs(st[e, :na] - arm_o[e]).max())
        if not same[e] and (~same).sum() <= 3:
            print('%s env %d (crosses %s): caches differ\n   device: %s\n   oracle: %s' % (kind, e, sorted(scenes[e]['crossed']), cache_rows.describe(rd), cache_rows.describe(ro)))
    ok = (status & 7) == 0
    arm_tw = np.array(arm_tw)
    a_dev, a_tw = float((d_arm[ok] > 1e-3).mean()), float((arm_tw[ok] > 1e-3).mean())
    crossing = np.array([bool(sc['crossed']) for sc in scenes])
    print('%s: %d envs (%d cross a cap), %d with a fault bit; cache rows equal to the oracle\'s (manifolds, GJK tags) in %.4f (%.4f of those that cross a cap); arm |dq| median %.1e, > 1e-3 in %.4f (fp64 twin against fp32: %.4f)'
          % (kind, n, crossing.sum(), (~ok).sum(), same[ok].mean(), same[ok & crossing].mean() if (ok & crossing).any() else float('nan'), np.median(d_arm[ok]), a_dev, a_tw))
    assert ok.mean() >= 0.98
    assert same[ok].mean() >= 0.97, same[ok].mean()
    if (ok & crossing).any():
        assert same[ok & crossing].mean() >= 0.9, same[ok & crossing].mean()
    assert np.median(d_arm[ok]) <= 1e-5
    assert a_dev <= 2.0 * a_tw + 0.01, (a_dev, a_tw)      # (test_gpu_dist_a.py's arm bound against its twin; contact-rich crowded scenes move the twin too)


@pytest.mark.parametrize('kind', ['U', 'P', 'V'])
def test_contact_fuzz(kind):
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    every = cs.generate(kind, 1200, seed=0, fuzz=True)
    scenes = [sc for sc in every if not sc['deep']][:300] + [sc for sc in every if sc['deep']]      # 300 shallow scenes, and the deep ones met on the way
    env = VecPlayEnv(cs.IDS[kind], 2, seed=7)
    o = OracleEnv(cs.IDS[kind], seed=7, f32=True)
    o.reset()
    bad, bad_deep, ndeep, touched, worst = 0, 0, 0, 0, 0.0
    for i, sc in enumerate(scenes):
        gc = _device_list(env, o, kind, sc['state'])
        oc = sc['contacts']
        deep = sc['deep'] or (len(gc) and float(gc[:, 8].min()) < -cs.DEEP)
        if deep:
            ndeep += 1
            bad_deep += int(not _same_pairs(gc, oc))
            continue
        touched += int(len(oc) > 0)
        if _same_pairs(gc, oc) and _gap(gc, oc) <= 5e-5:
            worst = max(worst, _gap(gc, oc))
        else:
            bad += 1
            if bad <= 3:
                print('%s fuzz scene %d: device %d contacts, oracle %d' % (kind, i, len(gc), len(oc)))
                print(np.round(gc, 5)); print(np.round(oc, 5))
    print('%s: %d fuzz scenes, %d deep (%d with another pair list), %d shallow with contacts; %d shallow with another list on the device, worst gap %.1e'
          % (kind, len(scenes), ndeep, bad_deep, touched, bad, worst))
    assert touched >= 50
    assert bad == 0 and bad_deep == 0
