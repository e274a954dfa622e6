"""The action stage alone (k_action's body through rp_debug_action) against the CPU oracles, case by case: clip, the six action types, the cooperative IK, the two clamps,
motor targets and status bits 8 / 16 - on tests/action_cases.py's table, whose classes and bounds come from the reference alone (tests/test_action_cases.py,
profiles/action_stage_cpu_gaps.txt).

    exact cases (joint action types)   raw solution, clamped targets and every motor target word bit-equal to the fp32 oracle
    clean cases                        |raw - fp64 oracle| <= max(4 x the id's clean 99th percentile on the CPU, 3 x the followers' gap) per joint
    marginal cases                     the reference's, plus every clean case in which the device sets bit 16; together at most 10 % of an id; 3 x the id's largest
                                       marginal gap on the CPU
    fuzzy cases                        3 x the followers' gap; they stand outside the marginal share (a cap of their own, CPU test); bit 8 is compared where every
                                       CPU run agrees on it
    every case                         clamp(clamp(raw_dev, ll, ul), q +- inc) in fp32 numpy == the device's targets == the oracle's goto_joint_poses(raw_dev), bit for bit;
                                       the gripper's motor targets equal the fp32 oracle's; the hook's flags are the status word's bits 8 / 16

Then, bitwise and without an oracle: every case gives the same bits whatever its row in the wave, its wave mates (the id's slowest / fastest cases among them), the
number of envs (partial last waves), the group cut and a ranked member table (the hook reports every env's place: the test sees that the table is a permutation and not
the identity); and a real step gives the same targets and bits 8 / 16 in all three pipelines and group counts as the hook did, both as a pipeline's first step (identity
order) and as its third (ranked by the second step's loads).

The group / member layouts and the pipeline comparison use a handle of 192 envs (the table three times over): under 129 envs rp_step never cuts more than one group."""
import functools
import os

import numpy as np
import pytest

import action_cases as ac

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_MTARGET, ST_STATUS = 68, 118          # csrc/rp_device_model.h (the narrow record: every one-object id)
W = 64                                   # envs of the main handle: the table, padded with its first case


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


_ENVS = {}


def _close_envs():
    for env, _, _ in _ENVS.values():
        env.close()
    _ENVS.clear()


@pytest.fixture(scope='module', autouse=True)
def _handles():
    yield
    _close_envs()


def _env(gid, n):
    """one handle per size while the tests stay with one id, with the state after reset() kept to put back"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    if any(g != gid for g, _ in _ENVS):
        _close_envs()
    if (gid, n) not in _ENVS:
        env = VecPlayEnv(gid, n, seed=3)
        env.reset()
        _ENVS[(gid, n)] = (env, env.get_state().clone(), env.get_kinematics()['pos'].clone())
    return _ENVS[(gid, n)]


def _place(gid, n, idx, forget=True):
    """the handle of n envs with env e in case idx[e]'s measured joints (everything else as after reset()); returns (env, actions tensor).  forget: back to the split
    pipeline with one group and no member table (changing the pipeline forgets it: identity order until a step has run); otherwise pipeline, groups and the table the
    latest step left stay as they are"""
    import torch
    c = ac.build(gid)
    env, s0, kin0 = _env(gid, n)
    assert len(idx) == n
    if forget:
        env.set_fused(1); env.set_fused(0); env.set_groups(1)
    env.set_state(s0)
    kin = kin0.clone()
    kin[:, :c['q'].shape[1]] = torch.tensor(c['q'][idx], device=kin.device)
    env.set_kinematics(pos=kin)
    return env, torch.tensor(c['a'][idx])


def _read(env, nd, raw, flags, places):
    import torch
    torch.cuda.synchronize()
    st = env.get_state().cpu().numpy()
    status = st[:, ST_STATUS].copy().view(np.int32)
    return {'place': places.cpu().numpy().copy(), 'raw': raw.cpu().numpy()[:, :nd].copy(), 'flags': flags.cpu().numpy().copy(), 'tp': st[:, ST_MTARGET:ST_MTARGET + nd].copy(),
            'motor': st[:, ST_MTARGET:ST_MTARGET + 12].copy(), 'status': status & 24}


def _hook(gid, n, idx):
    """debug_action on the n-env handle in layout idx: per env the raw solution, the flags, the clamped targets, the motor target words and status bits 8 / 16"""
    env, a = _place(gid, n, idx)
    got = _read(env, ac.LIMITS[ac.arm_of(gid)][0].shape[0], *env.debug_action(a, places=True))
    assert np.array_equal(got['place'], np.arange(n)), 'no step yet: identity order'
    return got


def _identity(gid):
    n = len(ac.build(gid)['kinds'])
    return np.concatenate([np.arange(n), np.zeros(W - n, dtype=np.int64)])


@functools.lru_cache(maxsize=None)
def _base(gid):
    return _hook(gid, W, _identity(gid))


def _assert_cases_equal(gid, idx, got, what):
    """every env of layout idx carries the bits its case has in the identity layout"""
    base = _base(gid)
    for k in ('raw', 'flags', 'tp', 'motor', 'status'):
        g, b = got[k], base[k][idx]
        bad = np.where(_bits(g).reshape(len(idx), -1) != _bits(b).reshape(len(idx), -1))[0] if g.dtype == np.float32 else np.where(g != b)[0]
        assert len(bad) == 0, '%s: %s differs for envs %s (cases %s)' % (what, k, sorted(set(bad.tolist()))[:8], sorted(set(np.asarray(idx)[bad].tolist()))[:8])


@functools.lru_cache(maxsize=None)
def _cpu_gaps():
    with open(os.path.join(REPO, ac.GAPS_FILE)) as f:
        return ac.parse_gaps(f.read())


@pytest.mark.parametrize('gid', list(ac.IDS))
def test_cases_against_oracle(gid):
    import oracle
    r = ac.reference(gid)
    c, f32, f64 = r['cases'], r['f32'], r['f64']
    n = len(c['kinds'])
    kinds, cls = np.array(c['kinds']), np.array(r['cls'])
    nd, n_arm = f64['raw'].shape[1], c['q'].shape[1]
    dev = {k: v[:n] for k, v in _base(gid).items()}
    row = _cpu_gaps()[gid]
    capped, marginal = (dev['status'] & 8) != 0, (dev['status'] & 16) != 0
    # the hook's flags are what the stage wrote into the status word
    assert np.array_equal(dev['flags'] & 1, capped.astype(np.int32)) and np.array_equal(dev['flags'] >> 1, marginal.astype(np.int32))
    err = np.abs(dev['raw'].astype(np.float64) - f64['raw'])
    # --- every case: the clamps, from the device's own raw solution, without a tolerance
    want_tp = ac.goto_clamps(gid, dev['raw'], c['q'][:, :nd])
    assert _same(want_tp, dev['tp']), np.where(_bits(want_tp) != _bits(dev['tp']))
    o = oracle.OracleEnv(gid, f32=True)
    o.reset()
    for i in range(n):
        o.set_arm_q(c['q'][i].astype(np.float64))
        assert _same(o.goto_joint_poses(dev['raw'][i].astype(np.float64)), dev['tp'][i]), i
    # the gripper's motor targets (and, the clamped targets being those words, all of them where the raw solutions agree)
    assert _same(f32['motor'][:, nd:], dev['motor'][:, nd:n_arm]), np.where(_bits(f32['motor'][:, nd:]) != _bits(dev['motor'][:, nd:n_arm]))
    # --- per class
    cls_dev = cls.copy()
    cls_dev[(cls == 'clean') & marginal] = 'marginal'
    share = (cls_dev == 'marginal').mean()
    floor = 4 * row['clean_p99']
    bound = np.zeros_like(err)
    bound[cls_dev == 'clean'] = np.maximum(floor, 3 * r['gap'])[cls_dev == 'clean']
    bound[cls_dev == 'marginal'] = 3 * row['marginal_max']
    bound[cls_dev == 'fuzzy'] = (3 * r['gap'])[cls_dev == 'fuzzy']
    e1 = err.max(axis=1)
    stat = lambda m: 'n %2d median %.2e p99 %.2e max %.2e' % (m.sum(), np.median(e1[m]), np.percentile(e1[m], 99), e1[m].max()) if m.any() else 'n  0'
    print('%-28s device - fp64: clean [%s]  marginal [%s; %d by the device\'s bit 16; share %.3f]  fuzzy [%s]  | CPU: floor %.2e, marginal bound %.2e'
          % (gid, stat(cls_dev == 'clean'), stat(cls_dev == 'marginal'), int(((cls == 'clean') & marginal).sum()), share, stat(cls_dev == 'fuzzy'), floor,
             3 * row['marginal_max']))
    for i in np.where((err > bound).any(axis=1) & (cls != 'exact'))[0]:
        print('   over its bound: case %d (%s, %s%s) err %s bound %s' % (i, kinds[i], cls[i], ' -> marginal' if cls_dev[i] != cls[i] else '', err[i], bound[i]))
    if ac.IDS[gid] in ac.JOINT_TYPES:
        assert (cls == 'exact').all()
        assert _same(f32['raw'], dev['raw']) and _same(f32['tp'], dev['tp']) and _same(f32['motor'], dev['motor'][:, :n_arm])
        assert not marginal.any() and np.array_equal(capped, f32['capped'])
        return
    assert share <= ac.MARGINAL_CAP, (share, list(np.where(cls_dev == 'marginal')[0]))
    assert (err <= bound).all(), [(int(i), kinds[i], cls_dev[i], float(e1[i])) for i in np.where((err > bound).any(axis=1))[0]]
    # --- status bits
    # (clean cases, and the fuzzy ones on which every CPU run agrees: a target pi away ends elsewhere in every run, and converges in every run)
    runs = np.array([f['capped'] for f in [f64] + r['followers']])
    cl = (cls_dev == 'clean') | ((cls_dev == 'fuzzy') & (runs == runs[0]).all(axis=0))
    assert np.array_equal(capped[cl], f32['capped'][cl]), np.where(cl & (capped != f32['capped']))
    assert capped[kinds == 'far'].all()
    every = np.all([f['window'] for f in r['followers']], axis=0)
    assert marginal[every].all(), np.where(every & ~marginal)


def _big(gid):
    """192 envs: the table in identity, reversed and stride-permuted order"""
    ident = _identity(gid)
    return np.concatenate([ident, ident[::-1], ident[_stride_perm(W)]])


def _assert_ranked(place):
    """the places the hook reports are a permutation of the envs, and not the identity: the launch went by a ranked member table"""
    assert np.array_equal(np.sort(place), np.arange(len(place))), 'not a permutation'
    moved = int((place != np.arange(len(place))).sum())
    print('   ranked member table: %d of %d envs off their own place, %d in another wave' % (moved, len(place), int((place // 4 != np.arange(len(place)) // 4).sum())))
    assert moved >= len(place) // 4, moved


@functools.lru_cache(maxsize=None)
def _stride_perm(n):
    """a permutation of range(n) (n a multiple of 4) after which every case sits in another row of its wave and with three other mates"""
    for k in range(5, n, 2):
        for b in range(1, n):
            idx = (np.arange(n) * k + b) % n
            if len(set(idx.tolist())) != n:
                continue
            pos = np.argsort(idx)                      # pos[c]: where case c sits
            ok = all(pos[c] % 4 != c % 4 and not ({int(x) for x in idx[pos[c] // 4 * 4: pos[c] // 4 * 4 + 4]} - {c}) & set(range(c // 4 * 4, c // 4 * 4 + 4))
                     for c in range(n))
            if ok:
                return idx
    raise AssertionError('no stride permutation')


@pytest.mark.parametrize('gid', list(ac.IDS))
def test_wave_mates_and_layouts(gid):
    """a case's bits do not depend on its row, its mates (or their iteration counts), a partial last wave, the group cut or the member table"""
    r = ac.reference(gid)
    n = len(r['cases']['kinds'])
    ident = _identity(gid)
    _assert_cases_equal(gid, ident, _hook(gid, W, ident), 'identity again')
    _assert_cases_equal(gid, ident[::-1].copy(), _hook(gid, W, ident[::-1].copy()), 'reversed')
    sp = ident[_stride_perm(W)]
    _assert_cases_equal(gid, sp, _hook(gid, W, sp), 'stride permutation')
    passes = r['f32']['passes']
    for what, mate in (('slowest', int(np.argmax(passes))), ('fastest', int(np.argmin(passes)))):
        for lo in range(0, n, 16):                   # sixteen cases per launch, each with three copies of `mate`, its own row moving along
            idx = np.full(W, mate, dtype=np.int64)
            for w, case in enumerate(range(lo, min(lo + 16, n))):
                idx[4 * w + w % 4] = case
            _assert_cases_equal(gid, idx, _hook(gid, W, idx), '%s mates (case %d), cases %d..' % (what, mate, lo))
    for m in (W - 3, W - 2, W - 1):                  # 4k + 1, 4k + 2, 4k + 3: the dead rows of the last wave run on the launch's first env
        idx = (np.arange(m) + 5 * (W - m)) % n
        _assert_cases_equal(gid, idx, _hook(gid, m, idx), 'N = %d' % m)
    # three groups (cut at 25 / 60 % of 192 envs: no multiple of four), first in identity order ...
    big = _big(gid)
    env, a = _place(gid, 3 * W, big)
    env.set_groups(3)
    nd = r['f64']['raw'].shape[1]
    got = _read(env, nd, *env.debug_action(a, places=True))
    assert np.array_equal(got['place'], np.arange(3 * W))
    _assert_cases_equal(gid, big, got, 'three groups, identity order')
    # ... then by a ranked member table: the first step of a pipeline runs in identity order and leaves load classes, the second ranks the envs by them (k_member)
    # and leaves that ranking behind.  The places the hook reports are then a permutation that is not the identity, and every case still has its bits.
    for _ in range(2):
        env.step(a)
    _place(gid, 3 * W, big, forget=False)
    got = _read(env, nd, *env.debug_action(a, places=True))
    _assert_ranked(got['place'])
    _assert_cases_equal(gid, big, got, 'three groups, ranked member table')


@pytest.mark.parametrize('gid', list(ac.IDS))
def test_pipelines_at_the_edges(gid):
    """a real step from the table's joints and actions: target_poses and status bits 8 / 16 are the same bits in the split pipeline (one group, three groups), the
    fused kernel and the chained one - and the ones debug_action gave; in identity order and under a ranked member table"""
    import torch
    big = _big(gid)
    base = _base(gid)
    nd = base['tp'].shape[1]

    def compare(env, a, what):
        _, _, _, info = env.step(a)
        torch.cuda.synchronize()
        tp, status = info['target_poses'].cpu().numpy(), info['status'].cpu().numpy() & 24
        assert _same(tp, base['tp'][big]), ('target_poses', what, np.where(_bits(tp) != _bits(base['tp'][big]))[0][:8])
        assert np.array_equal(status, base['status'][big]), ('status', what, np.where(status != base['status'][big])[0][:8])

    for fused, groups in ((0, 1), (0, 3), (1, 1), (2, 1)):
        env, a = _place(gid, 3 * W, big)
        env.set_fused(fused); env.set_groups(groups)
        compare(env, a, (fused, groups, 'first step: identity order'))
        if fused == 1:                       # (k_step: one env per block, no member table)
            continue
        # the step after a second one is cut by a ranking (k_member on the second step's load classes): the same cases from the same joints again
        env.step(a)
        _place(gid, 3 * W, big, forget=False)
        compare(env, a, (fused, groups, 'third step: ranked'))
        _place(gid, 3 * W, big, forget=False)
        got = _read(env, nd, *env.debug_action(a, places=True))      # (the table that third step went by, as the hook sees it)
        _assert_ranked(got['place'])
        _assert_cases_equal(gid, big, got, 'hook after %s' % ((fused, groups),))
    env.set_fused(0); env.set_groups(1)
