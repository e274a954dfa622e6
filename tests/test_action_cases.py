"""The action stage's case table (tests/action_cases.py) against the CPU oracles alone: what tests/test_gpu_action.py relies on holds before any device is asked.

Every case runs on the fp64 oracle, the fp32 oracle and fp32 followers whose measured joints are 1 and 2 fp32 ulps off; the classes (exact / fuzzy / marginal / clean) come
from those runs only.  The caps below are conditions on the table (its seed was chosen to meet them), not measurements of anything under test.  The per-id table of
fp32-against-fp64 gaps is printed and compared with the committed profiles/action_stage_cpu_gaps.txt, where the GPU test takes its bounds from."""
import os

import numpy as np
import pytest

import action_cases as ac

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MARGINAL_SHARE = 0.08      # the reference alone stays this far under MARGINAL_CAP: the device may add cases of its own (its bit 16) and the sum is held to the cap
POSE_KINDS = {'near', 'mid', 'wide', 'far', 'clip', 'orient', 'joint', 'grip'}
JOINT_KINDS = POSE_KINDS - {'orient'}


def _all_runs(r):
    return [r['f64']] + r['followers']


@pytest.mark.parametrize('gid', list(ac.IDS))
def test_table_shape_and_edges(gid):
    """48 - 64 finite fp32 cases per id, every kind present, and the clip edges really sit at, an ulp inside and beyond action_space.high"""
    c = ac.build(gid)
    kinds, a, q = np.array(c['kinds']), c['a'], c['q']
    assert 48 <= len(kinds) <= 64 and a.dtype == np.float32 and q.dtype == np.float32
    assert np.isfinite(a).all() and np.isfinite(q).all()
    assert set(kinds) == (JOINT_KINDS if ac.IDS[gid] in ac.JOINT_TYPES else POSE_KINDS)
    hi = ac.action_high(gid)
    clip = a[kinds == 'clip']
    assert (np.abs(clip) == hi).any() and (np.abs(clip) == np.nextafter(hi, np.float32(0))).any() and (np.abs(clip) > 2 * hi).any()
    assert (np.abs(clip[:, -1]) == 1).any() and (np.abs(clip[:, -1]) > 1).any()
    grip = a[kinds == 'grip'][:, -1]
    assert {-1.0, 0.0, 1.0} <= set(grip.tolist()) and (grip > 1).any() and (grip < -1).any()
    assert np.array_equal(ac.clip_action(gid, a), np.minimum(np.maximum(a, -hi), hi))
    # joint edges: a measured joint within inc of one of goto_joint_poses' limits, inside and outside it
    ll, ul, inc = ac.LIMITS[ac.arm_of(gid)]
    nd = len(ll)
    qj = q[kinds == 'joint'][:, :nd]
    d = np.minimum(np.abs(qj - ll), np.abs(qj - ul))
    assert ((d < inc).any(axis=1)).sum() >= 4          # (two more sit 1.5 inc outside: there the two clamps disagree)
    assert ((qj > ul) | (qj < ll)).any() and ((qj < ul) & (qj > ll)).any()
    if ac.IDS[gid] in ac.JOINT_TYPES:          # joint actions exactly q + inc and q - inc, and an ulp either side of each
        cl = ac.clip_action(gid, a)[kinds == 'joint'][:, :nd]
        for sgn in (1, -1):
            for k in (0, 1, -1):
                step = np.float32(sgn) * inc
                if ac.IDS[gid] == 'absolute_joints':
                    assert any(np.array_equal(row, ac.ulps(qq + step, k)) for row, qq in zip(cl, qj)), (sgn, k)
                else:
                    assert any(np.array_equal(row, ac.ulps(step, k)) for row in cl), (sgn, k)
    else:                                      # m3_to_quat's branch change: two orient targets whose rotation has trace 0
        tr = c['trace0']
        assert len(tr) == 2 and all(kinds[i] == 'orient' and abs(t) < 1e-6 for i, t in tr.items()), tr


@pytest.mark.parametrize('gid', list(ac.IDS))
def test_reference_conditions(gid):
    """the classes' caps, the near cases' inactive clamps, the far cases' capped flag - on the oracles alone"""
    r = ac.reference(gid)
    kinds, cls = np.array(r['cases']['kinds']), np.array(r['cls'])
    joint_type = ac.IDS[gid] in ac.JOINT_TYPES
    print(gid, {k: int((cls == k).sum()) for k in ('exact', 'clean', 'marginal', 'fuzzy')})
    if joint_type:
        assert (cls == 'exact').all()
        for f in _all_runs(r):
            assert not f['capped'].any() and not f['window'].any() and (f['passes'] == 0).all()
    else:
        assert (cls == 'marginal').mean() <= REF_MARGINAL_SHARE <= ac.MARGINAL_CAP, list(kinds[cls == 'marginal'])
        far = kinds == 'far'
        assert ((cls == 'fuzzy') & far).sum() <= ac.FUZZY_CAP * far.sum(), int(((cls == 'fuzzy') & far).sum())
        assert ((cls == 'fuzzy') & ~far).sum() <= ac.FUZZY_CAP * (~far).sum(), list(kinds[(cls == 'fuzzy') & ~far])
        for f in _all_runs(r):
            assert f['capped'][far].all(), 'a far case whose last IK call met its residual test'
            # the IK's budget: UR5 4 x 20 loop passes, Panda 1 x 200; a call that is not capped has stopped at a residual test after its first pass
            budget = 200 if ac.arm_of(gid) == 'panda' else 80
            assert (f['passes'] <= budget).all() and (f['passes'][f['capped']] >= (200 if ac.arm_of(gid) == 'panda' else 20)).all()
    near = kinds == 'near'
    assert near.sum() >= 8 and set(cls[near]) <= {'exact', 'clean', 'marginal'}, set(cls[near])
    for f in _all_runs(r):
        assert np.array_equal(f['tp'][near], f['raw'][near]), 'a near case with an active clamp'


@pytest.mark.parametrize('gid', list(ac.IDS))
def test_perform_action_is_goto_of_raw(gid):
    """rpo_perform_action is unchanged: its clamped targets are goto_joint_poses of rpo_perform_action_raw's solution, bit for bit, in fp64 and in fp32 - and in
    fp32 they are the two np.clip calls of the reference on the limit tables as fp32 holds them, in that order"""
    r = ac.reference(gid)
    c = r['cases']
    nd = r['f64']['raw'].shape[1]
    for f in _all_runs(r):
        assert np.array_equal(f['tp'], f['tp_of_raw'])
    for k, f in zip(ac.NUDGES, r['followers']):
        q = ac.ulps(c['q'][:, :nd], k)
        raw32 = f['raw'].astype(np.float32)
        assert np.array_equal(raw32.astype(np.float64), f['raw'])
        assert np.array_equal(ac.goto_clamps(gid, raw32, q).astype(np.float64), f['tp'])
        assert np.array_equal(f['motor'][:, :nd], f['tp'])
    # the two clamps do not commute on this table: swapping them changes some case's targets
    ll, ul, inc = ac.LIMITS[ac.arm_of(gid)]
    q, raw32 = c['q'][:, :nd], r['f32']['raw'].astype(np.float32)
    swapped = np.minimum(np.maximum(np.minimum(np.maximum(raw32, q - inc), q + inc), ll), ul)
    assert not np.array_equal(swapped.astype(np.float64), r['f32']['tp'])
    if ac.IDS[gid] in ac.JOINT_TYPES:      # exact cases: one fp32 add (relative) or none
        a = r['clipped'][:, :nd]
        want = a + q if ac.IDS[gid] == 'relative_joints' else a
        assert np.array_equal(raw32, want)
    # a component beyond action_space.high is the component at it: the clip cases 'beyond' and 'at the bound' (same measured joints) agree in every bit
    i = np.where(np.array(c['kinds']) == 'clip')[0]
    assert np.array_equal(c['q'][i[1]], c['q'][i[3]]) and np.array_equal(r['f32']['raw'][i[1]], r['f32']['raw'][i[3]])


def test_gaps_table():
    """prints the per-id table and holds the committed profiles/action_stage_cpu_gaps.txt (the GPU test's bounds) to it (RP_WRITE_ACTION_GAPS=1 rewrites the file); the
    floors it implies are in fp32's range, not wider"""
    rows = {gid: ac.gap_row(gid) for gid in ac.IDS}
    text = ac.format_gaps(rows)
    print(text)
    assert ac.parse_gaps(text).keys() == ac.IDS.keys()
    path = os.path.join(REPO, ac.GAPS_FILE)
    if os.environ.get('RP_WRITE_ACTION_GAPS') == '1':      # after a change of the table or the oracle: rewrite the committed file, on purpose
        with open(path, 'w') as f:
            f.write(text)
    with open(path) as f:
        committed = ac.parse_gaps(f.read())
    # the committed table (the GPU test's bounds) is this one: the same counts, the figures within 5 % (another libm's last bits; the bounds are 3 - 4 times them)
    fresh = ac.parse_gaps(text)
    assert committed.keys() == fresh.keys()
    for gid in fresh:
        for col in ac.GAPS_COLUMNS:
            want, got = fresh[gid][col], committed[gid][col]
            assert got == want if col in ac.GAPS_COLUMNS[:4] else abs(got - want) <= 0.05 * want, (gid, col, got, want)
    for gid, row in ac.parse_gaps(text).items():
        if ac.IDS[gid] in ac.JOINT_TYPES:
            assert row['clean'] == row['marginal'] == row['fuzzy'] == 0
            continue
        # fp32 against fp64 on a converged IK: some 1e-7 in the middle; the 99th percentile (the device's floor is four times it) stays well under the 1e-3 at
        # which a case counts as fuzzy, and a marginal stop ends within 1e-3 by construction
        assert row['clean_median'] < 1e-6 and row['clean_p99'] < 1e-4 and row['marginal_max'] <= ac.FUZZY_GAP, (gid, row)
