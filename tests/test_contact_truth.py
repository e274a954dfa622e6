"""The narrowphase's contacts against float64 geometry, pose by pose, on the CPU: the fp64 oracle, the fp32 oracle and the frozen reference step at the poses of
tests/contact_poses.py go through the certificates of tests/contact_truth.py (C1 - C4 per contact, P1 - P3 per pair against the exact signed distance D*).  The truth
runs no narrowphase code of the project; what it knows of the model are shapes, poses, the baked pair table and the documented rules (contact_truth's docstring).

`python tests/test_contact_truth.py --write` regenerates tests/golden/contact_truth.json (D* per pose and pair within reach: the GPU test reads it, scipy is only
needed here) and profiles/contact_truth_cpu.txt (the three tables).

What the truth found when it was first run ("The contacts against float64 geometry"): the broadphase box of a hull collider lacks the hull's
0.001 margin, so a link between `threshold` and `threshold + 0.001` (by its OBB) from a box is never handed to the narrowphase (a finger tip 0.6 mm over the table
top) - documented as the rule `culled`, its misses counted as `culled_near`; and EPA's round cap binds by rounding (contact_poses.epa_may_cap)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import contact_poses as cp  # noqa: E402
import contact_truth as ct  # noqa: E402
from contact_poses import contact_list  # noqa: E402
import oracle  # noqa: E402
from oracle import OracleEnv  # noqa: E402

pytest.importorskip('scipy')
KINDS = ('U', 'P', 'V', 'W')
CAPS = {'pairs': 64, 'candidates': 64, 'manifolds': 11, 'contacts': 21, 'torsional': 4}      # MAX_ACTIVE_PAIRS, MAX_CANDIDATES, PM_MAX, MAX_CONTACTS, MAX_TORS
# fp64 bounds (metres): rounding level.  Measured worst 9.5e-11 (a hull vertex table held in float32, FK and the detector in another operation order than numpy's)
FP64_BOUND = {c: 1e-9 for c in ct.CHECKS}
PROFILE = os.path.join(os.path.dirname(HERE), 'profiles', 'contact_truth_cpu.txt')


@functools.lru_cache(maxsize=None)
def run(kind):
    """everything the tests of one id share: poses, scenes, D*, and the three readings' reports"""
    tables = ct.model_tables(kind)
    o64 = OracleEnv(kind, seed=7, env_index=0)
    o64.reset()
    poses = cp.poses(kind, o64)
    scenes, dstars = [], []
    for tag, s in poses:
        o64.set_state(s)
        sc = ct.Scene.from_oracle(tables, o64)
        scenes.append(sc)
        dstars.append(ct.dstar_for(sc))
    out = dict(poses=poses, scenes=scenes, dstar=dstars, lists={}, reports={}, stats={}, counts={})
    for name, kw in (('fp64', {}), ('fp32', dict(f32=True)), ('reference step', dict(bullet_ref=True))):
        o = OracleEnv(kind, seed=7, env_index=0, **kw)
        o.reset()
        rep = ct.Report()
        lists, stats, counts = [], [], []
        for i, (tag, s) in enumerate(poses):
            oc, st, cc = contact_list(o, s)
            if name == 'reference step':
                st['capped'] = True                          # (its EPA has its own iteration limits; one-sided like a capped call)
            ct.check_pose(scenes[i], oc, dstars[i], rep, '%s pose %d (%s)' % (kind, i, tag), epa_capped=st['capped'])
            lists.append(oc)
            stats.append(st)
            counts.append(cc)
        out['lists'][name], out['reports'][name], out['stats'][name], out['counts'][name] = lists, rep, stats, counts
    return out


def _show(rep, bounds):
    bad = sorted(rep.exceed(bounds), key=lambda f: -f[2])
    return '%d beyond the bounds; the worst:\n' % len(bad) + '\n'.join('  %s %s %.3e  %s' % f for f in bad[:12])


@pytest.mark.parametrize('kind', KINDS)
def test_fp64_oracle_is_within_rounding_of_the_truth(kind):
    r = run(kind)
    rep = r['reports']['fp64']
    print(rep.table('%s fp64 oracle' % kind))
    assert not rep.exceed(FP64_BOUND), _show(rep, FP64_BOUND)
    assert rep.worst_of('P2') <= 1e-9 and rep.worst_of('P3') == 0.0


@pytest.mark.parametrize('kind', KINDS)
def test_fp32_oracle_sizes_the_device_bounds(kind):
    """the fp32 oracle through the same checks: no missing or surplus contact (P3 is discrete), and its worst gap per check is what contact_poses.FP32_WORST says -
    the block the device's bounds are made from (at most the constant, and the constant no more than 1.5 x the measurement + 1e-9)"""
    r = run(kind)
    rep = r['reports']['fp32']
    print(rep.table('%s fp32 oracle' % kind))
    assert rep.worst_of('P3') <= 1e-9, _show(rep, dict(FP64_BOUND, C1=1, C2=1, C3=1, P1=1, P2=1))
    for c in ct.CHECKS:
        w, k = rep.worst_of(c), cp.FP32_WORST[kind][c]
        print('%s %s: measured %.3e, constant %.3e' % (kind, c, w, k))
        assert w <= k <= 1.5 * w + 1e-9, (kind, c, w, k)


@pytest.mark.parametrize('kind', KINDS)
def test_poses_cover_the_classes_below_the_caps(kind):
    r = run(kind)
    rep = r['reports']['fp64']
    tags = [t for t, _ in r['poses']]
    assert len(tags) == cp.N_POSES
    for fam, n in (('flat', 24), ('edge45', 12), ('corner', 12), ('overhang', 12), ('crossed', 12), ('link_face', 16), ('link_rim', 8), ('link_edge', 20), ('grasp', 8),
                   ('arm_table', 12)) + ((('blocks', 16), ) if kind == 'W' else ()) + ((('sphere', 8), ) if kind != 'P' else ()):
        assert tags.count(fam) >= n, (fam, tags.count(fam))
    n = {k[1]: v for k, v in rep.count.items() if k[0] == 'P2'}
    print(kind, 'pairs with a contact per class:', n, ' D* signs (negative, positive) per rule class:', rep.dstar_signs)
    need = dict(box_face=100, box_edge=5, vface=30, gjk=5)
    need.update(dict(obb_for_epa=5) if kind == 'U' else dict(epa_cap=3, epa=10))
    if kind != 'P':
        need['sphere'] = 4
    if kind == 'V':
        assert rep.dstar_signs.get('culled_near', [0, 0])[1] >= 1, 'no pose left at which the broadphase culls a hull pair whose shapes are within the threshold'
    for cls, k in need.items():
        assert n.get(cls, 0) >= k, (cls, n.get(cls, 0), k)
    # both signs of D* per shape class
    sg = rep.dstar_signs
    neg = lambda names: sum(sg.get(c, [0, 0])[0] for c in names)
    pos = lambda names: sum(sg.get(c, [0, 0])[1] for c in names)
    groups = [('box_face', 'box_edge', 'box_apart', 'obb_face', 'obb_edge'), ('vface', 'vface_tie', 'gjk', 'epa', 'obb_for_epa', 'hull_apart')] + ([('sphere', )] if kind != 'P' else [])
    for names in groups:
        assert neg(names) >= 4 and pos(names) >= 4, (names, neg(names), pos(names))
    st = r['stats']['fp64']
    gjk, epa, capped = sum(s['gjk_contacts'] for s in st), sum(s['epa_calls'] for s in st), sum(s['capped'] for s in st)
    print('%s: %d GJK contacts, %d EPA calls (%d gave up) in %d rounds, %d poses with a call that may have ended at the round cap' %
          (kind, gjk, epa, sum(s['epa_gave_up'] for s in st), sum(s['epa_rounds'] for s in st), capped))
    assert gjk >= 5
    assert (epa == 0) if kind == 'U' else (epa >= 20 and capped >= 3), (epa, capped)
    assert sum(s['epa_gave_up'] for s in st) == 0
    # marginal pairs and caps
    assert rep.marginal <= 0.10 * rep.pairs, (rep.marginal, rep.pairs)
    for name in ('fp64', 'fp32'):
        for i, cc in enumerate(r['counts'][name]):
            for k, cap in CAPS.items():
                assert cc[k] <= cap, (kind, name, i, tags[i], cc)


@pytest.mark.parametrize('kind', KINDS)
def test_golden_distances_are_reproduced(kind):
    r = run(kind)
    with open(ct.GOLDEN) as f:
        g = json.load(f)[kind]
    assert len(g) == len(r['dstar'])
    for i, (row, ds) in enumerate(zip(g, r['dstar'])):
        assert [(a, b) for a, b, _ in row] == sorted(ds), i
        for a, b, d in row:
            assert abs(d - ds[(a, b)]) <= 1e-10, (i, a, b, d, ds[(a, b)])


def test_reference_step_and_profile_file():
    """the frozen reference step through the same checks: reported, nothing asserted about its gaps (nobody may change it); and the recorded tables are there"""
    for kind in KINDS:
        print(run(kind)['reports']['reference step'].table('%s reference step (report only)' % kind))
    text = open(PROFILE).read()
    for kind in KINDS:
        for name in ('fp64 oracle', 'fp32 oracle', 'reference step'):
            assert '%s %s' % (kind, name) in text


# ---------------------------------------------------------------------------------------------------------------- the truth notices injected faults
def _first_pose(r, fam, pred):
    for i, (tag, _) in enumerate(r['poses']):
        if tag == fam and pred(r['lists']['fp64'][i]) and not r['stats']['fp64'][i]['capped']:      # (a capped EPA call is held from one side only)
            return i
    raise AssertionError('no pose of family %s for the injection' % fam)


def _check(r, i, lst):
    rep = ct.Report()
    ct.check_pose(r['scenes'][i], lst, r['dstar'][i], rep, 'injected', epa_capped=r['stats']['fp64'][i]['capped'])
    return rep


@pytest.mark.parametrize('fam', ['flat', 'corner', 'link_face', 'link_edge'])
def test_truth_detects_injected_faults(fam):
    """on the fp64 oracle's own list (which passes): one normal flipped, 1e-4 added to one distance, one pair's contacts dropped, one point moved 1 mm off its face -
    each must push a check beyond the fp32-sized bound the DEVICE is held to (the loosest bound in use), not just beyond rounding"""
    r = run('P')
    bound = {c: max(3 * cp.FP32_WORST['P'][c], 2e-6) for c in ct.CHECKS}
    i = _first_pose(r, fam, lambda l: len(l) >= 1 and any(int(x[0]) == 17 for x in l))
    lst = r['lists']['fp64'][i]
    assert not _check(r, i, lst).exceed(bound)
    k = int(np.argmin(np.where(lst[:, 0] == 17, lst[:, 8], np.inf)))      # the block's deepest contact
    flipped = lst.copy()
    flipped[k, 5:8] *= -1
    assert {f[0] for f in _check(r, i, flipped).exceed(bound)} & {'C4'}
    farther = lst.copy()
    farther[k, 8] += 1e-4
    assert {f[0] for f in _check(r, i, farther).exceed(bound)} & {'C3', 'P2'}
    dropped = lst[~((lst[:, 0] == lst[k, 0]) & (lst[:, 1] == lst[k, 1]))]
    assert {f[0] for f in _check(r, i, dropped).exceed(bound)} & {'P3', 'P2'}
    moved = lst.copy()
    moved[k, 2:5] += 1e-3 * lst[k, 5:8]
    assert 'C3' in {f[0] for f in _check(r, i, moved).exceed(bound)}


# ---------------------------------------------------------------------------------------------------------------- regeneration
def _write():
    golden, text = {}, []
    for kind in KINDS:
        r = run(kind)
        golden[kind] = [[[a, b, float(repr(d))] for (a, b), d in sorted(ds.items())] for ds in r['dstar']]
        st = r['stats']['fp64']
        text.append('%s: %d poses, %d pairs within reach; fp64 oracle: %d GJK contacts, %d EPA calls in %d rounds, %d poses with a call that may have ended at the round cap' %
                    (kind, len(r['poses']), r['reports']['fp64'].pairs, sum(s['gjk_contacts'] for s in st), sum(s['epa_calls'] for s in st), sum(s['epa_rounds'] for s in st),
                     sum(s['capped'] for s in st)))
        for name in ('fp64', 'fp32', 'reference step'):
            rep = r['reports'][name]
            text.append(rep.table('%s %s' % (kind, name + (' oracle' if name != 'reference step' else ' (report only)'))))
            bad = sorted(rep.exceed(FP64_BOUND if name == 'fp64' else {c: 1e-4 for c in ct.CHECKS}), key=lambda f: -f[2])
            for f in bad[:6]:
                text.append('    beyond %s: %s %s %.3e  %s' % ('1e-9' if name == 'fp64' else '1e-4', f[0], f[1], f[2], f[3][:200]))
        text.append('')
    with open(ct.GOLDEN, 'w') as f:
        json.dump(golden, f, separators=(',', ':'))
    with open(PROFILE, 'w') as f:
        f.write('Contacts against float64 geometry (tests/test_contact_truth.py --write): worst gap per check and class, metres; 0 = inside the certificate.\n'
                'Classes: contact_truth.py.  P3 gaps are 1.0 for a missing / surplus contact.\n\n' + '\n'.join(text))
    print('\n'.join(text))


if __name__ == '__main__':
    if '--write' in sys.argv:
        _write()
