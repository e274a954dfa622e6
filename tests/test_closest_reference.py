"""The float64 truth of closest_points on the CPU (tests/closest_cases.py): the golden D* file regenerates, the closed forms agree with the Minkowski route where both
apply, the conditions the GPU test relies on hold, and the fp32 allowance - D* with every pose record and hull vertex rounded to float32 - reproduces
closest_cases.FP32_WORST.  No device, no GJK: the truth is the facets of the Minkowski difference (contact_truth.signed_distance)."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
pytest.importorskip('scipy')
import closest_cases as cc  # noqa: E402
import contact_truth as ct  # noqa: E402

KINDS = tuple(cc.IDS)
CLASSES = ('box-box', 'hull-box', 'hull-hull', 'sphere-box')


@functools.lru_cache(maxsize=None)
def truth(kind):
    return cc.Truth(kind)


@functools.lru_cache(maxsize=None)
def pairs_of(kind):
    tr = truth(kind)
    return cc.pairs_of(kind, tr.scene(cc.poses_of(kind)[0]), tr.o.n_free)


@functools.lru_cache(maxsize=None)
def golden():
    return cc.load_golden()


def test_the_golden_names_the_ids_the_poses_and_the_asked_pairs():
    g = golden()
    assert set(g) == set(KINDS)
    assert os.path.getsize(cc.GOLDEN) < 1 << 20
    for kind in KINDS:
        e = g[kind]
        assert e['id'] == cc.IDS[kind] and tuple(e['poses']) == cc.poses_of(kind)
        assert len(e['dstar']) == len(cc.poses_of(kind)) and all(len(d) == e['n_pairs'] for d in e['dstar'])
        assert 1 <= e['n_pairs'] <= 4096
        tr = truth(kind)
        assert len(pairs_of(kind)) == e['n_pairs']
        if kind == 'W':
            continue
        assert e['tags'] == [tr.all_poses[i][0] for i in cc.poses_of(kind)]
        # the asked pairs hold the model's pair table, every arm-link pair and the block against the scene
        asked = {(min(a, b), max(a, b)) for a, b in pairs_of(kind)}
        sc = tr.scene(cc.poses_of(kind)[0])
        arm = [c for c in range(len(sc.cols)) if sc.is_arm(c)]
        assert {(min(a, b), max(a, b)) for a, b in tr.tables['pairs']} <= asked
        assert {(a, b) for i, a in enumerate(arm) for b in arm[i + 1:]} <= asked


@pytest.mark.parametrize('kind', KINDS)
def test_a_few_poses_regenerate_the_golden(kind):
    e = golden()[kind]
    tr = truth(kind)
    pairs = pairs_of(kind)
    P = cc.poses_of(kind)
    for k in ((0, 2, len(P) - 1) if kind != 'W' else (0,)):      # 5 mm into the table, 5 mm into a link, the last pose
        d = tr.dstar(tr.scene(P[k]), pairs)
        gap = float(np.abs(np.array(d) - np.array(e['dstar'][k])).max())
        print('%s pose %d: regenerated against the golden, worst gap %.3e' % (kind, P[k], gap))
        assert gap <= 0.51 * cc.UNIT      # (the golden keeps integers of cc.UNIT)


def test_the_closed_forms_agree_with_the_minkowski_route_on_boxes():
    """sphere against hull and sphere against sphere are closed forms of this helper; on a BOX read as the hull of its corners both routes exist: the facets of the
    Minkowski difference (a one-vertex 'hull' for the centre), contact_truth's own sphere-box form, and point_hull_signed"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(60):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        he = rng.uniform(0.01, 0.2, size=3)
        p = rng.normal(size=3) * 0.1
        box = ct.Shape('box', 0.0, R=R, p=p, he=he)
        as_hull = ct.Shape('hull', 0.0, V=box.V)
        c = p + R @ (he * rng.uniform(-1.6, 1.6, size=3))      # inside and outside
        r = float(rng.uniform(0.0, 0.05))
        sphere = ct.Shape('point', r, p=c)
        a = cc.signed_distance(sphere, as_hull)                                       # this helper's closed form
        b = ct.signed_distance(sphere, box)                                           # contact_truth's sphere-box form
        m = ct.signed_distance(ct.Shape('hull', r, V=c.reshape(1, 3)), as_hull)       # the Minkowski route
        worst = max(worst, abs(a - b), abs(a - m), abs(cc.signed_distance(as_hull, sphere) - a))
        # sphere against sphere: against a box of 1e-9 half extents around the other centre
        c2 = c + rng.normal(size=3) * 0.1
        s2 = ct.Shape('point', 0.02, p=c2)
        tiny = ct.Shape('box', 0.02, R=np.eye(3), p=c2, he=np.full(3, 1e-9))
        assert abs(cc.signed_distance(sphere, s2) - ct.signed_distance(sphere, tiny)) <= 2e-9
    print('closed forms against the Minkowski route: worst gap %.3e' % worst)
    assert worst <= 1e-12


def test_the_conditions_the_gpu_test_relies_on():
    """at most 2 % of the (pose, pair) cases lie within BAND of zero - the status comparison leaves out no more -, and every pair class has separated and overlapping
    cases"""
    signs = {c: [0, 0] for c in CLASSES}
    for kind in KINDS:
        e = golden()[kind]
        d = np.array(e['dstar'])
        share = float((np.abs(d) < cc.BAND).mean())
        print('%s: %d cases, %.3f %% within BAND of zero' % (kind, d.size, 100 * share))
        assert share <= 0.02
        sc = truth(kind).scene(cc.poses_of(kind)[0])
        cls = [cc.pair_class(cc.shape_of(sc, a), cc.shape_of(sc, b)) for a, b in pairs_of(kind)]
        for j, c in enumerate(cls):
            if c in signs:
                signs[c][0] += int((d[:, j] > cc.BAND).sum())
                signs[c][1] += int((d[:, j] < -cc.BAND).sum())
    print('separated / overlapping cases per class: %s' % signs)
    for c in CLASSES:
        assert signs[c][0] > 0 and signs[c][1] > 0, (c, signs[c])


@pytest.mark.parametrize('kind', KINDS)
def test_the_fp32_allowance_reproduces_its_entry(kind):
    """D* with every pose record and hull vertex rounded to float32 before the float64 distance, against the golden: the worst gap is at most FP32_WORST's entry and no
    less than a quarter of it.  The device's bound is max(3 x entry, 2e-6)."""
    e = golden()[kind]
    tr = truth(kind)
    pairs = pairs_of(kind)
    worst = 0.0
    for k, i in enumerate(cc.poses_of(kind)):
        d32 = tr.dstar(tr.scene(i), pairs, rounded=True)
        worst = max(worst, float(np.abs(np.array(d32) - np.array(e['dstar'][k])).max()))
    print('%s: fp32 inputs against D*, worst gap %.3e (entry %.1e, device bound %.1e)' % (kind, worst, cc.FP32_WORST[kind], cc.device_bound(kind)))
    assert 0.25 * cc.FP32_WORST[kind] <= worst <= cc.FP32_WORST[kind]
    assert cc.device_bound(kind) == max(3 * cc.FP32_WORST[kind], 2e-6)
