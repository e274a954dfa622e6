"""What the scenes of tests/test_gpu_prep2_tail.py cover, by the fp32 oracle's own counters (no GPU): the set of both ids together holds every case of
prep2_tail_scenes.CASES - a contact list of 0, of 8 and of 9 contacts (the end of k_prep2's first chunk of contact rows), 11 manifolds (PM_MAX), 4 torsional
rows (MAXT), a manifold created and one leaving in the second substep.

The long lists - 16 and 17 contacts (the end of the second chunk) and 21 with more wanted, MAXC's cut falling inside a manifold - lie beyond what the crowded scenes
of the one-object ids give (their longest list: 12).  prep2_tail_scenes.seeded() reaches them in the persistent model from rollout states with padded caches, and
prep2_tail_scenes.wide() in the stateless model at a contact margin of 0.05; both sets are asserted here to hold each of the three."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, 'oracle'), HERE) if p not in sys.path]
import prep2_tail_scenes as pts  # noqa: E402


def test_the_scenes_cover_the_tail_s_cases():
    sets = {kind: pts.select(kind) for kind in ('U', 'V')}
    total = {case: 0 for case in pts.CASES}
    for kind, scenes in sets.items():
        assert len(scenes) == pts.PICK, (kind, len(scenes))
        cov = pts.coverage(scenes)
        print(kind, cov, 'longest lists', max(len(sc['contacts']) for sc in scenes), max(len(sc['contacts2']) for sc in scenes))
        for case, n in cov.items():
            total[case] += n
    for case, n in total.items():
        assert n >= 1, (case, total)
    for kind in sets:                                           # either id sees manifolds come and go in its second substep
        cov = pts.coverage(sets[kind])
        assert cov['created'] >= 1 and cov['left'] >= 1, (kind, cov)


def test_the_long_lists_are_there():
    for name, fn in (('seeded', pts.seeded), ('wide', pts.wide)):
        total = {case: 0 for case in pts.LONG_CASES}
        for kind in ('U', 'V'):
            scenes = fn(kind)
            print(name, kind, [(sorted(pts.long_cases_of(sc)), len(sc['contacts']), sc['counts']['contacts'], sc['counts']['torsional']) for sc in scenes])
            for sc in scenes:
                for case in pts.long_cases_of(sc):
                    total[case] += 1
        for case, n in total.items():
            assert n >= 1, (name, case, total)
    # the persistent model's cut is inside a manifold (two or three of its four points listed), not between two
    assert any(sc['cut'] for kind in ('U', 'V') for sc in pts.seeded(kind))
