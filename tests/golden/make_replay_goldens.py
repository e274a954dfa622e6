#!/usr/bin/env python3
"""Write tests/golden/replay_fake_<env id>.json: fixtures from the PyBullet half of tools/pybullet_replay.py (dump_from_pybullet), run through
the REFERENCE'S OWN env classes against fake_bullet.StaticWorldClient.  No physics: `source` = "fake", a sample of the fixture format, never a pin.
tests/test_pybullet_golden.py holds them to the tool's FORMAT and to the sections the fixture's consumers read.

    python tests/golden/make_replay_goldens.py --reference-root /path/to/RoboticsPlayroomPybullet

Needs the reference repository; rerun it whenever pybullet_replay.FORMAT or the sections of a fixture change.
"""
import argparse
import json
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CASES = (('UR5PlayAbsRPY1Obj-v0', 'random'), ('pandaPick-v0', 'grasp'))


def fixture_path(env_id):
    return os.path.join(HERE, 'replay_fake_%s.json' % env_id)


def dump_one(reference_root, env_id, scenario):
    """one fixture, in a process of its own (install_stubs replaces pybullet and gym in sys.modules)"""
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import fake_bullet
    gold = json.load(open(os.path.join(HERE, 'assets_independent.json')))

    def joint_types(model):       # Bullet's joint order: depth-first, children in XML order (pybullet: 0 revolute, 1 prismatic, 4 fixed)
        out = []

        def visit(link):
            for j in model['joints']:
                if j['parent'] == link:
                    out.append({'revolute': 0, 'continuous': 0, 'prismatic': 1}.get(j['type'], 4))
                    visit(j['child'])
        visit(model['root'])
        return out
    fake_bullet.UR5_JOINT_TYPES, fake_bullet.PANDA_JOINT_TYPES = joint_types(gold['ur5']), joint_types(gold['panda'])
    fake_bullet.install_stubs([], fake_bullet.StaticWorldClient)
    import pybullet_replay
    args = types.SimpleNamespace(env=env_id, steps=4, seed=0, scenario=scenario, reference_root=reference_root, dump=fixture_path(env_id),
                                 source_label='fake')
    pybullet_replay.dump_from_pybullet(args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference-root', required=True, help='checkout of the reference repository')
    ap.add_argument('--one', nargs=2, metavar=('ENV', 'SCENARIO'), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        dump_one(os.path.abspath(a.reference_root), *a.one)
        return
    for env_id, scenario in CASES:
        subprocess.run([sys.executable, os.path.abspath(__file__), '--reference-root', a.reference_root, '--one', env_id, scenario], check=True)


if __name__ == '__main__':
    main()
