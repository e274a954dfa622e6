"""The camera cases of tests/camera_cases.py on the CPU: that the table is fair before tests/test_gpu_camera_cases.py holds the device to it.  The float64 reference alone
- the same rays cast over the fp32 oracle's collider poses and over the fp64 oracle's - uses less than half of the 0.005 of the pixels the device is allowed to miss; every
case shows enough of the scene; the gripper camera's basis is the reference's formula and its cases cover the Euler angles that tell it from a fixed rotation of the link
frame; the ghost rule tints nothing but ghosted bodies when the sub-goal is the state itself."""
import functools

import numpy as np
import pytest

pytest.importorskip('scipy')

import camera_cases as cc      # noqa: E402
from oracle import euler_from_quat, quat_from_euler      # noqa: E402

measure = functools.lru_cache(maxsize=None)(cc.measure)


def is_gripper(case):
    return case[2] == 'gripper'


def test_the_reference_alone_stays_under_its_share_of_the_cap():
    """segmentation that differs between the fp32 and the fp64 oracle's poses, plus pixels where the float64 cast meets the surface at |n . d| < 0.02: at most 0.002 of
    every image.  A case that fails is replaced in the table; the cap stays."""
    worst = max(cc.cases(), key=lambda c: measure(c)['spread'])
    for case in cc.cases():
        m = measure(case)
        print(case, 'spread %.5f = %d differing + %d grazing pixels' % (m['spread'], m['differ'], m['graze']))
    assert measure(worst)['spread'] <= cc.SPREAD_CAP, (worst, measure(worst))


def test_every_case_shows_the_scene():
    """more than 5 % hit pixels and at least 6 colliders in view; from the gripper camera, which looks up past the arm's own wrist, at least 1 % and 2"""
    for case in cc.cases():
        m = measure(case)
        print(case, 'hits %.3f colliders %d' % (m['hits'], m['colliders']))
        if is_gripper(case):
            assert m['hits'] >= 0.01 and m['colliders'] >= 2, (case, m)
        else:
            assert m['hits'] > 0.05 and m['colliders'] >= 6, (case, m)


def test_table_shape():
    cases = cc.cases()
    assert len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == set(cc.IDS) and {c[2] for c in cases} == set(cc.CAMERA_NAMES)
    assert {c[3] for c in cases if not is_gripper(c)} == set(cc.SIZES) == {(70, 45), (33, 50)}
    assert {c[:3] for c in cases if c[3] == (200, 200)} == {(cc.U, s, 'gripper') for s in cc.GRIPPER_STATES}          # the one large size: the UR5's gripper camera
    assert {c[1] for c in cases if c[0] == cc.W2} == {'reset'} and max(c[4] for c in cases) < cc.NUM_ENVS <= 3
    for gid in (cc.U, cc.V):          # the states are what the table says they are
        rst, arm, scene = (cc.oracle_of(gid, s) for s in ('reset', 'arm', 'scene'))
        chain, free, joint = cc.state_layout(rst)
        moved = np.abs(arm.get_state()[:chain] - rst.get_state()[:chain])
        assert (moved > 0.2 - 1e-6).all() and (moved < 0.6 + 1e-6).all(), moved
        table = arm.arm_table()
        q = arm.get_state()[:arm.n_arm]
        assert (q >= table[:, 1]).all() and (q <= table[:, 2]).all()
        np.testing.assert_allclose(q[chain:], 0.5 * table[chain:, 2], atol=1e-6)          # the gripper half open
        s = scene.get_state()
        np.testing.assert_allclose([s[free + 13 + 1], *s[joint:joint + 3]], [-0.06, 0.12, 0.01, 1.5], atol=1e-7)
        assert s[free + 2] - rst.get_state()[free + 2] == pytest.approx(0.08, abs=1e-6) and (np.abs(s[free + 3:free + 7]) > 0.2).all()
        colours = lambda o: cc.collider_colours(o, o.colliders()[2])[o.colliders()[2][:, 7] > 0]      # noqa: E731
        assert not np.array_equal(colours(rst), colours(scene))          # the toggles recolour the globe and the grill
    rows = np.array([cc.ROWS[k] for k in ('yaw', 'distance', 'fov', 'aspect')])
    assert all(len(set(r)) == 3 for r in rows)


def test_gripper_basis_is_the_references_formula():
    rng = np.random.default_rng(3)
    rz = lambda a: np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])      # noqa: E731
    ry = lambda a: np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])      # noqa: E731
    for i in range(200):
        roll, pitch, yaw = rng.uniform(-np.pi, np.pi), rng.uniform(-1.2, 1.2), rng.uniform(-np.pi, np.pi)
        if i < 3:
            roll = (np.pi, 0.0, -np.pi)[i]
        quat = quat_from_euler([roll, pitch, yaw])
        f, s, u = cc.gripper_basis(np.zeros(3), quat)
        B = np.stack([f, s, u])
        np.testing.assert_allclose(B @ B.T, np.eye(3), atol=1e-12)
        np.testing.assert_allclose(np.cross(f, u), s, atol=1e-12)          # s = f x u: the camera's right
        # the closed form: f = Rz(yaw) Ry(pitch) z, u = Rz(yaw) Ry(pitch) (-cos roll, -sin roll, 0)
        np.testing.assert_allclose(f, rz(yaw) @ ry(pitch) @ [0, 0, 1], atol=1e-12)
        np.testing.assert_allclose(u, rz(yaw) @ ry(pitch) @ [-np.cos(roll), -np.sin(roll), 0], atol=1e-12)
        R = cc.quat_matrix(quat)
        if abs(abs(roll) - np.pi) < 1e-12:
            np.testing.assert_allclose(np.stack([f, u]), np.stack([-R[:, 2], R[:, 0]]), atol=1e-12)          # roll = pi: (-z, +x) of the link frame
            assert cc.basis_angle((f, s, u), cc.link_frame_basis(quat)) < 1e-5
        if roll == 0.0:
            np.testing.assert_allclose(np.stack([f, u]), np.stack([R[:, 2], -R[:, 0]]), atol=1e-12)          # roll = 0: (+z, -x)
            assert cc.basis_angle((f, s, u), cc.link_frame_basis(quat)) == pytest.approx(180.0, abs=1e-4)
    quat = quat_from_euler([np.pi - 0.3, 0.4, -0.7])
    assert cc.basis_angle(cc.gripper_basis(np.zeros(3), quat), cc.link_frame_basis(quat)) == pytest.approx(np.degrees(0.3), abs=1e-6)      # 17.19 degrees


def test_gripper_cases_cover_the_euler_angles():
    for gid in (cc.U, cc.V):
        eul = {s: euler_from_quat(cc.oracle_of(gid, s).site_pose(0)[1]) for s in cc.GRIPPER_STATES}
        print(gid, {s: np.round(e, 4) for s, e in eul.items()})
        assert abs(eul['reset'][0]) < 0.05                                                     # the reset pose: roll about 0, the link-frame basis is 180 degrees off
        assert np.pi - abs(eul['grip_pi'][0]) < 0.05                                           # where the link-frame basis is right
        for s in ('grip_a', 'grip_b'):
            assert 0.3 < abs(eul[s][0]) < 2.5 and (np.abs(eul[s]) > 0.1).all(), (s, eul[s])
    for case in cc.cases():
        if is_gripper(case):
            e = euler_from_quat(cc.oracle_of(case[0], case[1], case[4]).site_pose(0)[1])
            assert abs(e[1]) < 1.2, (case, e)                                                  # away from the Euler singularity


def test_ghosts_on_their_own_bodies_tint_only_those():
    """sub_goal == achieved_goal: whatever the ghost reference changes lies on pixels whose solid hit is a ghosted body; a block moved 12 cm aside tints pixels, and
    leaves depth and segmentation alone.  The achieved goal carries the dial as dial_to_0_1_range reads it and the reference writes a sub-goal's joint entries into the
    ghost's joints raw (environments.py:695-703), so with the dial away from 0 the ghost dial is another dial: in the 'scene' state the entry is put back to radians."""
    for gid, state in ((cc.U, 'reset'), (cc.U, 'scene'), (cc.V, 'reset'), (cc.W2, 'reset')):
        o = cc.oracle_of(gid, state)
        ag = np.array(o.calc_state()['achieved_goal'])
        o.clear_quat_memory()
        ag[-1] = o.get_state()[cc.state_layout(o)[2] + 2]
        cam = cc.host_camera('default', o)
        bare = cc.reference_layers(o, cam, 70, 45)
        g = cc.ghost_records(cc.sub_goal_oracle(gid, o, ag))
        same = cc.reference_layers(o, cam, 70, 45, ghosts=[g])
        changed = (cc.to_bytes(same['rgb']) != cc.to_bytes(bare['rgb'])).any(axis=2)
        print(gid, state, 'changed by ghosts on their bodies', int(changed.sum()), 'ghosted colliders', list(g[-1]))
        assert np.isin(bare['who'][changed], g[-1]).all()
        moved = np.array(ag)
        moved[0] += 0.12
        g2 = cc.ghost_records(cc.sub_goal_oracle(gid, o, moved))
        aside = cc.reference_layers(o, cam, 70, 45, ghosts=[g2])
        assert aside['tint'].sum() > 4 and (cc.to_bytes(aside['rgb']) != cc.to_bytes(bare['rgb'])).any(axis=2).sum() > 4          # (the block is some ten pixels at this size)
        assert np.array_equal(aside['z'], bare['z']) and np.array_equal(aside['seg'], bare['seg'])
