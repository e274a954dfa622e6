"""The device's dynamics stage against an independent float64 model (tests/arm_truth.py; cases and the fp32 oracle's gaps in tests/arm_cases.py; the CPU half is
tests/test_arm_truth.py).  Run with -m gpu -s on the MI355X box to see the gaps (profiles/arm_truth_gpu.txt).

Every bound is arm_cases.bound(kind, quantity) = max(3 x the fp32 oracle's worst gap on the same cases, the floor of test_gpu_kinematics.py: 1e-6 on positions, angles
and E_M, 1e-5 on velocities); 3 x is the project's allowance for another evaluation order (test_gpu_contact_truth.py).  Gaps: E_M = max |Minv_dev M_ref - I|; tau, v*,
twists and velocities |x - ref| / max(1, |ref|) per entry; positions and joint angles absolute; orientations as rotation matrices.

- Stage half (rp_debug_substep: arm_dynamics + unconstrained_velocities as every pipeline instantiates them): M^-1, tau and v* of every dof - the arm's, the free
  bodies' linear and angular, the scene joints' - per case; the records are unchanged by the calls.
- Observation half (rp_calc_state): the end effector's position, orientation and `velocity`, `joints`, the gripper entry and the velocity entries of obs_quat where
  the id has them, against FK and the site Jacobian; one pose with qd = e_j per env reads every column of the Jacobian on its own.
- Production half: the usable free-fall cases with every motor off and a hold action, one rp_step under the split pipeline with one and with three env groups, the
  fused step and the chain - records bit-identical across the four, arm q and qd at the golden end state, no arm contact (the row counts' flag where the model has
  no drawer - the flag counts the drawer's rail contacts too -, the end state's contact list everywhere), half of the envs under a tilted gravity.  The handle has
  192 envs, eight copies of the 24 cases: rp_step forms three groups only from 129 envs up.  Then, motors on again, the tumbling blocks after one step against their
  golden end states (x, quaternion as its rotation matrix, v, w)."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, 'oracle'), HERE) if p not in sys.path]
import arm_cases as ac  # noqa: E402
import arm_truth as at  # noqa: E402

KINDS = ['U', 'V', 'P', 'W']
COPIES = 8
REC = 128          # floats of a state record; a state row's contact cache lies behind it
_SHARED = {}


def shared(kind):
    """computed once per kind and left unchanged: model, cases, golden entries, per-case references, the usable free-fall cases and their hold actions (CPU only)"""
    if kind not in _SHARED:
        from oracle import OracleEnv
        from roboticsplayroompybullet_amd import vec_env
        model = vec_env._model(kind)
        with open(os.path.join(HERE, 'golden', 'arm_truth.json')) as f:
            golden = json.load(f)[kind]
        s0 = ac.scene0(kind)
        cs = ac.cases(kind, model)
        o64 = OracleEnv(ac.IDS[kind], seed=7)
        o64.reset()
        use = [i for i in range(ac.N_FREEFALL) if ac.usable(cs[i], golden['ff'][str(i)]['room'], o64, s0)]
        refs = [ac.stage_reference(model, c, golden['c'][str(i)]) for i, c in enumerate(cs)]
        hold = []
        for c in cs:
            o64.set_state(ac.freefall_state(c, s0))
            hold.append(ac.hold_action(o64))
        tb = ac.tumbles(kind, model, s0)
        tb_hold = []
        for s in tb:
            o64.set_state(s)
            tb_hold.append(ac.hold_action(o64))
        _SHARED[kind] = dict(model=model, golden=golden, s0=s0, cases=cs, use=use, refs=refs, hold=hold, tumbles=tb, tb_hold=tb_hold, flags=o64.flags(),
                             dims=(model['n_arm'], len(model['free']), len(model['joint1'])))
    return _SHARED[kind]


def place_cases(env, sh):
    """every case as an env: state, gravity, wrenches, masses"""
    n, nf, nj = sh['dims']
    cs = sh['cases']
    kin = [ac.kin_of(ac.state_of(c), n, nf, nj) for c in cs]
    env.set_kinematics(pos=np.stack([k[0] for k in kin]), vel=np.stack([k[1] for k in kin]), clear_contacts=True)
    env.set_actuation(gravity=np.stack([c['gravity'] for c in cs]).astype(np.float32))
    env.set_wrench(np.stack([c['wrench'] for c in cs]).astype(np.float32))
    if nf:
        env.set_dynamics(mass=np.stack([c['mass'] for c in cs]).astype(np.float32))


def report(kind, what, worst, where):
    print('%s %s: %s' % (kind, what, '  '.join('%s %.1e (bound %.1e, case %s)' % (k, worst[k], ac.bound(kind, k), where[k]) for k in worst)))
    bad = {k: (worst[k], ac.bound(kind, k), where[k]) for k in worst if not worst[k] <= ac.bound(kind, k)}
    assert not bad, '%s %s beyond its bound: %s' % (kind, what, bad)


def track(worst, where, gaps, i):
    for k, v in gaps.items():
        if k not in worst or v > worst[k]:
            worst[k], where[k] = v, i


@pytest.mark.parametrize('kind', KINDS)
def test_stage_against_the_reference(kind):
    from roboticsplayroompybullet_amd import VecPlayEnv
    sh = shared(kind)
    n, nf, nj = sh['dims']
    nv = n + 6 * nf + nj
    env = VecPlayEnv(ac.IDS[kind], ac.N_CASES, seed=7)
    env.reset()
    place_cases(env, sh)
    before = env.get_state().cpu()
    worst, where = {}, {}
    for i, ref in enumerate(sh['refs']):
        dbg = env.debug_substep(i).numpy().astype(np.float64)
        Minv = dbg[320:320 + 144].reshape(12, 12)[:n, :n]
        gaps = ac.stage_gaps(ref, n, Minv, dbg[512:512 + n], dbg[480:480 + nv], None, None, None)
        track(worst, where, gaps, i)
        if not all(gaps[k] <= ac.bound(kind, k) for k in gaps):
            print('%s case %d (%s): %s; cond(M) %.1e' % (kind, i, sh['cases'][i]['tag'], {k: '%.1e' % v for k, v in gaps.items()}, np.linalg.cond(ref['M'])))
    after = env.get_state().cpu()
    diff = before.view(torch.int32) != after.view(torch.int32)
    print('%s: words changed by the %d rp_debug_substep calls: %d in the records, %d in the contact caches behind them'
          % (kind, ac.N_CASES, int(diff[:, :REC].sum()), int(diff[:, REC:].sum())))
    report(kind, 'stage', worst, where)
    assert not bool(diff[:, :REC].any()), 'rp_debug_substep changed a record'


@pytest.mark.parametrize('kind', KINDS)
def test_observation_against_the_reference(kind):
    from roboticsplayroompybullet_amd import VecPlayEnv
    sh = shared(kind)
    n, nf, nj = sh['dims']
    arm = at.Arm(sh['model'])
    fl = sh['flags']
    env = VecPlayEnv(ac.IDS[kind], ac.N_CASES, seed=7)
    env.reset()
    place_cases(env, sh)
    obs = {k: v.cpu().numpy().astype(np.float64) for k, v in env.calc_state().items() if isinstance(v, torch.Tensor)}
    grip_dof = arm.dof_of_joint(9 if sh['model']['arm_type'] == 'Panda' else 18)
    grip_scale = 1.0 if sh['model']['arm_type'] == 'Panda' else 23.0
    o_vel, o_orn = 3, 3 + 3 * fl['return_velocity']
    o_grip = o_orn + 4 * fl['use_orientation']
    worst, where = {}, {}
    for i, (c, ref) in enumerate(zip(sh['cases'], sh['refs'])):
        oq = obs['obs_quat'][i]
        gaps = {'ee_pos': max(ac.abs_gap(oq[:3], ref['ee_pos']), ac.abs_gap(obs['controllable_achieved_goal'][i, :3], ref['ee_pos'])),
                'ee_twist': ac.rel_gap(obs['velocity'][i], ref['ee_twist'])}
        if fl['use_orientation']:
            gaps['ee_rot'] = ac.abs_gap(at.quat_rot(oq[o_orn:o_orn + 4]), ref['ee_rot'])
            assert abs(np.linalg.norm(oq[o_orn:o_orn + 4]) - 1.0) <= 1e-6
        if fl['return_velocity']:
            gaps['ee_twist'] = max(gaps['ee_twist'], ac.rel_gap(oq[o_vel:o_vel + 3], ref['ee_twist'][:3]))
        joints = np.array([c['q'][arm.dof_of_joint(j)] if arm.dof_of_joint(j) >= 0 else 0.0 for j in range(8)])
        assert ac.abs_gap(obs['joints'][i], joints) <= 1e-6, (i, obs['joints'][i], joints)
        assert abs(oq[o_grip] - grip_scale * c['q'][grip_dof]) <= 1e-6 and abs(obs['controllable_achieved_goal'][i, 3] - grip_scale * c['q'][grip_dof]) <= 1e-6, i
        track(worst, where, gaps, i)
    # every column of the site Jacobian on its own: the pose of case 16 (joints anywhere in their ranges) in n_arm envs, qd = e_j in env j
    c = sh['cases'][ac.GROUPS['range'][0]]
    kin = ac.kin_of(ac.state_of(c), n, nf, nj)
    vel = np.tile(kin[1], (ac.N_CASES, 1))
    vel[:n, :n] = np.eye(n, dtype=np.float32)
    mask = (np.arange(ac.N_CASES) < n).astype(np.uint8)
    env.set_kinematics(pos=np.tile(kin[0], (ac.N_CASES, 1)), vel=vel, mask=mask)
    v = env.calc_state()['velocity'].cpu().numpy().astype(np.float64)
    ref = sh['refs'][ac.GROUPS['range'][0]]
    J = np.vstack([ref['Jv'], ref['Jw']])
    for j in range(n):
        track(worst, where, {'ee_twist': ac.rel_gap(v[j], J[:, j])}, 'column %d' % j)
    assert np.count_nonzero(np.abs(J).max(axis=0) > 1e-3) >= 6      # (the columns are there to be read: at least the six joints below the site move it)
    report(kind, 'observation', worst, where)


@pytest.mark.parametrize('kind', KINDS)
def test_production_step_in_free_fall_and_tumbling_blocks(kind):
    from roboticsplayroompybullet_amd import VecPlayEnv
    sh = shared(kind)
    n, nf, nj = sh['dims']
    cs, use, N = sh['cases'], sh['use'], COPIES * ac.N_CASES
    assert len(use) * 4 >= 3 * ac.N_FREEFALL
    tilted = [i for i in use if cs[i]['gravity'][0] != 0.0]
    assert abs(2 * len(tilted) - len(use)) <= 2      # half of the envs that count fall under a tilted gravity (every other case does; an unusable one or two shift it)
    env = VecPlayEnv(ac.IDS[kind], N, seed=7)
    env.reset()
    kin = [ac.kin_of(ac.freefall_state(c, sh['s0']), n, nf, nj) for c in cs] * COPIES
    env.set_kinematics(pos=np.stack([k[0] for k in kin]), vel=np.stack([k[1] for k in kin]), clear_contacts=True)
    env.set_actuation(gravity=np.stack([c['gravity'] for c in cs] * COPIES).astype(np.float32), motor_strength=np.zeros((N, n), dtype=np.float32))
    env.set_wrench(np.stack([ac.freefall_wrench(c) for c in cs] * COPIES).astype(np.float32))
    acts = torch.tensor(np.stack(sh['hold'] * COPIES), dtype=torch.float32)
    start = env.get_state().clone()
    out, kins, rows = {}, {}, None
    for name, fused, groups in (('split, one group', 0, 1), ('split, three groups', 0, 3), ('fused', 1, None), ('chain', 2, None)):
        env.set_fused(fused)
        if groups is not None:
            env.set_groups(groups)
        env.set_state(start)
        env.step(acts)
        torch.cuda.synchronize()
        out[name] = env.get_state().cpu()
        kins[name] = {k: v.cpu().numpy().astype(np.float64) for k, v in env.get_kinematics().items()}
        if name == 'split, one group':
            rows = env.debug_row_counts().numpy()
    ref = out['split, one group']
    for name, st in out.items():
        eq = (ref.view(torch.int32) == st.view(torch.int32)).all(dim=1)
        assert bool(eq.all()), '%s: split pipeline with one group != %s: first differing env %d' % (kind, name, int(torch.nonzero(~eq)[0]))
    pos, vel = kins['split, one group']['pos'], kins['split, one group']['vel']
    # no arm contact: the row counts' flag says "a contact in the arm's half of the velocity layout", where the rotation-locked drawer lives too and always rests on
    # its rails - so the flag is asked where the model has no such body, and everywhere the contact list of the end state (rp_debug_substep) names no arm collider
    row0_body = any(b.get('rot_locked') for b in sh['model']['free'])
    arm_col = [1 <= c['body'] <= n for c in sh['model']['col']]
    for i in use:
        dbg = env.debug_substep(i).numpy()
        pairs = dbg[16:16 + 9 * int(dbg[0])].reshape(-1, 9)[:, :2].astype(int)
        assert not any(arm_col[a] or arm_col[b] for a, b in pairs), 'case %d: an arm contact after the free fall: %s' % (i, pairs.tolist())
    worst, where = {}, {}
    for e in range(N):
        i = e % ac.N_CASES
        if i not in use:
            continue
        assert row0_body or rows[e, 2] == 0, 'env %d (case %d): an arm contact in free fall' % (e, i)
        g = sh['golden']['ff'][str(i)]
        track(worst, where, {'ff_q': ac.abs_gap(pos[e, :n], g['q']), 'ff_qd': ac.rel_gap(vel[e, :n], g['qd'])}, i)
        assert np.array_equal(pos[e, :n], pos[i, :n]) and np.array_equal(vel[e, :n], vel[i, :n]), 'env %d is not its copy %d' % (e, i)
    moved = max(np.abs(pos[i, :n] - cs[i]['q']).max() for i in use)
    assert moved > 0.02      # (the arms did fall: a step that stood still would not be compared with anything)
    # the tumbling blocks, motors on again, under the default pipeline
    env.set_fused(0)
    env.set_actuation(gravity=np.array(ac.GRAVITY[0], dtype=np.float32), motor_strength=np.ones(n, dtype=np.float32))
    env.set_wrench(None)
    env.set_state(start)
    tk = [ac.kin_of(s, n, nf, nj) for s in sh['tumbles']]
    reps = N // ac.N_TUMBLE
    env.set_kinematics(pos=np.stack([k[0] for k in tk] * reps), vel=np.stack([k[1] for k in tk] * reps), clear_contacts=True)
    env.step(torch.tensor(np.stack(sh['tb_hold'] * reps), dtype=torch.float32))
    torch.cuda.synchronize()
    k1 = {k: v.cpu().numpy().astype(np.float64) for k, v in env.get_kinematics().items()}
    for e in range(N):
        t = e % ac.N_TUMBLE
        free = np.concatenate([k1['pos'][e, n:n + 7 * nf].reshape(nf, 7), k1['vel'][e, n:n + 6 * nf].reshape(nf, 6)], axis=1)
        track(worst, where, ac.tumble_gaps(sh['model'], free, sh['golden']['tb'][str(t)]), 'tumble %d' % t)
    report(kind, 'production', worst, where)
