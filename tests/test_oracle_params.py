"""The CPU oracle's per-instance parameters - friction, mass, wrenches, gravity, motor gain and strength (rpo_set_friction .. rpo_set_motor; the HIP library's per-env
tables) - held by closed forms, on the CPU.  tests/test_gpu_param_lockstep.py holds the device to this oracle in contact; an oracle that merely mirrored the kernels would
share their mistakes, so everything here is derived from the physics the tables stand for, not from the other implementation:

  1. the defaults, and other values set and set back, move no bit in either precision;
  2. a free body in the air follows the substep recurrence under its own gravity, force, torque and mass;
  3. the arm's accelerations change by M^-1 (J_com^T f + J_w^T t) under a wrench and by M^-1 sum_i m_i J_com_i^T dg under a gravity change (Jacobians by central
     differences of the oracle's forward kinematics);
  4. friction sets the slide distance; a pair friction beyond 10 slides as 10 does;
  5. a collision keeps the momentum the masses give; a block that tips on its edge turns as the baked block does while its contact impulse scales with its mass - which
     needs the inertia to scale with the mass;
  6. strength 0 switches a motor off; the motor's first impulse is M_eff (0.1 gain) e / dt, clipped at the bound times strength;
  7. the control of the GPU lock-step: its three scenarios, free-running on the fp32 oracle, move by more than ten times the lock-step's bound when one value block is put
     back to its default - a device that ignored a block could not pass there.
"""
import functools
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_rows  # noqa: E402
import param_scenarios as ps  # noqa: E402
from tolerances import N_MAIN  # noqa: E402

pytest.importorskip('torch')
DT, KP, KD = 1.0 / 300.0, 0.1, 0.04


def _oracle(kind, f32=False, **kw):
    from oracle import OracleEnv
    return OracleEnv(kind, seed=ps.SEED, f32=f32, **kw)


def _block_to(o, pos, quat=(0.0, 0.0, 0.0, 1.0), vel=(0.0, 0.0, 0.0), om=(0.0, 0.0, 0.0), body=0):
    s = o.get_state()
    f0 = 2 * o.n_arm + 13 * body
    s[f0:f0 + 13] = list(pos) + list(quat) + list(vel) + list(om)
    o.set_state(s)


def _free(o, body=0):
    s = o.get_state()
    return s[2 * o.n_arm + 13 * body:2 * o.n_arm + 13 * body + 13]


# ---------------------------------------------------------------- 1. defaults and round trip
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('kind', ps.KINDS)
def test_defaults_and_values_set_back_move_no_bit(kind, f32):
    """30 steps of the kind's contact scenario (param_scenarios.Script; U from its scatter start) on three instances: untouched; the defaults written; drawn values written
    and the defaults written over them.  States and cache rows stay bit-identical, in fp64 and fp32."""
    n, steps = 2, 30
    dflt, other = ps.defaults(kind, n), ps.draws(kind, n, 0)
    pos, quat = ps.scatter_poses(kind, n)
    contacts = 0
    for e in range(n):
        trio = [_oracle(kind, f32, env_index=e) for _ in range(3)]
        fresh = trio[0].get_dynamics(), trio[0].get_wrench(), trio[0].get_actuation()
        assert np.all(fresh[1] == 0) and fresh[2]['gravity'].tolist() == [0.0, 0.0, np.float32(-9.8) if f32 else -9.8] and np.all(fresh[2]['motor_gain'] == 1) \
            and np.all(fresh[2]['motor_strength'] == 1)
        assert np.array_equal(fresh[0]['friction'].astype(np.float32), dflt['friction'][e]) and np.array_equal(fresh[0]['mass'].astype(np.float32), dflt['mass'][e])
        ps.apply_row(trio[2], other, e)
        got = trio[2].get_dynamics(), trio[2].get_wrench(), trio[2].get_actuation()
        assert np.array_equal(got[0]['friction'], other['friction'][e]) and np.array_equal(got[0]['mass'], other['mass'][e]) and np.array_equal(got[1], other['wrench'][e])
        assert all(np.array_equal(got[2][k], other[k][e]) for k in ('gravity', 'motor_gain', 'motor_strength'))
        for o in trio[1:]:          # the defaults are what a fresh instance reports, to the last bit of the build's precision
            o.set_dynamics(friction=fresh[0]['friction'], mass=fresh[0]['mass'])
            o.set_wrench(fresh[1])
            o.set_actuation(**fresh[2])
        for o in trio:
            o.reset()
            if kind == 'U':
                _block_to(o, pos[e], quat[e])
        script = ps.Script(kind, n, steps)
        for t in range(steps):
            blk = np.tile(_free(trio[0])[:3], (n, 1))
            a = script.action(t, blk)[e].astype(np.float64)
            for o in trio:
                o.step(a)
            contacts += trio[0].lib.rpo_cache_size(trio[0].h, None) > 0
            s0, r0 = trio[0].get_state(), trio[0].get_cache_row()
            for k, o in enumerate(trio[1:]):
                assert np.array_equal(o.get_state().view(np.int64), s0.view(np.int64)), (kind, f32, e, t, k)
                assert np.array_equal(o.get_cache_row().view(np.int32), r0.view(np.int32)), (kind, f32, e, t, k)
    assert contacts >= steps, contacts          # (a contact scenario: most steps end with cached manifolds)


def test_the_reference_builds_refuse():
    """librp_oracle_bullet.so keeps the baked model and its own constants: its setters say no"""
    from oracle import OracleEnv
    o = OracleEnv('U', bullet_ref=True)
    with pytest.raises(ValueError):
        o.set_actuation(gravity=[0.0, 0.0, -5.0])
    with pytest.raises(ValueError):
        o.set_wrench(None)


# ---------------------------------------------------------------- 2. free flight
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('kind', ['U', 'V'])
def test_free_flight_follows_the_recurrence(kind, f32):
    """the block in the air (tests/test_gpu_wrench.py's AIR), one step = twelve substeps of v <- v - dt kd (1 + |v|) v + dt (g + f / m), w likewise with t / (I_baked m / m_baked)
    about a principal axis of the unrotated block; that test's recurrence and bound"""
    from roboticsplayroompybullet_amd.vec_env import _model
    from test_gpu_wrench import AIR, _close, _recur
    mdl = _model(kind)
    I0, m0 = np.array(mdl['free'][0]['inertia']), mdl['free'][0]['mass']
    rng = np.random.default_rng(5)
    o = _oracle(kind, f32)
    o.reset()
    nb, na = len(o.get_wrench()), o.n_arm
    masses = o.get_dynamics()['mass']
    got_v, want_v, got_w, want_w = [], [], [], []
    for mass in (0.1, 0.15, 0.3, 0.8):
        for g in ((0.0, 0.0, -9.8), (3.0, 2.0, -5.0), (-4.0, 1.0, -12.0), (0.3, -0.2, 1.6)):
            m32, g32 = float(np.float32(mass)), np.array(g, np.float32).astype(np.float64)
            ms = masses.copy(); ms[0] = m32
            o.set_dynamics(mass=ms)
            o.set_actuation(gravity=g32)
            w = np.zeros((nb, 6))
            f = rng.uniform(-2.0, 2.0, 3).astype(np.float32).astype(np.float64)
            ax = int(rng.integers(3))
            tq = float(np.float32(rng.uniform(-2e-3, 2e-3)))
            w[na, 0:3] = f; w[na, 3 + ax] = tq
            o.set_wrench(w)
            v0 = rng.uniform(-0.5, 0.5, 3).astype(np.float32).astype(np.float64)
            w0 = np.zeros(3); w0[ax] = float(np.float32(rng.uniform(-1.0, 1.0)))
            _block_to(o, AIR, vel=v0, om=w0)
            o.run_simulation()
            s = _free(o)
            assert np.all(np.abs(s[:3] - np.array(AIR)) < 0.2)
            acc = np.zeros(3); acc[ax] = tq / (I0[ax] * m32 / m0)
            got_v.append(s[7:10]); want_v.append(_recur(v0, g32 + f / m32))
            got_w.append(s[10:13]); want_w.append(_recur(w0, acc))
    assert _close(np.array(got_v), np.array(want_v))
    assert _close(np.array(got_w), np.array(want_w))
    assert np.abs(np.array(want_w)).max() > 0.5 and np.abs(np.array(want_v)).max() > 0.5


def test_a_scene_joint_feels_force_and_gravity_along_its_axis():
    """the sliding door (a prismatic scene joint).  Its velocity motor holds it, so what a force or a gravity change does shows in the motor row's right-hand side
    (des - v*) / minv, not in the velocity after the solve: a force f on the door changes v* by dt (axis_world . f) / m, so the rhs by -dt (axis_world . f); a gravity
    change dg is the force m dg, to rounding"""
    from roboticsplayroompybullet_amd.vec_env import _model, wrench_names
    mdl = _model('U')
    k = next(i for i, j in enumerate(mdl['joint1']) if j['jtype'] == 1)
    j1 = mdl['joint1'][k]
    axis = np.array(j1['rot']).reshape(3, 3) @ np.array(j1['axis'])
    b = mdl['n_arm'] + len(mdl['free']) + k          # (the first prismatic scene joint: the sliding door)
    assert wrench_names('U')[b] == 'door'
    dg = np.array([1.5, -2.0, 1.0])
    rhs = []
    for case in range(3):
        o = _oracle('U')
        o.reset()
        if case == 1:
            o.set_actuation(gravity=np.array(ps.G0) + dg)
        if case == 2:
            w = np.zeros((len(wrench_names('U')), 6)); w[b, 0:3] = j1['mass'] * dg
            o.set_wrench(w)
        o.substep()
        rows = o.last_rows()
        r = rows[(rows[:, 0] == 1) & (rows[:, 1] == o.n_arm + 6 * o.n_free + k)]
        assert len(r) == 1 and abs(r[0, 6] - j1['mass']) < 1e-12 * j1['mass']
        rhs.append(r[0, 3])
    want = -DT * float(axis @ (j1['mass'] * dg))
    assert abs(want) > 1e-5
    assert abs(rhs[2] - rhs[0] - want) <= 1e-9 * abs(want), (rhs, want)
    assert abs(rhs[1] - rhs[2]) <= 1e-9 * abs(want), rhs


# ---------------------------------------------------------------- 3. the arm
@pytest.mark.parametrize('kind', ['U', 'V'])
def test_arm_accelerations_change_by_the_jacobian_transpose(kind):
    """rpo_forward_dynamics at four poses with moving joints.  A wrench (f through the centre of mass, t) on link i is the generalised force J_com_i^T f + J_w_i^T t: the
    accelerations change by M^-1 of it (the library's tau = tau0 - J_com^T f - J_w^T t is the bias torque, qdd = -M^-1 tau).  A gravity change dg is the force m_i dg on
    every link.  The device tests' bound: 1e-4 of max(1, |.|)"""
    from roboticsplayroompybullet_amd.vec_env import _model
    from test_gpu_wrench import _oracle_jacobians
    mdl = _model(kind)
    na = mdl['n_arm']
    rng = np.random.default_rng(11)
    o, fk = _oracle(kind), _oracle(kind)
    o.reset(); fk.reset()
    nb = len(o.get_wrench())
    worst = largest = 0.0
    for pose in range(4):
        s = o.get_state()
        lo, hi = o.arm_table()[:, 1], o.arm_table()[:, 2]
        q = np.array(o.rest_pose()) + rng.uniform(-0.3, 0.3, na)
        q = np.where(lo < hi, np.clip(q, lo + 1e-3, hi - 1e-3), q)
        s[:na], s[na:2 * na] = q, rng.uniform(-0.5, 0.5, na)
        o.set_state(s)
        o.set_wrench(None); o.set_actuation(gravity=ps.G0)
        qdd0 = o.forward_dynamics()
        Minv = o.mass_matrix_inv()
        Jc, Jw = _oracle_jacobians(fk, mdl, q)
        for i in range(na):
            w = np.zeros((nb, 6))
            w[i, 0:3], w[i, 3:6] = rng.uniform(-5.0, 5.0, 3), rng.uniform(-1.0, 1.0, 3)
            o.set_wrench(w)
            got = o.forward_dynamics() - qdd0
            want = Minv @ (Jc[i].T @ w[i, 0:3] + Jw[i].T @ w[i, 3:6])
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            assert np.all(err <= 1e-4), (kind, pose, i, got.tolist(), want.tolist())
            worst, largest = max(worst, err.max()), max(largest, np.abs(want).max())
        o.set_wrench(None)
        for dg in ((1.7, 0.0, 0.15), (0.0, -2.5, 0.4), (3.0, 2.0, 4.8), (-4.0, 1.0, -2.2)):
            o.set_actuation(gravity=np.array(ps.G0) + np.array(dg))
            got = o.forward_dynamics() - qdd0
            want = Minv @ sum(mdl['arm'][i]['mass'] * (Jc[i].T @ np.array(dg)) for i in range(na))
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            assert np.all(err <= 1e-4), (kind, pose, dg, got.tolist(), want.tolist())
            worst, largest = max(worst, err.max()), max(largest, np.abs(want).max())
    print('%s arm: largest |dqdd - want| / max(1, |want|) = %.3e, largest |want| %.1f' % (kind, worst, largest))
    assert largest > 1.0


# ---------------------------------------------------------------- 4. friction
def _parked(gid, target, f32=False):
    """an instance of an absolute_quat id after reset with its end effector driven to `target` (tests/test_gpu_dynamics.py's _park_arm), and the hold action"""
    o = _oracle(gid, f32)
    obs = o.reset()
    a = np.zeros(8)
    a[0:3], a[3:7] = target, obs['obs_quat'][3:7]
    for _ in range(30):
        obs = o.step(a)[0]
    assert np.linalg.norm(obs['obs_quat'][0:3] - np.array(target)) < 0.05
    return o, a


def _slide_run(block_mu, v0, steps=50):
    """tests/test_gpu_dynamics.py::test_friction_sets_the_slide_distance's scene on the oracle: (distance, end speed, the block's state, the pair frictions met)"""
    from roboticsplayroompybullet_amd.vec_env import dynamics_names
    o, hold = _parked('UR5Play1Obj-v0', (0.15, 0.0, 0.25))
    names = dynamics_names('U')['friction']
    fr = o.get_dynamics()['friction']
    assert fr[names.index('table')] == 0.5
    fr[names.index('block')] = block_mu
    o.set_dynamics(friction=fr)
    x0 = -0.05
    _block_to(o, (x0, 0.25, 0.0), vel=(-v0, 0.0, 0.0))
    mus = set()
    for _ in range(steps):
        o.step(hold)
        mus |= set(o.contact_mu().tolist())
    s = _free(o)
    return x0 - s[0], -s[7], s, mus


def test_friction_sets_the_slide_distance():
    """that test's scene, prediction (_slide) and tolerance (SLIDE_TOL), on the fp64 oracle"""
    from test_gpu_dynamics import K_LIN_DAMP, SLIDE_MU, SLIDE_TOL, SLIDE_V0, _slide
    runs = [_slide_run(mu, v0) for mu, v0 in zip(SLIDE_MU, SLIDE_V0)]
    dist, vend = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
    T = 50 * 12 / 300.0
    c = np.log(SLIDE_V0[0] / vend[0]) / (T * (1.0 + 0.5 * (SLIDE_V0[0] + vend[0])))
    assert abs(c - K_LIN_DAMP) < 1e-3 * K_LIN_DAMP, c
    assert np.all(np.abs(vend[1:]) < 1e-3), vend
    pred = np.array([_slide(v, m * 0.5 * 9.8, c) for v, m in zip(SLIDE_V0[1:], SLIDE_MU[1:])])
    rel = np.abs(dist[1:] - pred) / pred
    print('slide distances', dist.tolist(), 'predicted', pred.tolist(), 'relative error', rel.tolist())
    assert np.all(rel < SLIDE_TOL), rel
    for (d, v, s, mus), mu in zip(runs[1:], SLIDE_MU[1:]):
        assert float(np.float64(mu) * 0.5) in mus, (mu, mus)


def test_a_pair_friction_beyond_ten_slides_as_ten_does():
    """block frictions 24 and 80 against the table's 0.5 (products 12 and 40) behave as 20 does (product 10): the block thrown along the table at 2 m/s - friction that high
    trips it over its leading edge - has bit-identical states after four steps, and every contact of the pair carries the coefficient 10.  18 (product 9) ends elsewhere
    (3e-7 m, 4e-5 rad/s: with a block that tumbles the friction rows are at their bounds only for a few substeps), so the scene does tell coefficients apart"""
    ten, twelve, forty, nine = [_slide_run(mu, 2.0, steps=4) for mu in (20.0, 24.0, 80.0, 18.0)]
    for r in (twelve, forty):
        assert np.array_equal(r[2].view(np.int64), ten[2].view(np.int64))
        assert 10.0 in r[3] and max(r[3]) == 10.0, r[3]
    assert np.abs(nine[2] - ten[2]).max() > 1e-6 and 9.0 in nine[3] and 10.0 not in nine[3], (nine[2], ten[2], nine[3])


# ---------------------------------------------------------------- 5. mass
def test_mass_sets_the_momentum_exchange():
    """tests/test_gpu_dynamics.py::test_mass_sets_the_momentum_exchange's balance and tolerance on the fp64 oracle of the two-block scene (W)"""
    from roboticsplayroompybullet_amd.vec_env import dynamics_names
    from test_gpu_dynamics import K_LIN_DAMP, MASS_PAIRS, MOMENTUM_TOL
    names = dynamics_names('W')
    v0 = 0.3
    for mA, mB in MASS_PAIRS:
        o, hold = _parked('pandaPlay-v0', (-0.15, 0.0, 0.25))
        d = o.get_dynamics()
        for b in ('block', 'block2'):
            d['friction'][names['friction'].index(b)] = 0.0
        d['mass'][names['mass'].index('block')], d['mass'][names['mass'].index('block2')] = mA, mB
        o.set_dynamics(**d)
        _block_to(o, (0.0, 0.25, 0.0), vel=(v0, 0.0, 0.0), body=0)
        s = o.get_state()
        f1 = 2 * o.n_arm + 13
        s[f1:f1 + 13] = [0.12, 0.25, 0.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0]
        o.set_state(s)
        vs = [(v0, 0.0)]
        for _ in range(12):
            o.step(hold)
            vs.append((_free(o, 0)[7], _free(o, 1)[7]))
        vs = np.array(vs)
        m = np.array([mA, mB])
        damp = K_LIN_DAMP * (m * (1.0 + np.abs(vs)) * vs).sum(1)
        p_after = m @ vs[-1] + (0.5 * (damp[1:] + damp[:-1])).sum() * (12 / 300.0)
        assert _free(o, 1)[0] > 0.125
        rel = abs(p_after - mA * v0) / (mA * v0)
        print('masses', mA, mB, 'velocities after', vs[-1].tolist(), 'relative momentum error %.2e' % rel)
        assert rel < MOMENTUM_TOL, (mA, mB, rel)


def test_a_tipping_block_needs_the_inertia_to_scale_with_the_mass():
    """A frictionless block of mass m, tilted by 0.35 rad about y, falls from rest onto the table: its lower edge touches first and it tips.  Row by row: a normal row at lever r
    from the centre of mass has 1 / dinv = 1 / m + (r x n) . I^-1 (r x n) and rhs = -(n . v* + ...) dinv, where v* (gravity and damping) does not know the mass.  With
    I = I_baked m / m_baked both terms of 1 / dinv are 1 / s times the baked block's (s = m / m_baked), and so is every coupling between the rows, so every impulse is
    lambda = s lambda_baked, and the velocity changes dv = lambda n / m and dw = I^-1 (r x n) lambda are the baked block's own: the angular velocity the block gains per
    unit of normal impulse, w / sum(lambda), is m_baked / m times the baked block's.  Asserted on the first substep with contact rows, to 1e-9 in fp64: lambda's ratio,
    w's equality, and - the control - that a block whose inertia did NOT scale (the mass set, the torque's inverse inertia probed in free flight) would be told apart: the
    tipping rate changes by more than 10 % when only 1 / m changes in 1 / dinv."""
    from roboticsplayroompybullet_amd.vec_env import _model, dynamics_names
    names = dynamics_names('U')
    mdl = _model('U')
    m0 = mdl['free'][0]['mass']
    th = 0.35
    out = {}
    for mass in (m0, 0.25 * m0, 4.0 * m0):
        o, hold = _parked('UR5Play1Obj-v0', (0.15, 0.0, 0.25))
        d = o.get_dynamics()
        d['friction'][names['friction'].index('block')] = 0.0
        d['mass'][names['mass'].index('block')] = mass
        o.set_dynamics(**d)
        _block_to(o, (-0.1, 0.25, 0.03), quat=(0.0, np.sin(th / 2), 0.0, np.cos(th / 2)))
        na = o.n_arm
        for _ in range(60):
            o.substep()
            rows = o.last_rows()
            # the block's contact normals: no parent, upper bound 1e10, first dof among the block's six (the drawer rests on its rail all the time)
            con = rows[(rows[:, 0] == 0) & (rows[:, 2] < 0) & (rows[:, 5] > 1e9) & (rows[:, 1] >= na) & (rows[:, 1] < na + 6)]
            if len(con):
                break
        assert len(con) >= 1 and con[:, 7].sum() > 0, rows
        out[mass] = (con[:, 7].sum(), _free(o)[10:13].copy(), _free(o)[7:10].copy(), len(con), con[:, 6].copy())
    lam0, w0, v0, n0, dinv0 = out[m0]
    assert np.linalg.norm(w0) > 0.1, w0          # it tips
    for mass in (0.25 * m0, 4.0 * m0):
        lam, w, v, nc, dinv = out[mass]
        s = mass / m0
        assert nc == n0
        assert abs(lam / lam0 - s) <= 1e-9 * s, (lam, lam0, s)
        assert np.abs(w - w0).max() <= 1e-9 * np.linalg.norm(w0) and np.abs(v - v0).max() <= 1e-9 * np.linalg.norm(v0), (w, w0)
        assert np.abs(np.linalg.norm(w) / lam - (np.linalg.norm(w0) / lam0) / s) <= 1e-9 * np.linalg.norm(w0) / lam0 / s
        assert np.abs(dinv / dinv0 - s).max() <= 1e-9 * s          # the rows' effective masses scale as the mass: both the 1 / m and the inertia term did
        # the control: with the baked inertia 1 / dinv would be 1 / m + (1 / dinv0 - 1 / m0) - far from 1 / (s dinv0) because most of an edge row's 1 / dinv is the inertia term
        unscaled = 1.0 / (1.0 / mass + (1.0 / dinv0 - 1.0 / m0))
        assert np.abs(unscaled / (s * dinv0) - 1.0).min() > 0.1, unscaled / (s * dinv0)


# ---------------------------------------------------------------- 6. motors
def _motor_case(kind, joint, e_want, gain, strength, f32=False):
    """the arm at its rest pose, at rest, without gravity (so v* = 0), joint `joint` commanded e away, one substep: (e, the joint's motor row, 1 / Minv[j][j], qd after)"""
    o = _oracle(kind, f32)
    o.reset()
    na = o.n_arm
    s = o.get_state()
    s[:na], s[na:2 * na] = o.rest_pose(), 0.0
    o.set_state(s)
    o.set_actuation(gravity=[0.0, 0.0, 0.0], motor_gain=np.full(na, gain), motor_strength=np.full(na, strength))
    tgt = np.array(o.rest_pose()[:o.n_target])
    tgt[joint] += e_want
    o.goto_joint_poses(tgt)
    mode, mt, mx = o.get_motor()
    e = mt[joint] - o.get_state()[joint]
    assert mode[joint] == 1 and abs(e - e_want) < 1e-6 and abs(mx[joint] - 240 * DT) < 1e-6
    meff = 1.0 / o.mass_matrix_inv()[joint, joint]
    o.substep()
    rows = o.last_rows()
    r = rows[(rows[:, 0] == 1) & (rows[:, 1] == joint)]
    assert len(r) == 1
    return e, dict(zip(o.ROW_FIELDS, r[0])), meff, o.get_state()[na:2 * na], mx[joint], rows


@pytest.mark.parametrize('kind', ['U', 'P'])
def test_the_motor_row_follows_gain_and_strength(kind):
    """The row asks for the velocity (0.1 gain) e / dt: its first impulse (rhs, the row's unclamped step from lambda = 0, v* = 0) is M_eff (0.1 gain) e / dt with
    M_eff = 1 / Minv[j][j], and its bounds are -+ (240 dt) strength.  Below the clip the joint reaches the asked velocity (50 sweeps over rows that are otherwise satisfied);
    above it lambda is the bound exactly and the joint is slower.  Gains 0.5 / 1 / 2, either side of the clip; fp64"""
    j = 1
    for gain in (0.5, 1.0, 2.0):
        for strength, e_want, clipped in ((1.0, 2e-4, False), (0.4, 2e-4, False), (1.0, 0.08, True), (0.4, 0.08, True)):
            e, r, meff, qd, mx, rows = _motor_case(kind, j, e_want, gain, strength)
            des = KP * gain * e / DT
            assert abs(r['rhs'] - meff * des) <= 1e-9 * abs(meff * des), (gain, strength, r['rhs'], meff * des)
            assert abs(r['dinv'] - meff) <= 1e-9 * meff
            assert abs(r['hi'] - mx * strength) <= 1e-12 and r['lo'] == -r['hi']
            assert (meff * des > r['hi']) == clipped, (kind, gain, strength, meff * des, r['hi'])          # (the case is on the side of the clip it is meant for)
            if clipped:
                assert r['lambda'] == r['hi'] and 0 < qd[j] < des, (r, qd[j], des)
            else:
                assert abs(qd[j] - des) <= 1e-2 * des and abs(r['lambda']) < r['hi'], (qd[j], des, r)      # (50 Gauss-Seidel sweeps over the arm's coupled motor rows: 7e-4 off measured; the gains here are a factor 2 apart)


@pytest.mark.parametrize('kind', ['U', 'P'])
def test_strength_zero_switches_the_motors_off(kind):
    """strength 0: every arm motor row has the bounds [0, 0] and ends with lambda = 0; commanded 0.08 rad away, the arm's joints keep qd = 0 exactly (no gravity), where
    strength 1 moves them"""
    e, r, meff, qd, mx, rows = _motor_case(kind, 1, 0.08, 1.0, 0.0)
    motors = rows[(rows[:, 0] == 1) & (rows[:, 1] < N_MAIN[kind])]
    assert len(motors) == N_MAIN[kind] and np.all(motors[:, 4] == 0) and np.all(motors[:, 5] == 0) and np.all(motors[:, 7] == 0)
    assert np.all(qd[:N_MAIN[kind]] == 0.0), qd
    assert _motor_case(kind, 1, 0.08, 1.0, 1.0)[3][1] > 1e-2


# ---------------------------------------------------------------- 7. the control of the GPU scenarios
SENS = 1e-2          # ten times the lock-step's bound on a free body / an arm joint (1e-3)
# measured here (fp32 oracle, free-running; share of the comparable env-steps of the three scenarios together whose one-step result moves by more than SENS when the block is put
# back to its default), halved: see test_each_value_block_moves_the_scenarios' docstring
TWIN_SAME = {'U': 1.0000, 'P': 0.9952, 'V': 0.9891}          # the one-ulp CPU twin's share of env-steps with the same manifolds / points / GJK pairs, measured in the same run
SENS_FLOOR = {'friction': 0.14, 'mass': 0.12, 'wrench': 0.07, 'gravity': 0.076, 'motor': 0.41}


@functools.lru_cache(maxsize=None)
def free_run(kind):
    """the kind's scenario free-running on fp32 oracles with its parameter draws; per env-step: comparable (finite, the block above the floor), contacts, torsional rows,
    the one-step distance of each value block put back to its default, and the one-ulp twin's cache agreement"""
    from gpu_debug import oracle_state_from_record  # noqa: F401  (the record layout this scenario's GPU twin relies on)
    n, steps = ps.N_ENVS, ps.STEPS
    nm = N_MAIN[kind]
    tabs, fresh, dflt, mask = ps.draws(kind, n, 0), ps.draws(kind, n, 1), ps.defaults(kind, n), ps.redraw_mask(n)
    tabs = {k: v.copy() for k, v in tabs.items()}
    fz = ps.floor_z(kind)
    main = [_oracle(kind, True, env_index=e) for e in range(n)]
    side = [_oracle(kind, True, env_index=e) for e in range(n)]
    pos, quat = ps.scatter_poses(kind, n)
    for e, o in enumerate(main):
        ps.apply_row(o, tabs, e)
        o.reset()
        if kind == 'U':
            _block_to(o, pos[e], quat[e])
    script = ps.Script(kind, n, steps)
    na = main[0].n_arm
    out = dict(ok=np.zeros((steps, n), bool), ncon=np.zeros((steps, n), int), tors=np.zeros((steps, n), int), same=np.zeros((steps, n), bool),
               lifted=0, twin_arm=np.zeros((steps, n)), **{b: np.zeros((steps, n)) for b in ps.BLOCKS})
    pool = ThreadPoolExecutor(16)
    for t in range(steps):
        if t == ps.REDRAW_AT:
            for k in tabs:
                tabs[k][mask] = fresh[k][mask]
            for e in np.nonzero(mask)[0]:
                ps.apply_row(main[e], tabs, e)
        blk = np.array([_free(o)[:3] if o.n_free else np.zeros(3) for o in main])
        acts = script.action(t, blk)

        def one(e):
            o, x = main[e], side[e]
            pre_s, pre_r = o.get_state(), o.get_cache_row()
            a = acts[e].astype(np.float64)
            o.perform_action(a)
            tp = o.get_motor()[1][:o.n_target]
            o.run_simulation()
            so = o.get_state()
            d = {}

            def replay(block, nudge=False):
                s = pre_s.copy()
                if nudge:
                    s[:na] = np.nextafter(s[:na].astype(np.float32), np.float32(np.inf)).astype(np.float64)
                ps.apply_row(x, tabs, e, dflt, block)
                x.set_state(s)
                x.set_cache_row(pre_r)
                x.perform_action(a)
                x.goto_joint_poses(tp, gripper=float(a[-1]))
                x.run_simulation()
                return x.get_state()
            base = replay(None)
            assert np.array_equal(base, so), (kind, t, e)          # (a replay from state + cache row + targets is the step itself, bit for bit)
            for b in ps.BLOCKS:
                sx = replay(b)
                arm = (np.abs(sx[:na] - so[:na]) / np.maximum(1.0, np.abs(so[:na])))[:nm].max()
                free = np.abs(sx[2 * na:] [[i for k in range(o.n_free) for i in range(13 * k, 13 * k + 7)]] - so[2 * na:][[i for k in range(o.n_free) for i in range(13 * k, 13 * k + 7)]]).max()
                d[b] = max(arm, free)
            sw = replay(None, nudge=True)
            twin_arm = (np.abs(sw[:na] - so[:na]) / np.maximum(1.0, np.abs(so[:na])))[:nm].max()
            rw = x.get_cache_row()
            ro = o.get_cache_row()
            same = cache_rows.manifolds(rw) == cache_rows.manifolds(ro) and cache_rows.gjk_tags(rw) == cache_rows.gjk_tags(ro)
            ncon = len(o.contacts())          # (the contact list at the post-step state: what the next substep will meet)
            o.set_state(so); o.set_cache_row(ro)
            ok = bool(np.all(np.isfinite(so))) and all(_free(o, k)[2] >= fz for k in range(o.n_free - (1 if kind in 'UV' else 0)))
            return d, same, ncon, o.lib.rpo_last_num_tors(o.h), ok, twin_arm
        for e, (d, same, ncon, tors, ok, twin_arm) in enumerate(pool.map(one, range(n))):
            out['ok'][t, e], out['same'][t, e], out['ncon'][t, e], out['tors'][t, e], out['twin_arm'][t, e] = ok, same, ncon, tors, twin_arm
            for b in ps.BLOCKS:
                out[b][t, e] = d[b]
    pool.shutdown()
    if kind == 'P':
        out['lifted'] = int(sum(_free(o)[2] > 0.05 for o in main))
    return out


def test_each_value_block_moves_the_scenarios():
    """The three scenarios of tests/test_gpu_param_lockstep.py, free-running on the fp32 oracle with the same scripts, draws and seeds.  Every pre-state is stepped once more
    with one value block put back to its default; the share of comparable env-steps in which that moves a free body, a scene joint or an arm joint (relative to max(1, |q|))
    by more than 1e-2 - ten times what the lock-step tolerates - must reach SENS_FLOOR, half of what was measured when the scenarios were written.  Also here: at least 0.9
    of the env-steps stay comparable; the one-ulp twin's share of env-steps with the same manifolds / points / GJK pairs (the lock-step's yardstick); how many contacts
    a scenario reaches (the device's BIG class starts at 15).

    Measured (16 envs x 40 steps each, wrench scale 2; 1 867 comparable env-steps of 1 920): moved by more than 1e-2 in 0.2849 (friction), 0.2475 (mass), 0.1409 (wrench),
    0.1532 (gravity), 0.8243 (motor gain + strength) of them - SENS_FLOOR is half of each.  Per scenario: U comparable 0.948 (a block dropped onto an edge may roll out of
    the scene), 6.5 contacts per env-step, at most 18 (15 or more in 2 env-steps), torsional rows in 76 env-steps, the one-ulp twin keeps the same manifolds / points / GJK
    pairs in 1.0000 and its arm joints leave the oracle's by more than 1e-3 in 0.0016; P 0.969, 3.8, at most 9, torsional rows in 384, twin 0.9952 / 0.0065 (four env-steps of
    the lift, the block slipping between the pads), the block in the air at the end in 5 envs; V 1.000, 8.0, at most 20 (15 or more in 9), torsional rows in 118, twin
    0.9891 / 0.0031.  TWIN_SAME carries the twins' shares to the GPU test, and BIG is reached (V, U).  The twin's arm rate is asserted below the lock-step's own bound of 1 %:
    a scenario in which the reference's one-ulp twin misses that bound holds no device to it (V with sustained pressing: 5.0 %, param_scenarios.V_PRESS)."""
    runs = {k: free_run(k) for k in ps.KINDS}
    tot = sum(int(r['ok'].sum()) for r in runs.values())
    for k, r in runs.items():
        ok = r['ok']
        print('%s: comparable %.3f, contacts per env-step mean %.1f max %d (>= 15 in %d), torsional rows in %d env-steps, one-ulp twin same caches %.4f, its arm joints beyond 1e-3 in %.4f%s; moved > 1e-2 by: %s'
              % (k, ok.mean(), r['ncon'][ok].mean(), r['ncon'][ok].max(), int((r['ncon'][ok] >= 15).sum()), int((r['tors'][ok] > 0).sum()), r['same'][ok].mean(), (r['twin_arm'][ok] > 1e-3).mean(),
                 ', block in the air at the end in %d envs' % r['lifted'] if k == 'P' else '', {b: round(float((r[b][ok] > SENS).mean()), 4) for b in ps.BLOCKS}))
        assert ok.mean() >= 0.9, (k, ok.mean())
        assert r['same'][ok].mean() >= TWIN_SAME[k] - 0.005, (k, r['same'][ok].mean())          # (what the GPU test subtracts its 0.03 from still holds)
        assert (r['twin_arm'][ok] > 1e-3).mean() < 0.01, (k, (r['twin_arm'][ok] > 1e-3).mean())
    assert max(int(r['ncon'][r['ok']].max()) for r in runs.values()) >= 15          # BIG is reached, so the GPU test asserts it
    assert sum(int((r['tors'][r['ok']] > 0).sum()) for r in runs.values()) > 0
    assert runs['P']['lifted'] >= 1
    for b in ps.BLOCKS:
        share = sum(int((r[b][r['ok']] > SENS).sum()) for r in runs.values()) / tot
        print('%s: moved by more than %.0e in %.4f of %d env-steps (floor %.4f)' % (b, SENS, share, tot, SENS_FLOOR[b]))
        assert SENS_FLOOR[b] > 0 and share >= SENS_FLOOR[b], (b, share)
