"""Per-env gravity and arm-motor gain / strength (rp_set_actuation / VecPlayEnv.set_actuation).  Run with -m gpu on the MI355X box.

Gravity, gain and strength where they meet contacts - a held block under a tilted gravity, motor strength against a table, the motor rows that k_solve2 rebuilds in
solve4_body, heavy_solve and super_solve - are held by tests/test_gpu_param_lockstep.py: the CPU oracle has gravity, gain and strength per instance (rpo_set_gravity,
rpo_set_motor; their closed forms: tests/test_oracle_params.py) and follows the device step by step with the device's own table rows.  This file holds the table and the
properties that need no oracle step: the table's semantics; the default row moves no bit in any
pipeline; a free body in the air follows the substep recurrence under the env's own gravity, and agrees with the same change expressed as a wrench; the
arm's bias torques change by -sum_i m_i J_com_i^T dg (the oracle's Jacobians); the drawer and the prismatic scene joints feel the component along their
axis; strength 0 switches a motor off and a strength below / above the gravity torque lets a joint sag / hold; the gain follows e (1 - 0.1 gain)^12 as
closely as the fp64 oracle follows it at gain 1; a change in env k reaches env k only; set_actuation never waits for the device.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_gpu_autoreset import actions
from test_gpu_reset_table import start_table
from test_gpu_wrench import (HEADLINE, IDS, PANDA, PIPES, WIDE, _close, _fly, _isolated, _oracle_jacobians, _park, _recur, make, model_of, set_pipe, snap)

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK = 'pandaPick-v0'
ABS_JOINTS = {HEADLINE: 'UR5PlayAbsJoints1Obj-v0', PANDA: 'pandaPlayAbsJoints1Obj-v0'}
DT, KP, SUBSTEPS = 1.0 / 300.0, 0.1, 12      # the library's substep, its position-motor gain, substeps per step (rp_kernels.cuh)
G0 = (0.0, 0.0, -9.8)


def defaults(env):
    n, na = env.num_envs, len(env.actuation_names['motor'])
    return {'gravity': torch.tensor(G0, device=env.device).expand(n, 3), 'motor_gain': torch.ones((n, na), device=env.device),
            'motor_strength': torch.ones((n, na), device=env.device)}


def random_actuation(env, seed):
    """a row per env: gravity tilted and scaled, gains in [0.5, 1.5], strengths in [0.3, 1.2]"""
    n, na = env.num_envs, len(env.actuation_names['motor'])
    g = torch.Generator().manual_seed(seed)
    grav = torch.tensor(G0) + torch.tensor([3.0, 3.0, 2.0]) * (2 * torch.rand((n, 3), generator=g) - 1)
    return {'gravity': grav.to(env.device), 'motor_gain': (0.5 + torch.rand((n, na), generator=g)).to(env.device),
            'motor_strength': (0.3 + 0.9 * torch.rand((n, na), generator=g)).to(env.device)}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ('gravity', 'motor_gain', 'motor_strength'))


# ---------------------------------------------------------------- 1. the table
@pytest.mark.parametrize('gid', IDS + (PICK, WIDE))
def test_table_semantics(gid):
    n = 6
    env = make(gid, n, 1, autoreset=True, max_episode_steps=0, end_on_fault=False)
    kind, mdl = model_of(env)
    na = C.c_int32()
    assert env.lib.rp_get_actuation_dims(env.h, C.byref(na)) == 0 and na.value == mdl['n_arm']
    names = env.actuation_names
    assert list(names['gravity']) == ['x', 'y', 'z'] and tuple(names['motor']) == tuple(env.wrench_names[:na.value])
    a0 = env.get_actuation()
    assert a0['gravity'].shape == (n, 3) and a0['motor_gain'].shape == (n, na.value) and a0['motor_strength'].shape == (n, na.value)
    assert all(v.dtype == torch.float32 for v in a0.values())
    assert same(a0, defaults(env))                                                                  # a fresh handle: (0, 0, -9.8), ones, ones
    rnd = random_actuation(env, 2)
    env.set_actuation(gravity=rnd['gravity'][0])                                                    # rows = 1, the other parts NULL: left alone
    want = dict(defaults(env), gravity=rnd['gravity'][0][None].expand(n, -1))
    assert same(env.get_actuation(), want)
    env.set_actuation(motor_gain=rnd['motor_gain'])                                                 # rows = N
    want['motor_gain'] = rnd['motor_gain']
    assert same(env.get_actuation(), want)
    env.set_actuation(motor_strength=rnd['motor_strength'][3])
    want['motor_strength'] = rnd['motor_strength'][3][None].expand(n, -1)
    assert same(env.get_actuation(), want)
    env.set_actuation(**rnd)                                                                        # all three, rows = N
    assert same(env.get_actuation(), rnd)
    m = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.uint8, device=env.device)
    other = random_actuation(env, 3)
    env.set_actuation(gravity=other['gravity'], motor_strength=other['motor_strength'], mask=m)     # rows = N under a mask, the gain NULL
    want = {k: (torch.where(m.bool()[:, None], other[k], rnd[k]) if k != 'motor_gain' else rnd[k]) for k in rnd}
    assert same(env.get_actuation(), want)
    env.set_actuation(gravity=other['gravity'][2], motor_gain=other['motor_gain'], mask=1 - m)      # one row and N rows in one call, under a mask
    want['gravity'] = torch.where(m.bool()[:, None], want['gravity'], other['gravity'][2][None].expand(n, -1))
    want['motor_gain'] = torch.where(m.bool()[:, None], want['motor_gain'], other['motor_gain'])
    assert same(env.get_actuation(), want)
    env.set_actuation(gravity=[1.0, -2.0, -9.0], motor_gain=np.full(na.value, 0.5), mask=[0, 1, 0, 0, 0, 0])      # host values
    want['gravity'] = want['gravity'].clone(); want['motor_gain'] = want['motor_gain'].clone()
    want['gravity'][1] = torch.tensor([1.0, -2.0, -9.0], device=env.device)
    want['motor_gain'][1] = 0.5
    assert same(env.get_actuation(), want)
    # refused arguments leave the table as it is
    lib, s = env.lib, env._stream()
    gp, kp = C.c_void_p(rnd['gravity'].data_ptr()), C.c_void_p(rnd['motor_gain'].data_ptr())
    for rows in (0, 2, n - 1, n + 1, -1):
        assert lib.rp_set_actuation(env.h, gp, kp, kp, rows, None, s) == -1, rows                   # RP_ERR_ARG
    assert lib.rp_set_actuation(env.h, None, None, None, 1, None, s) == -1
    assert lib.rp_set_actuation(env.h, None, None, None, n, None, s) == -1
    assert lib.rp_get_actuation(env.h, None, None, None, s) == -1
    assert lib.rp_get_actuation_dims(env.h, None) == -1
    with pytest.raises(ValueError):
        env.set_actuation()
    for bad in (dict(gravity=rnd['gravity'][:, :2]), dict(gravity=rnd['gravity'][:3]), dict(motor_gain=rnd['motor_gain'][:, :-1]),
                dict(motor_strength=rnd['motor_strength'][:n - 1]), dict(motor_gain=rnd['gravity'][0]),
                dict(gravity=rnd['gravity'], mask=torch.ones(n + 1, dtype=torch.uint8, device=env.device))):
        with pytest.raises(ValueError):
            env.set_actuation(**bad)
    for bad in (dict(gravity=[0.0, 0.0, -50.5]), dict(gravity=[51.0, 0.0, 0.0]), dict(gravity=[0.0, float('nan'), 0.0]), dict(motor_gain=[-0.1] * na.value),
                dict(motor_gain=[10.5] * na.value), dict(motor_strength=[-1e-3] * na.value), dict(motor_strength=np.full((n, na.value), 10.5)),
                dict(motor_strength=[float('inf')] * na.value)):
        with pytest.raises(ValueError):
            env.set_actuation(**bad)                                                                # host values out of range
    assert same(env.get_actuation(), want)
    # parameters, not state: reset, reset(mask), reset(o) (rp_reset_to), steps, an autoreset end (settled, then from a table) and rp_set_state keep them
    env.reset()
    env.reset(mask=m)
    table = start_table(env, n, 5)
    env.reset(o=table)
    acts = actions(env, 3, 4)
    ones = torch.ones(n, dtype=torch.uint8, device=env.device)
    env.step(acts[0])
    _, _, done, _ = env.step(acts[1], end_mask=ones)
    assert bool(done.all())
    env.set_reset_table(table)
    _, _, done, _ = env.step(acts[2], end_mask=ones)
    assert bool(done.all())
    env.set_state(env.get_state().clone())
    assert same(env.get_actuation(), want)
    env.close()


# ---------------------------------------------------------------- 2. the default row moves no bit
@pytest.mark.parametrize('pipe', PIPES)
@pytest.mark.parametrize('gid', IDS + (WIDE,))
def test_defaults_change_no_bit(gid, pipe):
    """A untouched; B had the defaults written explicitly; Cn ran a reset and a step under other values, had the defaults written back and was put to A's
    state.  Over reset and 20 steps of random actions B's and Cn's observations, rewards and full state rows are A's, bit for bit."""
    n, seed, steps = 8, 7, 20
    A, B, Cn = (make(gid, n, seed) for _ in range(3))
    for E in (A, B, Cn):
        set_pipe(E, pipe)
    na = len(A.actuation_names['motor'])
    B.set_actuation(gravity=list(G0), motor_gain=[1.0] * na, motor_strength=[1.0] * na)
    Cn.set_actuation(**random_actuation(Cn, seed))
    Cn.reset()
    Cn.step(actions(Cn, 1, seed + 1)[0])
    Cn.set_actuation(**defaults(Cn))
    oa = snap(A.reset())
    ob = B.reset()
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    Cn.reset()
    Cn.set_state(A.get_state())
    assert torch.equal(A.get_state(), B.get_state()) and torch.equal(A.get_state(), Cn.get_state())
    acts = actions(A, steps, seed)
    for t in range(steps):
        o, r, _, _ = A.step(acts[t])
        ra = (snap(o), r.clone())
        for E in (B, Cn):
            o, r, _, _ = E.step(acts[t])
            for k in ra[0]:
                assert torch.equal(ra[0][k], o[k]), (t, k)
            assert torch.equal(ra[1], r), t
        sa = A.get_state()
        assert torch.equal(sa, B.get_state()) and torch.equal(sa, Cn.get_state()), t
    assert same(B.get_actuation(), defaults(B)) and same(Cn.get_actuation(), defaults(Cn))
    for E in (A, B, Cn):
        E.close()


# ---------------------------------------------------------------- 3. free flight
GRAVITIES = ((0.0, 0.0, -9.8), (0.0, 0.0, 0.0), (0.0, 0.0, 9.8), (1.7, 0.0, -9.65), (0.0, -2.5, -9.4), (3.0, 2.0, -5.0), (-4.0, 1.0, -12.0), (0.3, -0.2, 1.6))


@pytest.mark.parametrize('gid', IDS)
def test_free_flight_under_the_envs_gravity(gid):
    """eight envs, eight gravity vectors (default, zero, +z, tilted, scaled): the flying block's velocity after a step is the fp64 recurrence with acc = g_env
    within 1e-5 |v| + 1e-6; and an env at default gravity whose block is pushed with m (g' - g) agrees with the env under g' within twice that bound (two
    independent fp32 evaluation orders)"""
    n = 8
    env = make(gid, n, 2)
    env.reset()
    grav = torch.tensor(GRAVITIES, dtype=torch.float32)
    g64 = grav.numpy().astype(np.float64)
    rng = np.random.default_rng(5)
    v0 = torch.tensor(rng.uniform(-0.5, 0.5, (n, 3)), dtype=torch.float32)
    env.set_actuation(gravity=grav)
    v, w = _fly(env, v0, 0.0)
    assert _close(v, _recur(v0.numpy(), g64))
    assert np.all(w == 0.0)
    v_rest, _ = _fly(env, 0.0, 0.0)
    assert _close(v_rest, _recur(np.zeros((n, 3)), g64))
    assert np.all(v_rest[1] == 0.0)                                     # zero gravity, at rest: nothing moves
    assert v_rest[2, 2] > 0.3 and v_rest[0, 2] < -0.3                     # +z lifts, the default drops
    # the same change as a wrench at default gravity
    mass = float(env.get_dynamics()['mass'][0, env.dynamics_names['mass'].index('block')])
    env.set_actuation(gravity=list(G0))
    env.push('block', force=(grav - torch.tensor(G0)) * mass)
    v_w, _ = _fly(env, v0, 0.0)
    err = np.abs(v - v_w)
    tol = 2 * (1e-5 * np.abs(v) + 1e-6)
    print('gravity against wrench: max |difference| %.3e  max difference / bound %.3f' % (err.max(), (err / tol).max()))
    assert np.all(err <= tol)
    env.close()


# ---------------------------------------------------------------- 4. the arm
@pytest.mark.parametrize('gid', IDS)
def test_arm_torques_change_by_the_links_weights(gid):
    """four envs = four arm poses (drifted apart over 9 random steps), a gravity change dg per env: tau (debug_substep) minus tau at default gravity is
    -sum_i m_i J_com_i^T dg within 1e-4 max(1, |.|) per joint, the Jacobians by central differences of the oracle's forward kinematics, the masses the
    bake's; and the wrenches m_i dg on every link at default gravity give the same tau within that bound"""
    from oracle import OracleEnv
    n = 4
    env = make(gid, n, 9)
    env.reset()
    acts = actions(env, 9, 2)
    for t in range(9):
        env.step(acts[t])
    kind, mdl = model_of(env)
    na = mdl['n_arm']
    names = env.wrench_names
    o = OracleEnv(kind)
    o.reset()
    q = env.get_state()[:, :na].cpu().numpy().astype(np.float64)
    assert np.abs(q[0] - q[1]).max() > 1e-2          # (different poses)
    torch.cuda.synchronize()

    def taus():
        torch.cuda.synchronize()
        return np.array([env.debug_substep(e)[512:512 + na].numpy() for e in range(n)], dtype=np.float64)

    tau0 = taus()
    assert np.abs(tau0).max() > 1.0
    masses = np.array([a['mass'] for a in mdl['arm']], dtype=np.float64)
    dg = torch.tensor([[2.0, 0.0, 0.0], [0.0, -3.0, 1.0], [1.5, 2.5, -4.0], [-1.0, 0.5, 9.8]], dtype=torch.float32)
    env.set_actuation(gravity=torch.tensor(G0) + dg)
    dg_dev = (env.get_actuation()['gravity'].cpu() - torch.tensor(G0)).numpy().astype(np.float64)      # (what fp32 kept of g0 + dg)
    got_g = taus() - tau0
    env.set_actuation(gravity=list(G0))
    w = torch.zeros((n, len(names), 6))
    w[:, :na, 0:3] = torch.tensor(masses, dtype=torch.float32)[None, :, None] * torch.tensor(dg_dev, dtype=torch.float32)[:, None, :]
    env.set_wrench(w.to(env.device))
    got_w = taus() - tau0
    worst = worst_w = largest = 0.0
    for e in range(n):
        Jc, _ = _oracle_jacobians(o, mdl, q[e])
        want = -sum(masses[i] * (Jc[i].T @ dg_dev[e]) for i in range(na))
        err = np.abs(got_g[e] - want) / np.maximum(1.0, np.abs(want))
        err_w = np.abs(got_g[e] - got_w[e]) / np.maximum(1.0, np.abs(want))
        worst, worst_w, largest = max(worst, err.max()), max(worst_w, err_w.max()), max(largest, np.abs(want).max())
        assert np.all(err <= 1e-4), (e, got_g[e].tolist(), want.tolist())
        assert np.all(err_w <= 1e-4), (e, got_g[e].tolist(), got_w[e].tolist())
    print('arm: worst |dtau - want| / max(1, |want|) = %.3e (bound 1e-4), against the wrenches %.3e, largest |want| %.2f' % (worst, worst_w, largest))
    assert largest > 1.0
    env.close()


# ---------------------------------------------------------------- 5. the drawer and the prismatic scene joints
@pytest.mark.parametrize('gid', IDS)
def test_a_tilt_along_its_axis_moves_the_drawer_both_ways(gid):
    """the drawer slides along y.  Envs: 0 at default gravity, 1 tilted along +y, 2 along -y (10 m/s^2: what the wrench test's 1 N is to the 0.1 kg drawer), 60
    steps with the arm parked: each tilted drawer ends on its tilt's side of the twin, at least one of them (the open side; the closed side has a stop) by
    more than 2 cm, and the twin stays where it was (1 mm)"""
    env = make(gid, 3, 4)
    hold = _park(env)
    lay = env.state_layout
    kind, mdl = model_of(env)
    d = next(k for k, fb in enumerate(mdl['free']) if fb['rot_locked'])
    fy = lay['free0'][0] + 13 * d + 1
    st = env.get_state()
    env.set_state(st[0:1].expand(3, -1).contiguous())          # three copies of env 0
    y_before = float(st[0, fy])
    T = 10.0
    env.set_actuation(gravity=torch.tensor([[0.0, 0.0, -9.8], [0.0, T, -9.8], [0.0, -T, -9.8]]))
    for _ in range(60):
        env.step(hold)
    y = env.get_state()[:, fy].cpu().numpy().astype(np.float64)
    print('drawer y: before %.4f, default gravity %.4f, tilted +y %.4f, tilted -y %.4f' % ((y_before,) + tuple(y)))
    assert y[1] >= y[0] and y[2] <= y[0]
    assert max(y[1] - y[0], y[0] - y[2]) > 0.02
    assert abs(y[0] - y_before) < 1e-3
    env.close()


@pytest.mark.parametrize('gid', IDS)
def test_a_prismatic_scene_joint_feels_the_component_along_its_axis(gid):
    """v* (debug_substep) of every prismatic scene joint: the unit changes of gravity along x, y, z give dt a_x, dt a_y, dt a_z with a the joint's world axis
    (a unit vector, 1e-3), a general change dg gives dt (a . dg) within 1e-6, and a revolute scene joint's v* does not move at all"""
    env = make(gid, 5, 4)
    env.reset()
    kind, mdl = model_of(env)
    na, nf = mdl['n_arm'], len(mdl['free'])
    dofs = [na + 6 * nf + k for k in range(len(mdl['joint1']))]
    dg = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [2.0, -3.0, 4.5]])
    st = env.get_state()
    env.set_state(st[0:1].expand(5, -1).contiguous())
    env.set_actuation(gravity=torch.tensor(dg + np.array(G0), dtype=torch.float32))
    torch.cuda.synchronize()
    vs = np.array([env.debug_substep(e)[480:512].numpy() for e in range(5)], dtype=np.float64)
    seen = 0
    for k, d in enumerate(dofs):
        dv = vs[1:, d] - vs[0, d]
        if mdl['joint1'][k]['jtype'] != 1:
            assert np.all(dv == 0.0), (k, dv)
            continue
        a = dv[:3] / DT
        print('scene joint %d: world axis from v* %s, general change %.6e against %.6e' % (k, a.round(5).tolist(), dv[3], DT * (a @ dg[4])))
        assert abs(np.linalg.norm(a) - 1.0) < 1e-3, a
        assert abs(dv[3] - DT * (a @ dg[4])) < 1e-6
        seen += 1
    assert seen >= 1
    env.close()


# ---------------------------------------------------------------- 6. strength 0
def _inside_limits(env, mdl):
    """the record with the arm at rest and every joint strictly inside its limits (a tenth of the range from either end; the prismatic finger joints at the
    middle of theirs, equal, so that the Panda's gear row has nothing to correct)"""
    na = mdl['n_arm']
    lay = env.state_layout
    rec = env.get_state()[:, :128].clone()
    lo = torch.tensor([a['lower'] for a in mdl['arm']], dtype=torch.float32, device=env.device)
    hi = torch.tensor([a['upper'] for a in mdl['arm']], dtype=torch.float32, device=env.device)
    pris = torch.tensor([a['jtype'] == 1 for a in mdl['arm']], device=env.device)
    q0 = lay['q'][0]
    q = torch.minimum(torch.maximum(rec[:, q0:q0 + na], lo + 0.1 * (hi - lo)), hi - 0.1 * (hi - lo))
    q = torch.where(pris[None, :], (0.5 * (lo + hi))[None, :].expand_as(q), q)
    rec[:, q0:q0 + na] = q
    rec[:, lay['qd'][0]:lay['qd'][0] + na] = 0.0
    return rec


@pytest.mark.parametrize('gid', IDS)
def test_strength_zero_switches_the_motors_off(gid):
    """no gravity, every strength 0, the arm at rest inside its limits: five steps of random actions leave the arm's joints where they were (1e-6; 0 expected);
    the twin env with default strengths moves a main joint by more than 1e-2 under the same actions"""
    env = make(gid, 2, 4)
    env.reset()
    kind, mdl = model_of(env)
    na = mdl['n_arm']
    rec = _inside_limits(env, mdl)
    rec[1] = rec[0]
    env.set_state(rec)
    env.set_actuation(gravity=[0.0, 0.0, 0.0])
    env.set_actuation(motor_strength=[0.0] * na, mask=[1, 0])
    q0 = env.get_state()[:, :na].cpu().numpy().astype(np.float64)
    acts = actions(env, 5, 6)
    acts[:, 1] = acts[:, 0]
    for t in range(5):
        env.step(acts[t])
    q = env.get_state()[:, :na].cpu().numpy().astype(np.float64)
    moved = np.abs(q - q0)
    print('strength 0: largest joint change %.3e (expected 0); default strength: largest main-joint change %.3e' % (moved[0].max(), moved[1, :6].max()))
    assert moved[0].max() <= 1e-6
    assert moved[1, :6].max() > 1e-2
    env.close()


# ---------------------------------------------------------------- 7. the strength threshold against gravity
@pytest.mark.parametrize('gid', IDS)
def test_a_joint_sags_below_the_gravity_torque_and_holds_above_it(gid):
    """an absolute-joints id of the same arm, 'hold here' for STEPS steps.  Joint j = the main joint with the largest gravity torque |tau_g[j]| (> 1 N m, from
    debug_substep at rest).  Env 0: strength_j such that strength_j * max impulse_j / dt = 0.5 |tau_g[j]| - the joint sags the way gravity pulls it; env 1: the
    factor 2.0 - it holds.  The sagging joint moves at least ten times as far."""
    STEPS = 10
    env = make(ABS_JOINTS[gid], 2, 4)
    env.reset()
    kind, mdl = model_of(env)
    na = mdl['n_arm']
    lay = env.state_layout
    rec = env.get_state()[:, :128].clone()
    rec[:, lay['qd'][0]:lay['qd'][0] + na] = 0.0
    rec[1] = rec[0]
    env.set_state(rec)
    torch.cuda.synchronize()
    tau_g = env.debug_substep(0)[512:512 + na].numpy().astype(np.float64)
    nd = env.action_high.numel() - 1
    j = int(np.argmax(np.abs(tau_g[:nd])))
    assert abs(tau_g[j]) > 1.0, tau_g
    a = torch.zeros((2, nd + 1), device=env.device)
    a[:, :nd] = rec[:, lay['q'][0]:lay['q'][0] + nd]
    env.step(a)                                       # (one step files the motor bounds into the record)
    mx = float(env.get_state()[0, lay['motor_maximp'][0] + j])
    env.set_state(rec)
    st = torch.ones((2, na))
    st[0, j] = 0.5 * abs(tau_g[j]) * DT / mx
    st[1, j] = 2.0 * abs(tau_g[j]) * DT / mx
    assert float(st.max()) <= 10.0
    env.set_actuation(motor_strength=st)
    for _ in range(STEPS):
        env.step(a)
    dq = (env.get_state()[:, lay['q'][0] + j] - rec[:, lay['q'][0] + j]).cpu().numpy().astype(np.float64)
    print('joint %d, tau_g %.3f N m, max impulse %.4f N m s, strengths %.4f / %.4f: moved %.6e (factor 0.5) and %.6e (factor 2.0) in %d steps' %
          (j, tau_g[j], mx, float(st[0, j]), float(st[1, j]), dq[0], dq[1], STEPS))
    assert dq[0] * -tau_g[j] > 0.0                    # (qdd = -M^-1 tau: the way gravity pulls)
    assert abs(dq[0]) > 1e-3
    assert abs(dq[0]) >= 10.0 * abs(dq[1])
    env.close()


# ---------------------------------------------------------------- 8. the gain
@pytest.mark.parametrize('gid', IDS)
def test_the_remaining_error_follows_the_gain(gid):
    """no gravity, the arm at rest, joint 0 of an absolute-joints id commanded e = 1e-3 rad away, gains 0.5, 1 and 2 in three envs: the error left after one
    step is e (1 - 0.1 gain)^12 within three times what the fp64 oracle - same state, same action, its own gain 1 - is away from that law (the solver's
    finite-iteration deviation; the factor: fp32 and a second evaluation order, as tests/tolerances.py argues), and a higher gain leaves a smaller error."""
    from oracle import OracleEnv
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    from gpu_debug import oracle_state_from_record
    E, J = 1e-3, 0
    gains = (0.5, 1.0, 2.0)
    env = make(ABS_JOINTS[gid], 3, 4)
    env.reset()
    kind, mdl = model_of(env)
    na = mdl['n_arm']
    lay = env.state_layout
    rec = env.get_state()[:, :128].clone()
    rec[:, lay['qd'][0]:lay['qd'][0] + na] = 0.0
    rec[1] = rec[0]; rec[2] = rec[0]
    env.set_state(rec)
    nd = env.action_high.numel() - 1
    a = torch.zeros((3, nd + 1), device=env.device)
    a[:, :nd] = rec[:, lay['q'][0]:lay['q'][0] + nd]
    a[:, J] += E
    target = a[0, J].double().item()
    e0 = target - rec[0, lay['q'][0] + J].double().item()      # (what fp32 kept of e)
    # the oracle at gain 1
    o = OracleEnv(ABS_JOINTS[gid], seed=4, env_index=0)
    o.reset()
    o.set_state(oracle_state_from_record(o, rec[0].cpu().numpy()))
    o.step(a[0].cpu().numpy().astype(np.float64))
    dev = abs((target - o.get_state()[J]) - e0 * (1.0 - KP) ** SUBSTEPS)
    bound = 3.0 * dev
    g = torch.ones((3, na))
    g[:, J] = torch.tensor(gains)
    env.set_actuation(gravity=[0.0, 0.0, 0.0], motor_gain=g)
    env.step(a)
    left = target - env.get_state()[:, lay['q'][0] + J].double().cpu().numpy()
    law = np.array([e0 * (1.0 - KP * k) ** SUBSTEPS for k in gains])
    print('oracle deviation from the law at gain 1: %.3e, bound %.3e; error left %s, law %s, |difference| %s' %
          (dev, bound, left.tolist(), law.tolist(), np.abs(left - law).tolist()))
    assert np.all(np.abs(left - law) <= bound)
    assert left[0] > left[1] > left[2]
    env.close()


# ---------------------------------------------------------------- 9. isolation
@pytest.mark.parametrize('pipe', PIPES + ('shard',))
@pytest.mark.parametrize('gid', IDS + (WIDE,))
def test_a_change_reaches_its_env_and_no_other(gid, pipe):
    """eight envs, env k's row changed (gravity, gains, strengths): through reset, reset(mask), steps, and autoreset ends settled and from a reset table every
    other env is bit for bit the run in which nothing was changed, and env k is not"""
    n, seed, k = 8, 11, 5
    kw = dict(autoreset=True, max_episode_steps=0, end_on_fault=False)      # (ends from end_mask only: the same envs end in both)
    if pipe == 'shard':
        kw['env_offset'] = 64
    A, Cn = make(gid, n, seed, **kw), make(gid, n, seed, **kw)
    if pipe != 'shard':
        set_pipe(A, pipe); set_pipe(Cn, pipe)
    m = torch.zeros(n, dtype=torch.uint8, device=A.device)
    m[k] = 1
    rnd = random_actuation(A, seed)
    A.set_actuation(mask=m, **rnd)
    table = start_table(Cn, 16, seed + 9)
    _isolated(A, Cn, k, 5, seed, table)
    want = {key: torch.where(m.bool()[:, None], rnd[key], v) for key, v in defaults(A).items()}
    assert same(A.get_actuation(), want)          # no reset changed it
    A.close(); Cn.close()


# ---------------------------------------------------------------- 10. asynchrony
@pytest.mark.parametrize('gid', IDS)
def test_set_actuation_never_waits_for_the_device(gid):
    """behind a ~1 s sleep kernel, set_actuation with device tensors and a device mask returns while the stream is busy; what it set acts in the next step"""
    n, seed = 8, 6
    A = make(gid, n, seed)
    A.reset()
    rnd = random_actuation(A, seed)
    m = (torch.arange(n, device=A.device) % 2 == 0).to(torch.uint8)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(A.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); torch.cuda._sleep(10 ** 7); t1.record()
    torch.cuda.synchronize()
    cycles = int(min(10 ** 7 * 1000.0 / max(t0.elapsed_time(t1), 1e-3), 5e9))
    torch.cuda._sleep(cycles)
    A.set_actuation(mask=m, **rnd)
    A.set_actuation(gravity=rnd['gravity'][1], mask=1 - m)
    A.set_actuation(gravity=defaults(A)['gravity'], mask=1 - m)
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy
    want = {key: torch.where(m.bool()[:, None], rnd[key], v) for key, v in defaults(A).items()}
    assert same(A.get_actuation(), want)
    B = make(gid, n, seed)
    B.reset()
    a = actions(A, 1, seed)[0]
    A.step(a); B.step(a)
    sa, sb = A.get_state(), B.get_state()
    assert torch.equal(sa[1::2], sb[1::2]) and all(not torch.equal(sa[e], sb[e]) for e in range(0, n, 2))
    A.close(); B.close()
