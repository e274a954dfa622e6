"""Per-env external wrenches (rp_set_wrench / VecPlayEnv.set_wrench, push).  Run with -m gpu on the MI355X box.

Wrenches on bodies in contact - pushed arm links on the furniture, a pushed block between the pads, in all of k_solve2's paths - are held by
tests/test_gpu_param_lockstep.py: the CPU oracle takes the same wrenches per instance (rpo_set_wrench; its closed forms: tests/test_oracle_params.py) and follows the
device step by step with the device's own table rows.  This file holds the table and the properties of a body that is alone: the table's semantics; a zero table moves
no bit in any pipeline; a free body in the air follows the substep recurrence the kernel states, in fp64 on the host; an arm link's wrench changes the joint torques by
-(J_com^T f + J_w^T t), the Jacobian by central differences of the oracle's forward kinematics; signs on the scene; a wrench in env k reaches env k only;
set_wrench never waits for the device.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_autoreset import actions, end_masks
from test_gpu_reset_table import start_table

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE, PANDA, WIDE = 'UR5PlayAbsRPY1Obj-v0', 'pandaPlayAbsRPY1Obj-v0', 'pandaPlay-v0'
IDS = (HEADLINE, PANDA)
OBS = ('obs_quat', 'achieved_goal', 'desired_goal', 'controllable_achieved_goal', 'full_positional_state', 'joints', 'velocity', 'observation',
       'gripper_proprioception')
PIPES = ('groups1', 'groups3', 'fused1', 'fused2')
DT, KD, G = 1.0 / 300.0, 0.04, -9.8      # the library's substep, its linear / angular damping dv/dt = -KD (1 + |v|) v, gravity along z (rp_kernels.cuh)
SUBSTEPS = 12


def make(gid, n, seed, **kw):
    from roboticsplayroompybullet_amd import VecPlayEnv
    return VecPlayEnv(gid, n, seed=seed, **kw)


def model_of(env):
    from roboticsplayroompybullet_amd.vec_env import MODEL_OF
    kind = MODEL_OF[env.env_id]
    return kind, next(m for m in json.load(open(os.path.join(REPO, 'roboticsplayroompybullet_amd', 'assets', 'models.json')))['models'] if m['kind'] == kind)


def set_pipe(env, pipe):
    if pipe.startswith('fused'):
        env.set_fused(int(pipe[-1]))
    else:
        env.set_groups(int(pipe[-1]))


def snap(obs):
    return {k: obs[k].clone() for k in OBS if obs.get(k) is not None}


def random_wrench(env, seed, scale=1.0):
    """[N, n_body, 6]: arm links up to 3 N / 0.3 N m, the other bodies up to 0.3 N / 0.003 N m - pushes that disturb a scene without throwing it about"""
    names = env.wrench_names
    g = torch.Generator().manual_seed(seed)
    w = 2 * torch.rand((env.num_envs, len(names), 6), generator=g) - 1
    mag = torch.tensor([[3.0] * 3 + [0.3] * 3 if nm.startswith('link') else [0.3] * 3 + [0.003] * 3 for nm in names])
    return (w * mag * scale).to(env.device)


# ---------------------------------------------------------------- 1. the table
@pytest.mark.parametrize('gid', IDS + (WIDE,))
def test_table_semantics(gid):
    n = 6
    env = make(gid, n, 1, autoreset=True, max_episode_steps=0, end_on_fault=False)
    names = env.wrench_names
    na, nf, nj = C.c_int32(), C.c_int32(), C.c_int32()
    assert env.lib.rp_get_wrench_dims(env.h, C.byref(na), C.byref(nf), C.byref(nj)) == 0
    kind, mdl = model_of(env)
    assert (na.value, nf.value, nj.value) == (mdl['n_arm'], len(mdl['free']), len(mdl['joint1']))
    nb = len(names)
    assert nb == na.value + nf.value + nj.value
    w0 = env.get_wrench()
    assert w0.shape == (n, nb, 6) and w0.dtype == torch.float32 and not bool(w0.any())          # a fresh handle: zeros
    rnd = random_wrench(env, 2)
    env.set_wrench(rnd[0])                                                                          # rows = 1
    assert torch.equal(env.get_wrench(), rnd[0][None].expand(n, -1, -1))
    env.set_wrench(rnd)                                                                             # rows = N
    assert torch.equal(env.get_wrench(), rnd)
    m = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.uint8, device=env.device)
    other = random_wrench(env, 3)
    env.set_wrench(other, mask=m)                                                                   # rows = N under a mask
    want = torch.where(m.bool()[:, None, None], other, rnd)
    assert torch.equal(env.get_wrench(), want)
    env.set_wrench(other[2], mask=1 - m)                                                            # rows = 1 under a mask
    want = torch.where(m.bool()[:, None, None], want, other[2][None].expand(n, -1, -1))
    assert torch.equal(env.get_wrench(), want)
    env.set_wrench(None, mask=m)                                                                    # NULL = zero, masked
    want = torch.where(m.bool()[:, None, None], torch.zeros_like(want), want)
    assert torch.equal(env.get_wrench(), want)
    env.push(names[-1], force=[0.1, 0.2, 0.3], mask=m)                                              # one body's force; its torque and the rest stay
    want[m.bool(), nb - 1, 0:3] = torch.tensor([0.1, 0.2, 0.3], device=env.device)
    assert torch.equal(env.get_wrench(), want)
    tq = torch.arange(3 * n, dtype=torch.float32, device=env.device).reshape(n, 3) * 1e-3
    env.push(names[0], torque=tq)
    want[:, 0, 3:6] = tq
    assert torch.equal(env.get_wrench(), want)
    # refused arguments leave the table as it is
    lib, s = env.lib, env._stream()
    p = C.c_void_p(rnd.data_ptr())
    for rows in (0, 2, n - 1, n + 1, -1):
        assert lib.rp_set_wrench(env.h, p, rows, None, s) == -1, rows                               # RP_ERR_ARG
        assert lib.rp_set_wrench(env.h, None, rows, None, s) == -1, rows
    assert lib.rp_get_wrench(env.h, None, s) == -1
    assert lib.rp_get_wrench_dims(env.h, None, C.byref(nf), C.byref(nj)) == -1
    for bad in (rnd[:, :-1], rnd[:3], rnd[0, :, :5], rnd.reshape(n, -1)):
        with pytest.raises(ValueError):
            env.set_wrench(bad)
    with pytest.raises(ValueError):
        env.set_wrench(rnd, mask=torch.ones(n + 1, dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError):
        env.set_wrench(np.full((nb, 6), np.nan))
    with pytest.raises(ValueError):
        env.push(names[0])
    with pytest.raises(ValueError):
        env.push('no such body', force=[0, 0, 1])
    with pytest.raises(ValueError):
        env.push(names[0], force=[0.0, float('inf'), 0.0])
    assert torch.equal(env.get_wrench(), want)
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
    env.set_state(torch.zeros((n, 128), device=env.device) + env.get_state()[:, :128])
    assert torch.equal(env.get_wrench(), want)
    env.close()


# ---------------------------------------------------------------- 2. a zero table moves no bit
@pytest.mark.parametrize('pipe', PIPES)
@pytest.mark.parametrize('gid', IDS + (WIDE,))
def test_zero_table_changes_no_bit(gid, pipe):
    """A untouched; B had a wrench on every body, stepped with it, and had it zeroed again (NULL) before it was put back to A's state; Cn was given an
    explicit all-zero table (with a few -0.0).  Over reset and 16 steps with contacts in every env, B's and Cn's observations, rewards and state rows
    (record + contact cache) are A's, bit for bit."""
    n, seed, steps = 24, 7, 16
    A, B, Cn = (make(gid, n, seed) for _ in range(3))
    for E in (A, B, Cn):
        set_pipe(E, pipe)
    B.set_wrench(random_wrench(B, seed))
    B.reset()
    B.step(actions(B, 1, seed + 1)[0])
    B.set_wrench(None)
    z = torch.zeros_like(A.get_wrench())
    z[::2, :, ::2] = -0.0
    Cn.set_wrench(z)
    oa = snap(A.reset())
    B.reset()
    B.set_state(A.get_state())
    oc = Cn.reset()
    for k in oa:
        assert torch.equal(oa[k], oc[k]), k
    assert torch.equal(A.get_state(), Cn.get_state()) and torch.equal(A.get_state(), B.get_state())
    acts = actions(A, steps, seed)
    contacts = 0
    for t in range(steps):
        o, r, _, _ = A.step(acts[t])
        ra = (snap(o), r.clone())
        if pipe.startswith('groups'):          # (the split pipeline keeps the row counts of its latest substep)
            contacts += int((A.debug_row_counts()[:, 1] > 0).sum())
        for E in (B, Cn):
            o, r, _, _ = E.step(acts[t])
            for k in ra[0]:
                assert torch.equal(ra[0][k], o[k]), (t, k)
            assert torch.equal(ra[1], r), t
        if t % 5 == 0 or t == steps - 1:
            sa = A.get_state()
            assert torch.equal(sa, B.get_state()) and torch.equal(sa, Cn.get_state()), t
    assert contacts >= steps * n // 2 or not pipe.startswith('groups'), contacts          # (a rollout with contacts)
    for E in (A, B, Cn):
        E.close()


# ---------------------------------------------------------------- 3. free flight
AIR = (1.5, -1.0, 1.0)      # far from the arm's reach and from every fixture: no contact can form within a step


def _fly(env, v0, w0):
    """the block of every env to AIR, unrotated, with linear / angular velocity v0 / w0 ([3] or [n, 3]); one step; returns its (v, w) as float64 arrays"""
    lay = env.state_layout
    f0 = lay['free0'][0]
    rec = env.get_state()[:, :128].clone()
    rec[:, f0:f0 + 3] = torch.tensor(AIR, device=env.device)
    rec[:, f0 + 3:f0 + 7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=env.device)
    rec[:, f0 + 7:f0 + 10] = torch.as_tensor(v0, dtype=torch.float32, device=env.device)
    rec[:, f0 + 10:f0 + 13] = torch.as_tensor(w0, dtype=torch.float32, device=env.device)
    env.set_state(rec)
    env.step(actions(env, 1, 3)[0])
    s = env.get_state().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(s[:, f0:f0 + 3] - np.array(AIR)) < 0.2)
    return s[:, f0 + 7:f0 + 10], s[:, f0 + 10:f0 + 13]


def _recur(v, acc):
    """twelve substeps of v <- v - dt kd (1 + |v|) v + dt acc, in fp64"""
    v = np.array(v, dtype=np.float64)
    for _ in range(SUBSTEPS):
        v = v - DT * KD * (1.0 + np.linalg.norm(v, axis=-1, keepdims=True)) * v + DT * acc
    return v


def _close(got, want):
    """the issue's bound: what twelve fp32 updates of a handful of operations can lose, 1e-5 relative plus 1e-6 absolute"""
    err = np.abs(got - want)
    tol = 1e-5 * np.abs(want) + 1e-6
    print('max |error| %.3e  max error / bound %.3f' % (err.max(), (err / tol).max()))
    return bool(np.all(err <= tol))


@pytest.mark.parametrize('gid', IDS)
def test_free_flight_follows_the_recurrence(gid):
    n = 8
    env = make(gid, n, 2)
    env.reset()
    names = env.wrench_names
    b = names.index('block')
    ms = env.get_dynamics()['mass'].clone()
    mass = torch.tensor([0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.65, 0.8], device=env.device)
    ms[:, env.dynamics_names['mass'].index('block')] = mass
    env.set_dynamics(mass=ms)
    m64 = mass.cpu().numpy().astype(np.float64)[:, None]
    grav = np.array([0.0, 0.0, G])
    rng = np.random.default_rng(5)
    # a force per env, the block moving
    f = torch.tensor(rng.uniform(-2.0, 2.0, (n, 3)), dtype=torch.float32)
    v0 = torch.tensor(rng.uniform(-0.5, 0.5, (n, 3)), dtype=torch.float32)
    env.push('block', force=f)
    v, w = _fly(env, v0, 0.0)
    assert _close(v, _recur(v0.numpy(), grav + f.numpy().astype(np.float64) / m64))
    assert np.all(w == 0.0)
    # ... against the same flight without it: the force is what made the difference
    env.set_wrench(None)
    v_free, _ = _fly(env, v0, 0.0)
    assert _close(v_free, _recur(v0.numpy(), grav))
    assert np.all(np.abs(v - v_free).max(1) > 1e-4)
    # a torque about each principal axis of the unrotated block, the block spinning about that axis already; the force holds it against gravity
    kind, mdl = model_of(env)
    I0, m0 = np.array(mdl['free'][0]['inertia']), mdl['free'][0]['mass']
    hold = (mass * 9.8).cpu()          # f = -m g in fp32, as a caller computes it
    for ax in range(3):
        tq = np.zeros((n, 3)); tq[:, ax] = rng.uniform(-2e-3, 2e-3, n)
        w0 = np.zeros((n, 3)); w0[:, ax] = rng.uniform(-1.0, 1.0, n)
        tq32 = torch.tensor(tq, dtype=torch.float32)
        fz = torch.zeros((n, 3)); fz[:, 2] = hold
        env.push('block', force=fz, torque=tq32)
        v, w = _fly(env, 0.0, torch.tensor(w0, dtype=torch.float32))
        I = I0[ax] * m64 / m0
        acc = np.zeros((n, 3)); acc[:, ax] = tq32.numpy().astype(np.float64)[:, ax] / I[:, 0]
        assert _close(w, _recur(torch.tensor(w0, dtype=torch.float32).numpy(), acc)), ax
        assert _close(v, np.zeros((n, 3))), ax          # f = -m g holds the block at rest
    # the same in one env leaves the others falling
    env.set_wrench(None)
    env.push('block', force=fz, mask=torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.uint8))
    v, _ = _fly(env, 0.0, 0.0)
    assert abs(v[2, 2]) <= 1e-6 and np.all(np.delete(v[:, 2], 2) < -0.3)
    env.close()


# ---------------------------------------------------------------- 4. the arm
def _oracle_link_frames(o, mdl, q):
    """world (R [n_arm, 3, 3], COM [n_arm, 3]) of the arm's links at joint positions q, from the oracle's collider poses and the bake's collider frames"""
    o.set_arm_q(np.asarray(q, dtype=np.float64))
    Rc, pc, _ = o.colliders()
    Rs, coms = [], []
    for i, a in enumerate(mdl['arm']):
        c = next(k for k, col in enumerate(mdl['col']) if col['body'] == 1 + i)
        R = Rc[c] @ np.array(mdl['col'][c]['rot']).T
        p = pc[c] - R @ np.array(mdl['col'][c]['pos'])
        Rs.append(R); coms.append(p + R @ np.array(a['com']))
    return np.array(Rs), np.array(coms)


def _oracle_jacobians(o, mdl, q, h=1e-6):
    """(J_com [n_arm links, 3, n_arm dofs], J_w [.., 3, ..]) by central differences in fp64"""
    na = mdl['n_arm']
    Jc, Jw = np.zeros((na, 3, na)), np.zeros((na, 3, na))
    R0, _ = _oracle_link_frames(o, mdl, q)
    for j in range(na):
        e = np.zeros(na); e[j] = h
        Rp, cp = _oracle_link_frames(o, mdl, q + e)
        Rm, cm = _oracle_link_frames(o, mdl, q - e)
        Jc[:, :, j] = (cp - cm) / (2 * h)
        W = np.einsum('lab,lcb->lac', (Rp - Rm) / (2 * h), R0)          # dR R^T = [w]x
        Jw[:, :, j] = np.stack([W[:, 2, 1] - W[:, 1, 2], W[:, 0, 2] - W[:, 2, 0], W[:, 1, 0] - W[:, 0, 1]], 1) / 2
    return Jc, Jw


@pytest.mark.parametrize('gid', IDS)
def test_arm_torques_change_by_the_jacobian_transpose(gid):
    """four envs = four arm poses (after 0 .. 9 random steps the envs have drifted apart, joints moving); for each link a random wrench on that link in every
    env: tau (debug_substep) minus tau without it is -(J_com^T f + J_w^T t) within 1e-4 max(1, |.|) per joint, and exactly 0 for joints that do not carry
    the link"""
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
    tau0 = np.array([env.debug_substep(e)[512:512 + na].numpy() for e in range(n)], dtype=np.float64)
    assert np.abs(tau0).max() > 1.0
    anc = []
    for i in range(na):
        s, k = set(), i
        while k >= 0:
            s.add(k); k = mdl['arm'][k]['parent']
        anc.append(s)
    jac = [_oracle_jacobians(o, mdl, q[e]) for e in range(n)]
    rng = np.random.default_rng(11)
    worst = largest = 0.0
    for i in range(na):
        w = torch.zeros((n, len(names), 6))
        w[:, i, 0:3] = torch.tensor(rng.uniform(-5.0, 5.0, (n, 3)), dtype=torch.float32)
        w[:, i, 3:6] = torch.tensor(rng.uniform(-1.0, 1.0, (n, 3)), dtype=torch.float32)
        env.set_wrench(w.to(env.device))
        torch.cuda.synchronize()
        for e in range(n):
            tau = env.debug_substep(e)[512:512 + na].numpy().astype(np.float64)
            got = tau - tau0[e]
            Jc, Jw = jac[e]
            want = -(Jc[i].T @ w[e, i, 0:3].numpy().astype(np.float64) + Jw[i].T @ w[e, i, 3:6].numpy().astype(np.float64))
            for j in range(na):
                if j not in anc[i]:
                    assert got[j] == 0.0 and abs(want[j]) < 1e-6, (i, e, j, got[j], want[j])
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, err.max())
            assert np.all(err <= 1e-4), (names[i], e, got.tolist(), want.tolist())
            largest = max(largest, np.abs(want).max())
    print('arm: largest |dtau - want| / max(1, |want|) = %.3e, largest |want| %.2f' % (worst, largest))
    assert largest > 1.0
    env.close()


# ---------------------------------------------------------------- 5. signs on the scene
def _ee_link(env):
    kind, mdl = model_of(env)
    return env.wrench_names[mdl['sites'][0]['body'] - 1]


def _park(env, steps=30):
    """the end effector to a fixed spot high above the table's corner; returns the hold action"""
    a = actions(env, 1, 3)[0].clone()
    a[:, 0:3] = torch.tensor([0.15, 0.0, 0.25], device=env.device)
    a[:, 3:6] = 0.0
    env.reset()
    for _ in range(steps):
        env.step(a)
    return a


@pytest.mark.parametrize('gid', IDS)
def test_a_force_along_its_axis_moves_the_drawer_both_ways(gid):
    """the drawer slides along y (its y is the observation's drawer entry).  Envs: 0 untouched, 1 pushed along +y, 2 along -y, 60 steps: each pushed drawer ends
    on its force's side of the twin, and at least one of them (the open side; the closed side has a stop) by more than 2 cm.  Then the opened drawer's
    force is reversed and a copy of it is left alone: the reversed one ends on the closing side of the copy by more than 1 cm."""
    env = make(gid, 3, 4)
    hold = _park(env)
    lay = env.state_layout
    kind, mdl = model_of(env)
    d = next(k for k, fb in enumerate(mdl['free']) if fb['rot_locked'])
    assert env.wrench_names[mdl['n_arm'] + d] == 'drawer'
    fy = lay['free0'][0] + 13 * d + 1
    st = env.get_state()
    env.set_state(st[0:1].expand(3, -1).contiguous())          # three copies of env 0
    F = 1.0                                                   # N on a 0.1 kg drawer: ten times its weight
    env.push('drawer', force=torch.tensor([[0.0, 0.0, 0.0], [0.0, F, 0.0], [0.0, -F, 0.0]]))
    for _ in range(60):
        env.step(hold)
    y = env.get_state()[:, fy].cpu().numpy().astype(np.float64)
    print('drawer y: untouched %.4f, pushed +y %.4f, pushed -y %.4f' % tuple(y))
    assert y[1] >= y[0] and y[2] <= y[0]
    assert max(y[1] - y[0], y[0] - y[2]) > 0.02
    k = 1 if y[1] - y[0] > y[0] - y[2] else 2
    sgn = 1.0 if k == 1 else -1.0
    st = env.get_state()
    env.set_state(st[k:k + 1].expand(3, -1).contiguous())
    env.push('drawer', force=torch.tensor([[0.0, 0.0, 0.0], [0.0, -sgn * F, 0.0], [0.0, 0.0, 0.0]]))
    for _ in range(30):
        env.step(hold)
    y2 = env.get_state()[:, fy].cpu().numpy().astype(np.float64)
    print('opened drawer: left alone %.4f, force reversed %.4f' % (y2[0], y2[1]))
    assert sgn * (y2[0] - y2[1]) > 0.01
    assert y2[2] == y2[0]
    env.close()


@pytest.mark.parametrize('gid', IDS)
def test_an_upward_force_lifts_the_position_controlled_arm(gid):
    env = make(gid, 2, 4)
    a = actions(env, 1, 6)[0].clone()
    a[1] = a[0]
    env.reset()
    st = env.get_state()
    env.set_state(st[0:1].expand(2, -1).contiguous())
    env.push(_ee_link(env), force=[0.0, 0.0, 30.0], mask=torch.tensor([0, 1], dtype=torch.uint8))
    for _ in range(50):
        o, _, _, _ = env.step(a)
    z = o['obs_quat'][:, 2].cpu().numpy().astype(np.float64)
    print('end effector z: twin %.6f, pushed up %.6f' % (z[0], z[1]))
    assert z[1] > z[0]
    env.close()


@pytest.mark.parametrize('gid', IDS)
def test_a_sideways_force_slides_the_block_only_above_friction(gid):
    """the block rests on the table top: mu = friction(block) friction(table) (at most 10), from get_dynamics.  1.3 mu m g sideways makes it slide (net 0.3 mu g
    for 0.2 s: about 4 cm), 0.7 mu m g does not (less than 1 mm)"""
    env = make(gid, 3, 4)
    hold = _park(env)
    dn, dyn = env.dynamics_names, env.get_dynamics()
    mu = min(float(dyn['friction'][0, dn['friction'].index('block')] * dyn['friction'][0, dn['friction'].index('table')]), 10.0)
    m = float(dyn['mass'][0, dn['mass'].index('block')])
    lay = env.state_layout
    f0 = lay['free0'][0]
    st = env.get_state()
    env.set_state(st[0:1].expand(3, -1).contiguous())
    x0 = float(st[0, f0])
    assert abs(x0) < 0.3 and float(st[0, f0 + 7:f0 + 13].abs().max()) < 1e-2          # on the table, at rest
    s = -1.0 if x0 > 0 else 1.0          # toward the table's middle
    w = mu * m * 9.8
    env.push('block', force=torch.tensor([[0.0, 0.0, 0.0], [s * 1.3 * w, 0.0, 0.0], [s * 0.7 * w, 0.0, 0.0]]))
    for _ in range(5):
        env.step(hold)
    x = env.get_state()[:, f0].cpu().numpy().astype(np.float64)
    print('mu %.3f m %.3f: block x untouched %.5f, 1.3 mu m g %.5f, 0.7 mu m g %.5f' % (mu, m, x[0], x[1], x[2]))
    assert s * (x[1] - x[0]) > 0.01
    assert abs(x[2] - x[0]) < 1e-3
    env.close()


# ---------------------------------------------------------------- 6. isolation
def _isolated(A, Cn, k, steps, seed, table):
    """A (a wrench in env k) against Cn (none) through reset(mask), autoreset steps in which env k ends twice (settled, then from a reset table): every
    env but k is Cn's bit for bit; env k is not"""
    n = A.num_envs
    keep = torch.ones(n, dtype=torch.bool, device=A.device)
    keep[k] = False
    differs = False

    def check(what, xa, xc):
        assert torch.equal(xa[keep], xc[keep]), what
        return not torch.equal(xa[k], xc[k])

    oa, oc = snap(A.reset()), snap(Cn.reset())
    for key in oa:
        differs |= check(('reset', key), oa[key], oc[key])
    m = (torch.arange(n, device=A.device) % 2 == k % 2).to(torch.uint8)
    oa, oc = snap(A.reset(mask=m)), snap(Cn.reset(mask=m))
    for key in oa:
        differs |= check(('reset(mask)', key), oa[key], oc[key])
    acts = actions(A, 2 * steps, seed)
    masks = end_masks(n, 2 * steps, seed + 1, A.device, 0.15)
    for t in range(2 * steps):
        if t == steps:
            A.set_reset_table(table); Cn.set_reset_table(table)
        masks[t][k] = 1 if t % steps == 2 else 0
        res = []
        for E in (A, Cn):
            o, r, d, _ = E.step(acts[t], end_mask=masks[t])
            res.append(dict(snap(o), reward=r.clone(), done=d.clone()))
        for key in res[0]:
            differs |= check((t, key), res[0][key], res[1][key])
    differs |= check('state', A.get_state(), Cn.get_state())
    assert differs


@pytest.mark.parametrize('pipe', PIPES + ('shard',))
@pytest.mark.parametrize('gid', IDS + (WIDE,))
def test_a_wrench_reaches_its_env_and_no_other(gid, pipe):
    n, seed, k = 40, 11, 17
    kw = dict(autoreset=True, max_episode_steps=0, end_on_fault=False)      # (ends from end_mask only: the same envs end in both)
    if pipe == 'shard':
        kw['env_offset'] = 64
    A, Cn = make(gid, n, seed, **kw), make(gid, n, seed, **kw)
    if pipe != 'shard':
        set_pipe(A, pipe); set_pipe(Cn, pipe)
    m = torch.zeros(n, dtype=torch.uint8, device=A.device)
    m[k] = 1
    w = random_wrench(A, seed)
    A.set_wrench(w, mask=m)
    table = start_table(Cn, 16, seed + 9)
    _isolated(A, Cn, k, 5, seed, table)
    want = torch.zeros_like(w)
    want[k] = w[k]
    assert torch.equal(A.get_wrench(), want)          # no reset changed it
    A.close(); Cn.close()


# ---------------------------------------------------------------- 7. asynchrony
@pytest.mark.parametrize('gid', IDS)
def test_set_wrench_never_waits_for_the_device(gid):
    """behind a ~1 s sleep kernel, set_wrench with device tensors and a device mask, set_wrench(None, mask) and push with device tensors all return while the
    stream is busy; what they set acts in the next step"""
    n, seed = 16, 6
    A = make(gid, n, seed)
    A.reset()
    w = random_wrench(A, seed)
    m = (torch.arange(n, device=A.device) % 2 == 0).to(torch.uint8)
    f = torch.rand((n, 3), device=A.device)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(A.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); torch.cuda._sleep(10 ** 7); t1.record()
    torch.cuda.synchronize()
    cycles = int(min(10 ** 7 * 1000.0 / max(t0.elapsed_time(t1), 1e-3), 5e9))
    torch.cuda._sleep(cycles)
    A.set_wrench(w, mask=m)
    A.set_wrench(None, mask=1 - m)
    A.push('block', force=f, mask=m)
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy
    want = torch.where(m.bool()[:, None, None], w, torch.zeros_like(w))
    b = A.wrench_names.index('block')
    want[m.bool(), b, 0:3] = f[m.bool()]
    assert torch.equal(A.get_wrench(), want)
    B = make(gid, n, seed)
    B.reset()
    a = actions(A, 1, seed)[0]
    oa, ob = A.step(a)[0], B.step(a)[0]
    sa, sb = A.get_state(), B.get_state()
    assert torch.equal(sa[1::2], sb[1::2]) and all(not torch.equal(sa[e], sb[e]) for e in range(0, n, 2))
    A.close(); B.close()
