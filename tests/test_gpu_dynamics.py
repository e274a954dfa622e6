"""Per-env lateral friction and free-body mass (rp_set_dynamics / VecPlayEnv.set_dynamics).  Run with -m gpu on the MI355X box.

What holds the values themselves in contact - the pair friction of arm-link and cached-point contacts, the heavy path's friction bounds, the torsional bound, the
clamp at 10, the inertia scale of a body that turns in contact - is tests/test_gpu_param_lockstep.py: the CPU oracle has the same parameters per instance
(rpo_set_friction, rpo_set_mass; their closed forms: tests/test_oracle_params.py) and follows the device step by step with the device's own table rows.  This file
holds the table and the properties that need no oracle: baked values written back change no bit; an env's values reach that env and no other, in every pipeline and
through every reset path; a block slides the distance its friction gives; a collision keeps the momentum its masses give.
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
IDS = ('UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'UR5Reach-v0', 'pandaPlay-v0')
ALL_KINDS = {'U': 'UR5PlayAbsRPY1Obj-v0', 'R': 'UR5Reach-v0', 'P': 'pandaPick-v0', 'Q': 'pandaReach-v0', 'V': 'pandaPlayAbsRPY1Obj-v0', 'W': 'pandaPlay-v0'}
OBS = ('obs_quat', 'achieved_goal', 'desired_goal', 'controllable_achieved_goal', 'full_positional_state', 'joints', 'velocity', 'observation',
       'gripper_proprioception')


def make(gid, n, seed, **kw):
    from roboticsplayroompybullet_amd import VecPlayEnv
    return VecPlayEnv(gid, n, seed=seed, **kw)


def random_dynamics(env, seed):
    """every env's baked values times U[0.25, 4], as [N, k] device tensors"""
    g = torch.Generator().manual_seed(seed)
    d = env.get_dynamics()
    return {k: (v.cpu() * (0.25 + 3.75 * torch.rand(v.shape, generator=g))).to(env.device) for k, v in d.items()}


def snap(env, obs):
    return {k: obs[k].clone() for k in OBS if obs.get(k) is not None}


def test_defaults_are_the_bake():
    """a fresh handle's table: per collision object the fp32 of the oracle's friction of its colliders, per free body the oracle's mass"""
    from oracle import OracleEnv
    models = {m['kind']: m for m in json.load(open(os.path.join(REPO, 'roboticsplayroompybullet_amd', 'assets', 'models.json')))['models']}
    for kind, gid in ALL_KINDS.items():
        env = make(gid, 3, 0)
        d = env.get_dynamics()
        torch.cuda.synchronize()
        mdl, cols = models[kind], OracleEnv(kind).collider_list()
        names = env.dynamics_names
        assert d['friction'].shape == (3, len(names['friction'])) and d['mass'].shape == (3, len(names['mass'])), kind
        fr = np.zeros(len(names['friction']), dtype=np.float32)
        for c, col in enumerate(cols):
            fr[mdl['col'][c]['obj']] = np.float32(col['friction'])
        ms = np.array([next(c['mass'] for c in cols if c['body'] == mdl['n_arm'] + 1 + f) for f in range(len(mdl['free']))], dtype=np.float32)
        assert np.array_equal(d['friction'].cpu().numpy(), np.tile(fr, (3, 1))), kind
        assert np.array_equal(d['mass'].cpu().numpy(), np.tile(ms, (3, 1)).reshape(3, -1)), kind
        env.close()


@pytest.mark.parametrize('rows', ('one', 'all'))
@pytest.mark.parametrize('gid', IDS)
def test_baked_values_written_back_change_nothing(gid, rows):
    """the bake written back (rows = 1 and rows = N): reset, 50 autoreset steps with ends, reset(mask) - every observation, state record and contact-cache
    row equals an untouched twin's, bit for bit"""
    n, seed = 48, 3
    A = make(gid, n, seed, autoreset=True, max_episode_steps=0)
    B = make(gid, n, seed, autoreset=True, max_episode_steps=0)
    d = B.get_dynamics()
    if rows == 'one':
        B.set_dynamics(friction=d['friction'][0].clone(), mass=d['mass'][0].clone())
    else:
        B.set_dynamics(friction=d['friction'].clone(), mass=d['mass'].clone())
    oa, ob = A.reset(), B.reset()
    for k in OBS:
        assert torch.equal(oa[k], ob[k]), k
    acts = actions(A, 50, seed)
    masks = end_masks(n, 50, seed, A.device, 0.05)
    for t in range(50):
        oa, ra, da, _ = A.step(acts[t], end_mask=masks[t])
        sa = (snap(A, oa), ra.clone(), da.clone())
        ob, rb, db, _ = B.step(acts[t], end_mask=masks[t])
        for k in sa[0]:
            assert torch.equal(sa[0][k], ob[k]), (t, k)
        assert torch.equal(sa[1], rb) and torch.equal(sa[2], db), t
    assert torch.equal(A.get_state(), B.get_state())
    m = (torch.arange(n, device=A.device) % 3 == 0).to(torch.uint8)
    oa = snap(A, A.reset(mask=m))
    ob = B.reset(mask=m)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(A.get_state(), B.get_state())
    A.close(); B.close()


def _run_three(A, B, Cn, S, steps, seed, table):
    """A, B, Cn through reset(mask), autoreset steps (settled resets, then from a reset table): B's rows in S equal A's, the others Cn's"""
    n = A.num_envs

    def check(what, xa, xb, xc):
        assert torch.equal(xb[S], xa[S]), what
        assert torch.equal(xb[~S], xc[~S]), what

    def check_obs(t, oa, ob, oc):
        for k in oa:
            check((t, k), oa[k], ob[k], oc[k])

    outs = [snap(E, E.reset()) for E in (A, B, Cn)]
    check_obs('reset', *outs)
    m = (torch.arange(n, device=A.device) % 2 == 1).to(torch.uint8)
    outs = [snap(E, E.reset(mask=m)) for E in (A, B, Cn)]
    check_obs('reset(mask)', *outs)
    acts = actions(A, 2 * steps, seed)
    masks = end_masks(n, 2 * steps, seed + 1, A.device, 0.15)
    for t in range(2 * steps):
        if t == steps:
            for E in (A, B, Cn):
                E.set_reset_table(table)
        outs = []
        for E in (A, B, Cn):
            o, r, d, _ = E.step(acts[t], end_mask=masks[t])
            outs.append(dict(snap(E, o), reward=r.clone(), done=d.clone()))
        check_obs(t, *outs)
    check('state', A.get_state(), B.get_state(), Cn.get_state())


@pytest.mark.parametrize('pipe', ('split', 'fused1', 'fused2', 'groups1', 'groups3'))
@pytest.mark.parametrize('gid', IDS)
def test_values_reach_their_env_and_no_other(gid, pipe):
    """A: random values in every env; B: the same values in a random third S of the envs, the rest baked; Cn: untouched.  Through reset(mask), settled
    autoreset and autoreset from a table: B's rows in S equal A's bit for bit, the other rows Cn's.  Catches a block, slot or list index read in place
    of the env."""
    n, seed = 40, 11
    kw = dict(autoreset=True, max_episode_steps=0, end_on_fault=False)      # (ends from end_mask only: the same envs end in all three)
    A, B, Cn = (make(gid, n, seed, **kw) for _ in range(3))
    for E in (A, B, Cn):
        if pipe.startswith('fused'):
            E.set_fused(int(pipe[-1]))
        elif pipe.startswith('groups'):
            E.set_groups(int(pipe[-1]))
    rnd = random_dynamics(A, seed)
    g = torch.Generator().manual_seed(seed + 5)
    S = (torch.rand(n, generator=g) < 1 / 3).to(A.device)
    S[0] = True; S[1] = False
    A.set_dynamics(**rnd)
    B.set_dynamics(friction=rnd['friction'], mass=rnd['mass'], mask=S)
    table = start_table(Cn, 16, seed + 9)
    _run_three(A, B, Cn, S, 6, seed, table)
    d = A.get_dynamics()
    assert torch.equal(d['friction'], rnd['friction']) and torch.equal(d['mass'], rnd['mass'])      # no reset changed them
    for E in (A, B, Cn):
        E.close()


@pytest.mark.parametrize('gid', IDS)
def test_shards_take_their_slices(gid):
    """one handle of 2n envs with random values equals two env_offset shards of n given the matching halves of the table"""
    n, seed = 24, 5
    kw = dict(autoreset=True, max_episode_steps=0, end_on_fault=False)
    full = make(gid, 2 * n, seed, **kw)
    a = make(gid, n, seed, env_offset=0, **kw)
    b = make(gid, n, seed, env_offset=n, **kw)
    rnd = random_dynamics(full, seed)
    full.set_dynamics(**rnd)
    a.set_dynamics(friction=rnd['friction'][:n].contiguous(), mass=rnd['mass'][:n].contiguous())
    b.set_dynamics(friction=rnd['friction'][n:].contiguous(), mass=rnd['mass'][n:].contiguous())
    of = snap(full, full.reset())
    oa, ob = a.reset(), b.reset()
    for k in of:
        assert torch.equal(of[k], torch.cat([oa[k], ob[k]])), k
    acts = actions(full, 8, seed)
    masks = end_masks(2 * n, 8, seed, full.device, 0.15)
    for t in range(8):
        of, rf, df, _ = full.step(acts[t], end_mask=masks[t])
        of = dict(snap(full, of), r=rf.clone(), d=df.clone())
        oa, ra, da, _ = a.step(acts[t, :n], end_mask=masks[t][:n])
        oa = dict(snap(a, oa), r=ra.clone(), d=da.clone())
        ob, rb, db, _ = b.step(acts[t, n:], end_mask=masks[t][n:])
        for k in of:
            assert torch.equal(of[k], torch.cat([oa[k], {**ob, 'r': rb, 'd': db}[k]])), (t, k)
    assert torch.equal(full.get_state(), torch.cat([a.get_state(), b.get_state()]))
    for E in (full, a, b):
        E.close()


def _park_arm(env, target, steps=30):
    """drive the end effector to `target` (absolute_quat ids: position, the orientation it has after reset, gripper 0) and return the hold action"""
    o = env.reset()
    a = torch.zeros((env.num_envs, 8), device=env.device)
    a[:, 0:3] = torch.tensor(target, device=env.device)
    a[:, 3:7] = o['obs_quat'][:, 3:7]
    for _ in range(steps):
        o, _, _, _ = env.step(a)
    ee = o['obs_quat'][:, 0:3].cpu()
    assert float((ee - torch.tensor(target)).norm(dim=1).max()) < 0.05, ee      # (the arm is where the test wants it: off the blocks' path)
    return a


def _place(rec, lay, body, pos, vel):
    f0 = lay['free%d' % body][0]
    rec[:, f0:f0 + 3] = pos
    rec[:, f0 + 3:f0 + 7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=rec.device)
    rec[:, f0 + 7:f0 + 10] = vel
    rec[:, f0 + 10:f0 + 13] = 0.0


# v0 [m/s], block friction per env; the table's friction is 0.5
SLIDE_MU = (0.0, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
SLIDE_V0 = (0.05, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
# relative error of the slide distance against the prediction with the damping the mu = 0 env measured: first MI355X run 0.017 % at most; 2e-3 keeps a
# tenfold margin, where one baked friction for every block (1.7 cm) misses by 45 % or more
SLIDE_TOL = 2e-3
K_LIN_DAMP = 0.04      # the library's linear damping: dv/dt = -K (1 + |v|) v (rp_kernels.cuh), measured here by the mu = 0 env


def _slide(v0, decel, c, dt=1.0 / 300.0):
    """distance to rest under dv/dt = -decel - c (1 + v) v, integrated per substep as the library does (semi-implicit), the last partial step closed form"""
    v, x = v0, 0.0
    while True:
        a = decel + c * (1.0 + v) * v
        if v - a * dt <= 0.0:
            return x + v * v / (2.0 * a)
        v -= a * dt
        x += v * dt


def test_friction_sets_the_slide_distance():
    """UR5 play scene, one block per env on the table top, arm parked high and to the side.  The block starts at v0 along -x with friction mu_b against the
    table's 0.5: it slides v0^2 / (2 mu_b 0.5 g), a little less for the linear damping, which the mu_b = 0 env measures (its speed decays by the damping
    alone).  With one baked friction every block would stop at the same 1.7 cm."""
    gid = 'UR5Play1Obj-v0'
    n = len(SLIDE_MU)
    env = make(gid, n, 2)
    hold = _park_arm(env, (0.15, 0.0, 0.25))
    names = env.dynamics_names
    d = env.get_dynamics()
    fr = d['friction'].clone()
    fr[:, names['friction'].index('block')] = torch.tensor(SLIDE_MU, device=env.device)
    table_mu = float(d['friction'][0, names['friction'].index('table')])
    assert table_mu == 0.5
    env.set_dynamics(friction=fr)
    rec = env.get_state()[:, :128].clone()
    lay = env.state_layout
    x0 = -0.05
    v0 = torch.tensor(SLIDE_V0, device=env.device)
    _place(rec, lay, 0, torch.tensor([-0.2, 0.25, 0.0], device=env.device), 0.0)
    rec[:, lay['free0'][0]] = x0
    rec[:, lay['free0'][0] + 7] = -v0          # toward -x, away from the parked arm
    env.set_state(rec)
    traj = []
    for _ in range(50):
        env.step(hold)
        traj.append(env.get_state()[:, lay['free0'][0]:lay['free0'][0] + 10].clone())
    traj = torch.stack(traj).cpu().numpy()          # [steps, n, 10]
    dist = x0 - traj[-1, :, 0]
    vend = -traj[-1, :, 7]
    g = 9.8
    print('slide distances', dist.tolist(), 'end speeds', vend.tolist())
    T = 50 * 12 / 300.0
    c = np.log(SLIDE_V0[0] / vend[0]) / (T * (1.0 + 0.5 * (SLIDE_V0[0] + vend[0])))      # mu = 0: the damping alone (first run: 0.040002)
    assert abs(c - K_LIN_DAMP) < 1e-3 * K_LIN_DAMP, c
    assert abs(dist[0] - SLIDE_V0[0] * T * (1 + vend[0] / SLIDE_V0[0]) / 2) < 0.01 * dist[0], dist[0]
    assert np.all(np.abs(vend[1:]) < 1e-3), vend
    pred = np.array([_slide(v, m * table_mu * g, c) for v, m in zip(SLIDE_V0[1:], SLIDE_MU[1:])])
    rel = np.abs(dist[1:] - pred) / pred
    assert np.all(rel < SLIDE_TOL), ('measured', dist[1:].tolist(), 'predicted', pred.tolist(), 'relative error', rel.tolist())
    env.close()


MASS_PAIRS = ((0.3, 0.3), (0.3, 1.2), (1.2, 0.3))
# relative momentum error after the impact, the damping's impulse added back: first MI355X run without that term 2.1 - 2.4 %, all of it the damping
# (exp(-0.04 (1 + v) 0.48 s)); with it 3e-5 - 1.3e-4 (the trapezoid over step samples).  1e-3 keeps a sevenfold margin, where baked masses miss the
# (0.3, 1.2) env by 2.5x or more
MOMENTUM_TOL = 1e-3


def test_mass_sets_the_momentum_exchange():
    """pandaPlay-v0, both blocks frictionless, faces aligned along x, the arm parked: block A at 0.3 m/s hits block B at rest.  mA vA + mB vB, with the env's
    masses, is what it was before the impact.  With the baked 0.3 / 0.3 the (0.3, 1.2) env would miss that balance by more than 2x."""
    gid = 'pandaPlay-v0'
    n = len(MASS_PAIRS)
    env = make(gid, n, 4)
    hold = _park_arm(env, (-0.15, 0.0, 0.25))
    names = env.dynamics_names
    d = env.get_dynamics()
    fr, ms = d['friction'].clone(), d['mass'].clone()
    for b in ('block', 'block2'):
        fr[:, names['friction'].index(b)] = 0.0
    ms[:, names['mass'].index('block')] = torch.tensor([p[0] for p in MASS_PAIRS], device=env.device)
    ms[:, names['mass'].index('block2')] = torch.tensor([p[1] for p in MASS_PAIRS], device=env.device)
    env.set_dynamics(friction=fr, mass=ms)
    lay = env.state_layout
    rec = env.get_state()[:, :128].clone()
    v0 = 0.3
    _place(rec, lay, 0, torch.tensor([0.0, 0.25, 0.0], device=env.device), torch.tensor([v0, 0.0, 0.0], device=env.device))
    _place(rec, lay, 1, torch.tensor([0.12, 0.25, 0.0], device=env.device), 0.0)
    env.set_state(rec)
    fa, fb = lay['free0'][0], lay['free1'][0]
    vs = [np.stack([np.full(n, v0), np.zeros(n)])]
    for _ in range(12):
        env.step(hold)
        s = env.get_state().cpu().numpy()
        vs.append(np.stack([s[:, fa + 7], s[:, fb + 7]]))
    vs = np.stack(vs)                                   # [13, 2, n]: x velocities of A and B after every step
    va, vb = vs[-1]
    mA, mB = np.array([p[0] for p in MASS_PAIRS]), np.array([p[1] for p in MASS_PAIRS])
    m = np.stack([mA, mB])
    damp = K_LIN_DAMP * (m * (1.0 + np.abs(vs)) * vs).sum(1)          # [13, n]: the damping's force on the pair
    p_after = mA * va + mB * vb + (0.5 * (damp[1:] + damp[:-1])).sum(0) * (12 / 300.0)
    p_before = mA * v0
    print('velocities after', va.tolist(), vb.tolist(), 'momentum', p_after.tolist(), 'before', p_before.tolist())
    assert np.all(s[:, fb] > 0.12 + 0.005), s[:, fb]          # B was hit
    rel = np.abs(p_after - p_before) / p_before
    assert np.all(rel < MOMENTUM_TOL), ('momentum after', p_after.tolist(), 'before', p_before.tolist(), 'relative error', rel.tolist())
    env.close()


def test_set_is_asynchronous_and_acts_from_the_next_step():
    """behind a ~1 s sleep kernel, set_dynamics with device tensors and a device mask returns while the stream is busy.  Values set between two autoreset
    steps act in the second: its result equals a handle that starts from the first step's state with those values, and differs from one without them.
    Neither reset() nor autoreset changes them."""
    gid, n, seed = 'UR5PlayAbsRPY1Obj-v0', 32, 6
    kw = dict(autoreset=True, max_episode_steps=0, end_on_fault=False)
    A = make(gid, n, seed, **kw)
    A.reset()
    acts = actions(A, 6, seed)
    masks = end_masks(n, 6, seed, A.device, 0.2)
    for t in range(3):
        A.step(acts[t], end_mask=masks[t])
    rnd = random_dynamics(A, seed)
    m = (torch.arange(n, device=A.device) % 2 == 0).to(torch.uint8)
    torch.cuda.synchronize()
    st, ep = A.get_state(), A.episode_steps
    stream = torch.cuda.current_stream(A.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); torch.cuda._sleep(10 ** 7); t1.record()
    torch.cuda.synchronize()
    cycles = int(min(10 ** 7 * 1000.0 / max(t0.elapsed_time(t1), 1e-3), 5e9))
    torch.cuda._sleep(cycles)
    A.set_dynamics(friction=rnd['friction'], mass=rnd['mass'], mask=m)
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy
    outs = {}
    for name, vals in (('with', True), ('without', False)):
        E = make(gid, n, seed, **kw)
        E.set_state(st)
        E.episode_steps = ep
        if vals:
            E.set_dynamics(friction=rnd['friction'], mass=rnd['mass'], mask=m)
        res = []
        for t in range(3, 6):
            o, r, d, _ = E.step(acts[t], end_mask=masks[t])
            res.append(snap(E, o))
        outs[name] = (res, E.get_state())
        E.close()
    res = []
    for t in range(3, 6):
        o, r, d, _ = A.step(acts[t], end_mask=masks[t])
        res.append(snap(A, o))
    sa = A.get_state()
    for t in range(3):
        for k in res[t]:
            assert torch.equal(res[t][k], outs['with'][0][t][k]), (t, k)
    assert torch.equal(sa, outs['with'][1])
    assert not torch.equal(sa, outs['without'][1])
    base = make(gid, n, seed).get_dynamics()
    want = {k: torch.where(m.bool()[:, None], rnd[k], base[k]) for k in rnd}
    A.reset()
    A.step(acts[0], end_mask=torch.ones(n, dtype=torch.uint8, device=A.device))
    d = A.get_dynamics()
    assert torch.equal(d['friction'], want['friction']) and torch.equal(d['mass'], want['mass'])
    A.close()


def test_bad_arguments_are_refused():
    from roboticsplayroompybullet_amd import _lib
    n = 8
    env = make('UR5PlayAbsRPY1Obj-v0', n, 0)
    d = env.get_dynamics()
    lib, s = env.lib, env._stream()
    fp = C.c_void_p(d['friction'].data_ptr())
    for rows in (0, 2, n - 1, n + 1, -1):
        assert lib.rp_set_dynamics(env.h, fp, None, rows, None, s) == -1, rows          # RP_ERR_ARG
    assert lib.rp_set_dynamics(env.h, None, None, 1, None, s) == -1
    assert lib.rp_set_dynamics(env.h, fp, None, n, None, s) == 0
    with pytest.raises(ValueError):
        env.set_dynamics(friction=d['friction'][:, :-1])
    with pytest.raises(ValueError):
        env.set_dynamics(mass=d['mass'][:3])
    with pytest.raises(ValueError):
        env.set_dynamics(friction=d['friction'][0], mask=torch.ones(n + 1, dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError):
        env.set_dynamics()
    with pytest.raises(ValueError):
        env.set_dynamics(friction=-d['friction'][0].cpu())
    with pytest.raises(ValueError):
        env.set_dynamics(mass=np.zeros(d['mass'].shape[1]))
    with pytest.raises(ValueError):
        env.set_dynamics(mass=[float('nan')] * d['mass'].shape[1])
    torch.cuda.synchronize()
    assert torch.equal(env.get_dynamics()['friction'], d['friction'])
    env.close()
