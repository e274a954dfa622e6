"""Per-env joint and body state by column (rp_get_kinematics / rp_set_kinematics; VecPlayEnv.get_kinematics, set_kinematics, set_body, set_joint) and envs
cloned on the device (rp_copy_envs / clone_envs).  Run with -m gpu on the MI355X box.

The feature moves words of the state record, so it is held bit for bit against the route the library already has - rp_get_state, an edit of the rows through
VecPlayEnv.state_layout, rp_set_state - which carries the oracle parity of the step; on top of that: the observations show what was set (the dial against the
oracle's calc_state), a thrown block follows the substep recurrence in fp64, a clone is a gather of the rows as they were before the call, and no call waits for
the device.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_wrench import AIR, DT, G, KD, OBS, SUBSTEPS, _close, _park, _recur, actions, make, model_of, snap

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

HEADLINE, PICK, REACH, WIDE = 'UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'UR5Reach-v0', 'pandaPlay-v0'
IDS = (HEADLINE, PICK, REACH, WIDE)
REC = 128          # floats of a state record; a state row's contact cache lies behind it


def bits(t):
    """a float tensor's bit patterns: equality that tells -0.0 from 0.0 and holds for NaN"""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def dims(env):
    na, nf, nj = C.c_int32(), C.c_int32(), C.c_int32()
    assert env.lib.rp_get_wrench_dims(env.h, C.byref(na), C.byref(nf), C.byref(nj)) == 0
    return na.value, nf.value, nj.value


def layout_columns(env):
    """(record offsets of the pos columns, of the vel columns) from VecPlayEnv.state_layout: the blob route's view of the same words"""
    lay = env.state_layout
    na, nf, nj = dims(env)
    pos = [lay['q'][0] + i for i in range(na)] + [lay['free%d' % f][0] + j for f in range(nf) for j in range(7)] + [lay['jq'][0] + k for k in range(nj)]
    vel = [lay['qd'][0] + i for i in range(na)] + [lay['free%d' % f][0] + 7 + j for f in range(nf) for j in range(6)] + [lay['jqd'][0] + k for k in range(nj)]
    dev = env.device
    return torch.tensor(pos, dtype=torch.long, device=dev), torch.tensor(vel, dtype=torch.long, device=dev)


def warm(env, seed, steps=4):
    env.reset()
    acts = actions(env, steps, seed)
    for t in range(steps):
        env.step(acts[t])


def some_mask(n, dev):
    return (torch.arange(n, device=dev) % 3 != 1).to(torch.uint8)


def perturbed(env, seed):
    """(pos', vel') near the env's own: joints and positions moved by up to 2 cm / 0.02 rad, the free bodies lifted 2 cm, the rotating bodies' quaternions
    turned a little and normalised, velocities changed by up to 0.1 - states the step can run on from"""
    kin = env.get_kinematics()
    kind, mdl = model_of(env)
    names = env.kinematics_names
    g = torch.Generator().manual_seed(seed)
    p, v = kin['pos'].clone(), kin['vel'].clone()
    dp = (0.04 * torch.rand(p.shape, generator=g) - 0.02).to(env.device)
    for f, fb in enumerate(mdl['free']):
        c = names['pos'].index(env.wrench_names[mdl['n_arm'] + f] + '.x')
        dp[:, c + 2] += 0.02
        if fb['rot_locked']:
            dp[:, c + 3:c + 7] = 0.0
    p += dp
    for k, nm in enumerate(names['pos']):
        if nm.endswith('.qx'):
            p[:, k:k + 4] /= p[:, k:k + 4].norm(dim=1, keepdim=True)
    v += (0.2 * torch.rand(v.shape, generator=g) - 0.1).to(env.device)
    return p, v


# ---------------------------------------------------------------- 1. the tables
@pytest.mark.parametrize('n', (5, 300))
@pytest.mark.parametrize('gid', IDS)
def test_table_semantics(gid, n):
    env = make(gid, n, 1)
    warm(env, 2)
    na, nf, nj = dims(env)
    kind, mdl = model_of(env)
    assert (na, nf, nj) == (mdl['n_arm'], len(mdl['free']), len(mdl['joint1']))
    names = env.kinematics_names
    n_pos, n_vel = na + 7 * nf + nj, na + 6 * nf + nj
    assert (len(names['pos']), len(names['vel'])) == (n_pos, n_vel)
    pi, vi = layout_columns(env)
    st0 = env.get_state()
    kin = env.get_kinematics()
    assert kin['pos'].shape == (n, n_pos) and kin['vel'].shape == (n, n_vel) and kin['pos'].dtype == torch.float32
    assert same(kin['pos'], st0[:, pi]) and same(kin['vel'], st0[:, vi])          # the getter reads the layout's words
    assert bool(kin['pos'][:, :na].abs().sum() > 0)
    other = torch.ones(st0.shape[1], dtype=torch.bool, device=env.device)          # every word of a row that is no kinematics column: record rest + cache
    other[pi] = False; other[vi] = False
    steps0 = torch.arange(n, dtype=torch.int32, device=env.device) * 3 + 1
    env.episode_steps = steps0
    g = torch.Generator().manual_seed(3)

    def rnd(rows, k):
        t = torch.randn((rows, k), generator=g)
        t[0, 0] = -0.0
        return t.to(env.device)

    lib, s = env.lib, env._stream()
    # rows = N, no mask, both halves (arbitrary bits: the words are written verbatim, quaternions too)
    p1, v1 = rnd(n, n_pos), rnd(n, n_vel)
    env.set_kinematics(pos=p1, vel=v1)
    k = env.get_kinematics()
    assert same(k['pos'], p1) and same(k['vel'], v1)
    st = env.get_state()
    assert same(st[:, pi], p1) and same(st[:, vi], v1) and same(st[:, other], st0[:, other])
    # rows = 1, no mask, pos only
    p2 = rnd(1, n_pos)
    env.set_kinematics(pos=p2[0])
    k = env.get_kinematics()
    assert same(k['pos'], p2.expand(n, -1)) and same(k['vel'], v1)
    # rows = N, mask, vel only
    m = some_mask(n, env.device)
    mb = m.bool()[:, None]
    v3 = rnd(n, n_vel)
    env.set_kinematics(vel=v3, mask=m)
    k = env.get_kinematics()
    want_v = torch.where(mb, v3, v1)
    assert same(k['pos'], p2.expand(n, -1)) and same(k['vel'], want_v)
    # rows = 1, mask, both halves (through the C ABI: one row each)
    p4, v4 = rnd(1, n_pos), rnd(1, n_vel)
    inv = 1 - m
    assert lib.rp_set_kinematics(env.h, C.c_void_p(p4.data_ptr()), C.c_void_p(v4.data_ptr()), 1, C.c_void_p(inv.data_ptr()), 0, s) == 0
    k = env.get_kinematics()
    want_p = torch.where(mb, p2.expand(n, -1), p4.expand(n, -1))
    want_v = torch.where(mb, want_v, v4.expand(n, -1))
    assert same(k['pos'], want_p) and same(k['vel'], want_v)
    # rows = N, mask, pos only; a single row beside an [N, .] half is broadcast by VecPlayEnv
    p5 = rnd(n, n_pos)
    env.set_kinematics(pos=p5, vel=v4[0], mask=m)
    want_p = torch.where(mb, p5, want_p)
    want_v = torch.where(mb, v4.expand(n, -1), want_v)
    k = env.get_kinematics()
    assert same(k['pos'], want_p) and same(k['vel'], want_v)
    # one half of the getter at a time
    only_p, only_v = torch.zeros_like(want_p), torch.zeros_like(want_v)
    assert lib.rp_get_kinematics(env.h, C.c_void_p(only_p.data_ptr()), None, s) == 0
    assert lib.rp_get_kinematics(env.h, None, C.c_void_p(only_v.data_ptr()), s) == 0
    assert same(only_p, want_p) and same(only_v, want_v)
    # refused arguments (RP_ERR_ARG) leave everything as it is
    pp, vp = C.c_void_p(p1.data_ptr()), C.c_void_p(v1.data_ptr())
    assert lib.rp_set_kinematics(env.h, None, None, n, None, 0, s) == -1
    assert lib.rp_set_kinematics(env.h, pp, vp, 2, None, 0, s) == -1
    assert lib.rp_set_kinematics(env.h, pp, vp, 0, None, 0, s) == -1
    assert lib.rp_set_kinematics(env.h, pp, vp, n, None, 2, s) == -1
    assert lib.rp_set_kinematics(env.h, pp, vp, n, None, 3, s) == -1
    assert lib.rp_get_kinematics(env.h, None, None, s) == -1
    src = torch.arange(n, dtype=torch.int32, device=env.device)
    assert lib.rp_copy_envs(env.h, None, None, 0, s) == -1
    assert lib.rp_copy_envs(env.h, C.c_void_p(src.data_ptr()), None, 2, s) == -1
    with pytest.raises(ValueError):
        env.set_kinematics()
    for bad in (p1[:, :-1], p1[:3] if n > 3 else p1[:2], p1.reshape(-1)):
        with pytest.raises(ValueError):
            env.set_kinematics(pos=bad)
    with pytest.raises(ValueError):
        env.set_kinematics(vel=np.full(n_vel, np.nan))
    with pytest.raises(ValueError):
        env.set_kinematics(vel=v1, mask=torch.ones(n + 1, dtype=torch.uint8, device=env.device))
    if nf:
        body = env.wrench_names[na]
        badq = kin['pos'][0].cpu().numpy().copy()
        c = names['pos'].index(body + '.qx')
        badq[c:c + 4] = [0.0, 0.0, 0.0, 1.01]
        with pytest.raises(ValueError):
            env.set_kinematics(pos=badq)
        with pytest.raises(ValueError):
            env.set_body(body, quat=[0.0, 0.0, 0.0, 1.01])
        with pytest.raises(ValueError):
            env.set_body(body)
        with pytest.raises(KeyError):
            env.set_joint(body + '.x', q=0.0)
    with pytest.raises(KeyError):
        env.set_body('no such body', pos=[0.0, 0.0, 0.0])
    with pytest.raises(KeyError):
        env.set_body(names['pos'][0], pos=[0.0, 0.0, 0.0])          # a dof is no free body
    with pytest.raises(KeyError):
        env.set_joint('no such joint', q=0.0)
    with pytest.raises(ValueError):
        env.set_joint(names['pos'][0])
    with pytest.raises(ValueError):
        env.set_joint(names['pos'][0], q=float('inf'))
    with pytest.raises(ValueError):
        env.clone_envs(list(range(n - 1)) + [n])
    with pytest.raises(ValueError):
        env.clone_envs([-1] + list(range(1, n)))
    with pytest.raises(ValueError):
        env.clone_envs(list(range(n - 1)))
    st = env.get_state()
    assert same(st[:, pi], want_p) and same(st[:, vi], want_v) and same(st[:, other], st0[:, other])          # nothing else moved, all along
    assert torch.equal(env.episode_steps, steps0)
    # the conveniences: one column group each, the rest of the row untouched
    x = torch.arange(n, dtype=torch.float32, device=env.device) * 0.01
    env.set_joint(names['pos'][1], q=x, qd=0.25, mask=m)
    want_p[:, 1] = torch.where(m.bool(), x, want_p[:, 1])
    want_v[:, 1] = torch.where(m.bool(), torch.full_like(x, 0.25), want_v[:, 1])
    if nj:
        env.set_joint(names['pos'][-1], q=-0.5)
        want_p[:, -1] = -0.5
    if nf:
        body = env.wrench_names[na + nf - 1]
        c, cv = names['pos'].index(body + '.x'), names['vel'].index(body + '.vx')
        env.set_body(body, pos=[0.1, 0.2, 0.3], ang_vel=torch.stack([x, -x, 2 * x], 1))
        want_p[:, c:c + 3] = torch.tensor([0.1, 0.2, 0.3], device=env.device)
        want_v[:, cv + 3:cv + 6] = torch.stack([x, -x, 2 * x], 1)
        s5 = float(np.sqrt(0.5))
        env.set_body(body, quat=[s5, 0.0, 0.0, s5], lin_vel=[1.0, 2.0, 3.0], mask=inv)
        want_p[:, c + 3:c + 7] = torch.where(mb, want_p[:, c + 3:c + 7], torch.tensor([s5, 0.0, 0.0, s5], device=env.device))
        want_v[:, cv:cv + 3] = torch.where(mb, want_v[:, cv:cv + 3], torch.tensor([1.0, 2.0, 3.0], device=env.device))
    k = env.get_kinematics()
    assert same(k['pos'], want_p) and same(k['vel'], want_v)
    assert same(env.get_state()[:, other], st0[:, other])
    env.close()


def test_stateless_contacts_have_no_cache_to_clear_or_copy():
    """under RP_CFG_STATELESS_CONTACTS a row is the record alone: RP_KIN_CLEAR_CONTACTS does nothing, rp_copy_envs moves records"""
    n = 5
    env = make(HEADLINE, n, 1, persistent_manifolds=False)
    warm(env, 2)
    st0 = env.get_state()
    assert st0.shape == (n, REC)
    pi, vi = layout_columns(env)
    p, v = perturbed(env, 4)
    m = some_mask(n, env.device)
    env.set_kinematics(pos=p, vel=v, mask=m, clear_contacts=True)
    want = st0.clone()
    rows = m.bool().nonzero()[:, 0]
    want[rows[:, None], pi[None]] = p[rows]
    want[rows[:, None], vi[None]] = v[rows]
    assert same(env.get_state(), want)
    src = torch.tensor([4, 3, 2, 1, 0], dtype=torch.int32, device=env.device)
    env.clone_envs(src)
    assert same(env.get_state(), want[src.long()])
    torch.cuda.synchronize()
    env.close()


# ---------------------------------------------------------------- 2. the blob route gives the same bits
@pytest.mark.parametrize('pipe', ('default', 'fused1'))
@pytest.mark.parametrize('clear', (False, True))
@pytest.mark.parametrize('gid', IDS)
def test_set_kinematics_is_the_blob_route_bit_for_bit(gid, clear, pipe):
    """A: set_kinematics(p', v', mask, clear_contacts); B (same id, seed, history): get_state, the same columns edited through state_layout (and the masked rows'
    cache zeroed when clear), set_state.  The state rows agree bit for bit, and so does every output of three more steps."""
    n, seed = 8, 5
    A, B = make(gid, n, seed), make(gid, n, seed)
    for E in (A, B):
        if pipe == 'fused1':
            E.set_fused(1)
        warm(E, seed + 1)
    assert same(A.get_state(), B.get_state())
    pi, vi = layout_columns(A)
    p, v = perturbed(A, seed + 2)
    m = some_mask(n, A.device)
    A.set_kinematics(pos=p, vel=v, mask=m, clear_contacts=clear)
    rows0 = B.get_state().clone()
    rows = rows0.clone()
    r = m.bool().nonzero()[:, 0]
    rows[r[:, None], pi[None]] = p[r]
    rows[r[:, None], vi[None]] = v[r]
    if clear:
        rows[r, REC:] = 0.0
    B.set_state(rows)
    sa = A.get_state()
    assert same(sa, B.get_state())
    assert all(not same(sa[e], rows0[e]) for e in r.tolist())          # (the call did set something in every masked env)
    acts = actions(A, 3, seed + 3)
    for t in range(3):
        oa, ra, _, ia = A.step(acts[t])
        ob, rb, _, ib = B.step(acts[t])
        for k in OBS:
            assert same(oa[k], ob[k]), (t, k)
        assert same(ra, rb) and same(ia['is_success'], ib['is_success']) and same(ia['target_poses'], ib['target_poses']) and same(ia['status'], ib['status']), t
        assert same(A.pack, B.pack), t
        assert int((ia['status'] & 1).sum()) == 0, t          # (states the step can run on from: nothing blew up)
    assert same(A.get_state(), B.get_state())
    A.close(); B.close()


# ---------------------------------------------------------------- 3. neutrality
@pytest.mark.parametrize('gid', (HEADLINE, PICK, WIDE))
def test_writing_back_what_was_read_changes_no_bit(gid):
    """with live contacts (the arm parked, the block at rest on the table: a cache row that is not empty), set_kinematics(**get_kinematics()) leaves every state row
    as it is; a masked write with clear_contacts empties the masked envs' cache rows and touches no other env"""
    n = 6
    env = make(gid, n, 4)
    _park(env)
    st0 = env.get_state()
    assert bool((st0[:, REC:] != 0).any(1).all())          # every env has contact history
    env.set_kinematics(**env.get_kinematics())
    assert same(env.get_state(), st0)
    m = some_mask(n, env.device)
    env.set_kinematics(**env.get_kinematics(), mask=m)
    assert same(env.get_state(), st0)
    p, v = perturbed(env, 6)
    env.set_kinematics(pos=p, vel=v, mask=m, clear_contacts=True)
    st = env.get_state()
    keep = ~m.bool()
    assert same(st[keep], st0[keep])
    assert not bool(bits(st[m.bool(), REC:]).any())
    assert same(st[m.bool(), :REC][:, layout_columns(env)[0]], p[m.bool()])
    env.close()


# ---------------------------------------------------------------- 4. through the public observations
@pytest.mark.parametrize('gid', (HEADLINE,))
def test_the_observations_show_what_was_set(gid):
    """door to 0.3 rad, the drawer 5 cm along its axis (world y: achieved_goal's drawer entry), the dial to 2.5 rad, the six main arm dofs to rest + 0.1 at rest:
    calc_state's joints carry the arm within 1e-6, achieved_goal's drawer and door entries moved by the set amounts within 1e-5, and the quaternion-free entries of
    achieved_goal (block position, drawer, door, button, dial through dial_to_0_1_range) equal the fp64 oracle's calc_state after OracleEnv.set_state with the same
    vector within 1e-5 (fp32 forward kinematics of values below 1: a few 1e-7)"""
    from oracle import OracleEnv
    n = 8
    env = make(gid, n, 3)
    warm(env, 4)
    kind, mdl = model_of(env)
    na, nf, nj = dims(env)
    names = env.kinematics_names
    ag0 = env.calc_state()['achieved_goal'].clone()
    i_drawer, i_door, i_dial = 7 * (nf - 1), 7 * (nf - 1) + 1, 7 * (nf - 1) + 3
    kin0 = env.get_kinematics()
    door0 = kin0['pos'][:, names['pos'].index('door')].clone()
    c = names['pos'].index('drawer.x')
    drawer0 = kin0['pos'][:, c:c + 3].clone()
    env.set_joint('door', q=0.3)
    env.set_body('drawer', pos=drawer0 + torch.tensor([0.0, 0.05, 0.0], device=env.device))
    env.set_joint('dial', q=2.5, qd=0.0)
    rest = [float(np.float32(x)) + 0.1 for x in mdl['rest'][:6]]
    for i in range(6):
        env.set_joint(names['pos'][i], q=rest[i], qd=0.0)
    obs = env.calc_state()
    joints = obs['joints'].cpu().numpy().astype(np.float64)
    ag = obs['achieved_goal'].cpu().numpy().astype(np.float64)
    a0 = ag0.cpu().numpy().astype(np.float64)
    print('joints error %.3e' % np.abs(joints[:, :6] - np.array(rest)).max())
    assert np.abs(joints[:, :6] - np.array(rest)).max() <= 1e-6
    d_drawer, d_door = ag[:, i_drawer] - a0[:, i_drawer], ag[:, i_door] - a0[:, i_door]
    print('drawer moved by %s, door at %s' % (d_drawer, ag[:, i_door]))
    assert np.abs(d_drawer - 0.05).max() <= 1e-5
    assert np.abs(d_door - (0.3 - door0.cpu().numpy().astype(np.float64))).max() <= 1e-5
    assert np.abs(ag[:, i_door] - 0.3).max() <= 1e-5
    kin = env.get_kinematics()
    p, v = kin['pos'].cpu().numpy().astype(np.float64), kin['vel'].cpu().numpy().astype(np.float64)
    free = [c for c in range(7 * (nf - 1)) if c % 7 < 3] + list(range(7 * (nf - 1), 7 * (nf - 1) + 4))
    worst = 0.0
    for e in (0, 3, 7):
        o = OracleEnv(kind)
        o.reset()
        s = np.concatenate([p[e, :na], v[e, :na]] + [np.concatenate([p[e, na + 7 * f:na + 7 * f + 7], v[e, na + 6 * f:na + 6 * f + 6]]) for f in range(nf)]
                           + [p[e, na + 7 * nf:], v[e, na + 6 * nf:]])
        assert len(s) == len(o.get_state())
        o.set_state(s)
        want = np.asarray(o.calc_state()['achieved_goal'], dtype=np.float64)
        err = np.abs(ag[e, free] - want[free])
        worst = max(worst, err.max())
        assert err.max() <= 1e-5, (e, ag[e].tolist(), want.tolist())
        assert abs(want[i_dial] - (2.5 % 2) / 2.2) < 1e-6          # (the dial went through dial_to_0_1_range)
    print('achieved_goal against the oracle: worst %.3e' % worst)
    env.close()


# ---------------------------------------------------------------- 5. free flight
@pytest.mark.parametrize('gid', (HEADLINE, PICK, WIDE))
def test_a_thrown_block_follows_the_recurrence(gid):
    """set_body puts every env's block at AIR, unrotated, with its own linear velocity and a spin about one principal axis (the recurrence has no gyroscopic term: a
    body spinning about a principal axis has none); after one step both velocities are _recur's within _close's bound, and the position has advanced by dt times the
    sum of the twelve substep velocities (the integrator moves a body with the velocity it has just computed) within 1e-5"""
    n = 8
    env = make(gid, n, 2)
    env.reset()
    rng = np.random.default_rng(7)
    v0 = torch.tensor(rng.uniform(-0.5, 0.5, (n, 3)), dtype=torch.float32)
    w0 = np.zeros((n, 3))
    w0[np.arange(n), np.arange(n) % 3] = rng.uniform(-1.0, 1.0, n)
    w0 = torch.tensor(w0, dtype=torch.float32)
    env.set_body('block', pos=AIR, quat=(0.0, 0.0, 0.0, 1.0), lin_vel=v0, ang_vel=w0.to(env.device), clear_contacts=True)
    names = env.kinematics_names
    c, cv = names['pos'].index('block.x'), names['vel'].index('block.vx')
    kin = env.get_kinematics()
    assert same(kin['pos'][:, c:c + 7], torch.tensor(AIR + (0.0, 0.0, 0.0, 1.0), device=env.device).expand(n, -1))
    assert same(kin['vel'][:, cv:cv + 6], torch.cat([v0, w0], 1).to(env.device))
    env.step(actions(env, 1, 3)[0])
    kin = env.get_kinematics()
    x = kin['pos'][:, c:c + 3].cpu().numpy().astype(np.float64)
    v = kin['vel'][:, cv:cv + 3].cpu().numpy().astype(np.float64)
    w = kin['vel'][:, cv + 3:cv + 6].cpu().numpy().astype(np.float64)
    grav = np.array([0.0, 0.0, G])
    assert _close(v, _recur(v0.numpy(), grav))
    assert _close(w, _recur(w0.numpy(), np.zeros(3)))
    vk, travelled = v0.numpy().astype(np.float64), np.zeros((n, 3))
    for _ in range(SUBSTEPS):
        vk = vk - DT * KD * (1.0 + np.linalg.norm(vk, axis=-1, keepdims=True)) * vk + DT * grav
        travelled += DT * vk
    err = np.abs(x - (np.array(AIR, dtype=np.float32).astype(np.float64) + travelled))
    print('position error %.3e' % err.max())
    assert err.max() <= 1e-5
    env.close()


# ---------------------------------------------------------------- 6. clones
def _maps(n, seed):
    g = torch.Generator().manual_seed(seed)
    k = max(2, n // 32)
    e = torch.arange(n)
    return {'identity': e, 'reversal': n - 1 - e, 'rotation': (e + 1) % n, 'block_broadcast': (e // k) * k,
            'many_to_one': torch.randint(0, max(1, n // 3), (n,), generator=g), 'permutation': torch.randperm(n, generator=g)}


@pytest.mark.parametrize('n', (5, 300))
@pytest.mark.parametrize('gid', IDS)
def test_clone_envs_is_a_gather_of_the_rows_as_they_were(gid, n):
    env = make(gid, n, 8)
    warm(env, 9)
    dev = env.device
    first = env.get_state().clone()
    assert not same(first[0], first[1])
    all_steps = torch.arange(n, dtype=torch.int32, device=dev) * 7 + 2
    for what, src in _maps(n, 10).items():
        for masked in (False, True):
            env.set_state(first)
            env.episode_steps = all_steps
            before = env.get_state()
            m = some_mask(n, dev) if masked else None
            with_steps = what != 'rotation'
            src_dev = src.to(device=dev, dtype=torch.int64 if what == 'reversal' else torch.int32)
            env.clone_envs(src_dev if what != 'many_to_one' else src.tolist(), mask=m, episode_steps=with_steps)
            after = env.get_state()
            sel = torch.ones(n, dtype=torch.bool, device=dev) if m is None else m.bool()
            want = torch.where(sel[:, None], before[src.to(dev)], before)
            assert same(after, want), (what, masked)
            want_steps = torch.where(sel, all_steps[src.to(dev)], all_steps) if with_steps else all_steps
            assert torch.equal(env.episode_steps, want_steps), (what, masked)
    # a device src is not range-checked: entries outside [0, N) leave their envs alone, and nothing faults
    env.set_state(first)
    before = env.get_state()
    src = torch.randperm(n, generator=torch.Generator().manual_seed(11)).to(torch.int32)
    src[0], src[n - 1], src[n // 2] = -1, n, 2 ** 31 - 1
    env.clone_envs(src.to(dev))
    torch.cuda.synchronize()
    after = env.get_state()
    ok = ((src >= 0) & (src < n)).to(dev)
    want = torch.where(ok[:, None], before[src.clamp(0, n - 1).long().to(dev)], before)
    assert same(after, want)
    env.close()


@pytest.mark.parametrize('gid', (HEADLINE, WIDE))
def test_cloned_envs_step_like_rows_set_from_a_gather(gid):
    """A: clone_envs(src); B: set_state(before[src]) - the route without the call.  Three steps with the same actions: every output equal bit for bit, and env e of
    both is env src[e] of an untouched twin given action[e]"""
    n, seed = 8, 12
    A, B = make(gid, n, seed), make(gid, n, seed)
    for E in (A, B):
        warm(E, seed + 1)
    before = B.get_state().clone()
    src = torch.tensor([3, 3, 0, 7, 7, 7, 1, 6], dtype=torch.int32, device=A.device)
    A.clone_envs(src)
    B.set_state(before[src.long()])
    assert same(A.get_state(), B.get_state())
    acts = actions(A, 3, seed + 2)
    for t in range(3):
        oa, ra, _, ia = A.step(acts[t])
        ob, rb, _, ib = B.step(acts[t])
        for k in OBS:
            assert same(oa[k], ob[k]), (t, k)
        assert same(ra, rb) and same(ia['status'], ib['status']) and same(ia['target_poses'], ib['target_poses']), t
    assert same(A.get_state(), B.get_state())
    A.close(); B.close()


# ---------------------------------------------------------------- 7. asynchrony
@pytest.mark.parametrize('gid', (HEADLINE, WIDE))
def test_the_calls_never_wait_for_the_device(gid):
    """behind a ~1 s sleep kernel, set_kinematics (device tensors, device mask, clear_contacts), set_body and set_joint with device tensors and clone_envs with a
    device src all return while the stream is busy; the state they leave is the one the same calls leave on an idle stream"""
    n, seed = 16, 6
    A, B = make(gid, n, seed), make(gid, n, seed)
    for E in (A, B):
        warm(E, seed + 1)
    dev = A.device
    p, v = perturbed(A, seed + 2)
    m = some_mask(n, dev)
    x = torch.rand((n, 3), device=dev)
    q = torch.rand(n, device=dev) * 0.1
    src = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(device=dev, dtype=torch.int32)
    link = A.kinematics_names['pos'][0]

    def calls(E):
        E.set_kinematics(pos=p, vel=v, mask=m, clear_contacts=True)
        E.set_body('block', pos=x, lin_vel=x, mask=1 - m)
        E.set_joint(link, q=q, qd=q)
        E.clone_envs(src, mask=m)

    calls(B)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); torch.cuda._sleep(10 ** 7); t1.record()
    torch.cuda.synchronize()
    cycles = int(min(10 ** 7 * 1000.0 / max(t0.elapsed_time(t1), 1e-3), 5e9))
    torch.cuda._sleep(cycles)
    calls(A)
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy
    assert same(A.get_state(), B.get_state())
    assert torch.equal(A.episode_steps, B.episode_steps)
    a = actions(A, 1, seed)[0]
    oa, ob = A.step(a)[0], B.step(a)[0]
    for k in OBS:
        assert same(oa[k], ob[k]), k
    A.close(); B.close()
