"""The per-env parameter tables - friction, mass, wrenches, gravity, motor gain and strength - held to the CPU oracle IN CONTACT, lock-step with contact history.  Run with
-m gpu on the MI355X box.

The property tests (test_gpu_dynamics / _wrench / _actuation) are sharp where a body is alone and say "env k reaches env k only"; they are silent about a wrong value reaching
the right env inside a contact row or one of k_solve2's three motor-row rebuilds.  Here the device runs three short contact scenarios (tests/param_scenarios.py) free, every env
under its own row of all tables, half the envs redrawn at step 20 through the masked setters.  Before every step an fp32 oracle and its two CPU twins (arm joints one ulp /
1e-5 off) take the device's record and cache row, the device's joint targets, and the env's own rows of the tables READ BACK FROM THE DEVICE (get_dynamics / get_wrench /
get_actuation) - not from the generator that wrote them; both take the step and are compared field by field as tests/test_gpu_dist_a.py compares them.  The oracle's
parameters are held by closed forms in tests/test_oracle_params.py, which also shows that putting any one value block back to its default moves these very scenarios by more
than ten times the bounds below in 14 - 82 % of the env-steps: a kernel that dropped or misplaced a block cannot pass.

pandaPlay-v0 (the wide build, model W) is not here: gpu_debug.oracle_state_from_record does not carry its record, so W stays with the property tests."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import cache_rows  # noqa: E402
import param_scenarios as ps  # noqa: E402
from test_gpu_dist_a import REC, actions_a, free_positions, positions  # noqa: E402,F401  (actions_a: the scenarios' scripts replace the random actions)
from test_oracle_params import TWIN_SAME  # noqa: E402
from tolerances import N_MAIN  # noqa: E402

pytestmark = pytest.mark.gpu
TABLES = ('friction', 'mass', 'wrench', 'gravity', 'motor_gain', 'motor_strength')


def _device_tables(env):
    """every env's rows as the device holds them: float32 numpy arrays by TABLES"""
    t = dict(env.get_dynamics())
    t['wrench'] = env.get_wrench()
    t.update(env.get_actuation())
    return {k: t[k].cpu().numpy() for k in TABLES}


def _write_tables(env, tab, mask=None):
    dev = {k: torch.tensor(v).to(env.device) for k, v in tab.items()}
    m = None if mask is None else torch.tensor(mask.astype(np.uint8)).to(env.device)
    env.set_dynamics(friction=dev['friction'], mass=dev['mass'], mask=m)
    env.set_wrench(dev['wrench'], mask=m)
    env.set_actuation(gravity=dev['gravity'], motor_gain=dev['motor_gain'], motor_strength=dev['motor_strength'], mask=m)


@pytest.mark.parametrize('kind', ps.KINDS)
def test_parameter_tables_lockstep_with_contact_history(kind):
    """One scenario (U scatter start, P grasp-and-lift, V the gripper pressed onto the table and the block), 16 envs x 40 steps, the default pipeline with three groups.  What
    each reaches, asserted from debug_row_counts and rpo_last_num_tors over the compared env-steps:
      U  light envs (neither arm nor spanning contacts): the block tumbling on the furniture (inertia scale, friction and mass of cached points), the drawer under a tilted
         gravity - k_solve2's four-env path;
      P  spanning contacts (arm against a movable body: the pads on the block) = the heavy, residual-form path with its friction bounds -+ mu lambda; torsional rows; a block
         of non-baked mass and friction held under non-default gravity and strength (the device holds it in the air in at least one env);
      V  arm contacts without spanning ones (hull contacts of arm links with per-env mu, motor strength against contact), torsional rows, and env-steps with 15 or more
         contacts (BIG, heavy_solve's two-register form: tests/test_oracle_params.py's CPU run reaches it in V).  The gripper touches down for two steps of ten: kept pressed, the oracle's own one-ulp twin
         leaves it by more than 1e-3 in the arm joints in 5 % of the env-steps under these frictions (param_scenarios.V_PRESS), and the bound below is 1 %.
    A second handle under debug flag 1 (super_solve instead of the four-env path) runs beside the first and must stay bit-identical to it: the three places where k_solve2
    rebuilds the motor rows from the env's gain and strength - solve4_body, heavy_solve, super_solve - are then all held to the oracle.
    Assertions: test_distribution_a_lockstep_with_contact_history's, unchanged in form; the twins carry the same parameters, so every margin is over the reference alone.
    The share of env-steps with the same manifolds / points / GJK pairs is held to the one-ulp CPU twin's own share minus 0.03 (TWIN_SAME, measured in
    tests/test_oracle_params.py's free run: U 1.0000, P 0.9952, V 0.9891), at most dist_a's 0.97."""
    from gpu_debug import oracle_state_from_record
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    n, steps = ps.N_ENVS, ps.STEPS
    env = VecPlayEnv(ps.IDS[kind], n, seed=ps.SEED)
    env.set_groups(3)
    tabs, fresh, mask = ps.draws(kind, n, 0), ps.draws(kind, n, 1), ps.redraw_mask(n)
    # a second handle under debug flag 1: its envs without spanning contacts take super_solve - the third place where k_solve2 rebuilds the motor rows - instead of the
    # four-env path; same tables, states and actions, and its records must be the first handle's bit for bit, which holds super_solve to the oracle through them
    sup = VecPlayEnv(ps.IDS[kind], n, seed=ps.SEED)
    sup.set_groups(3)
    sup.set_debug_flags(1)
    for h in (env, sup):
        _write_tables(h, tabs)
        h.reset()
    if kind == 'U':
        pos, quat = ps.scatter_poses(kind, n)
        st = env.get_state().cpu().numpy()
        st[:, 24:27], st[:, 27:31], st[:, 31:37] = pos, quat, 0.0
        st[:, REC:] = 0.0
        for h in (env, sup):
            h.set_state(torch.tensor(st))
    assert torch.equal(env.get_state().view(torch.int32), sup.get_state().view(torch.int32))
    obs = env.calc_state()
    script = ps.Script(kind, n, steps)
    trio = [[OracleEnv(kind, seed=ps.SEED, env_index=e, f32=True) for e in range(n)] for _ in range(3)]      # the oracle, its one-ulp twin, its 1e-5 twin
    for group in trio:
        for o in group:
            o.reset()
    ora = trio[0]
    nm, na = N_MAIN[kind], ora[0].n_arm
    shape = (steps, n)
    d_arm, d_pos, d_free, gap = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.full(shape, np.nan)
    t_pos, t_free, t5_free, t_gap = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.full(shape, np.nan)
    same, t_same, skipped = np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    tors, rows = np.zeros(shape, int), np.zeros(shape + (4,), int)
    pre = env.get_state().cpu().numpy()
    pool = ThreadPoolExecutor(16)
    for t in range(steps):
        if t == ps.REDRAW_AT:          # fresh rows of every table for half the envs, through the masked setters: cached manifold points meet another mu and another mass
            _write_tables(env, fresh, mask)
            _write_tables(sup, fresh, mask)
        dev = _device_tables(env)
        if t in (0, ps.REDRAW_AT):      # (the rows came back as written, and only where the mask said)
            want = {k: np.where(mask.reshape((n,) + (1,) * (v.ndim - 1)), fresh[k], v) if t else v for k, v in tabs.items()}
            assert all(np.array_equal(dev[k], want[k]) for k in TABLES)
        blk = obs['achieved_goal'][:, :3].cpu().numpy()
        acts = script.action(t, blk).astype(np.float32)
        obs, r, done, info = env.step(torch.tensor(acts))
        sup.step(torch.tensor(acts))
        differ = (env.get_state().view(torch.int32) != sup.get_state().view(torch.int32)).any(dim=1)
        assert not bool(differ.any()), 'step %d: the four-env path and super_solve differ in envs %s' % (t, torch.nonzero(differ).flatten().tolist())
        post = env.get_state().cpu().numpy()
        rows[t] = env.debug_row_counts().numpy()
        tp_dev = info['target_poses'].cpu().numpy().astype(np.float64)
        skipped[t] = (info['status'].cpu().numpy() & 3) != 0

        def one(e):
            a = acts[e].astype(np.float64)
            outs = []
            for o, rel in zip((trio[0][e], trio[1][e], trio[2][e]), (None, 0.0, 1e-5)):
                s = oracle_state_from_record(o, pre[e])
                if rel is not None:
                    q = s[:na].astype(np.float32)
                    s[:na] = (np.nextafter(q, np.float32(np.inf)) if rel == 0.0 else (q * np.float32(1.0 + rel) + np.float32(rel))).astype(np.float64)
                ps.apply_row(o, dev, e)
                o.set_state(s)
                o.set_cache_row(pre[e, REC:])
                o.perform_action(a)                                  # (every motor re-commanded from the same state, as the device's action stage does) ...
                o.goto_joint_poses(tp_dev[e], gripper=float(a[-1]))      # ... then the device's joint targets for the 12 substeps
                o.run_simulation()
                outs.append((o.get_state(), o.get_cache_row()))
            return outs, trio[0][e].lib.rpo_last_num_tors(trio[0][e].h)
        for e, (((so, ro), (sw, rw), (sw5, _)), nt) in enumerate(pool.map(one, range(n))):
            o = ora[e]
            sd, rd = oracle_state_from_record(o, post[e]), post[e, REC:]
            tors[t, e] = nt
            d_arm[t, e] = float((np.abs(sd[:na] - so[:na]) / np.maximum(1.0, np.abs(so[:na])))[:nm].max())
            d_pos[t, e], t_pos[t, e] = float(np.abs(positions(o, sd) - positions(o, so)).max()), float(np.abs(positions(o, sw) - positions(o, so)).max())
            d_free[t, e] = float(np.abs(free_positions(o, sd) - free_positions(o, so)).max())
            t_free[t, e] = float(np.abs(free_positions(o, sw) - free_positions(o, so)).max())
            t5_free[t, e] = float(np.abs(free_positions(o, sw5) - free_positions(o, so)).max())
            same[t, e] = cache_rows.manifolds(rd) == cache_rows.manifolds(ro) and cache_rows.gjk_tags(rd) == cache_rows.gjk_tags(ro)
            t_same[t, e] = cache_rows.manifolds(rw) == cache_rows.manifolds(ro) and cache_rows.gjk_tags(rw) == cache_rows.gjk_tags(ro)
            if cache_rows.integers(rd) == cache_rows.integers(ro):
                gap[t, e] = cache_rows.float_gap(rd, ro)
            if cache_rows.integers(rw) == cache_rows.integers(ro):
                t_gap[t, e] = cache_rows.float_gap(rw, ro)
        pre = post
    pool.shutdown()
    ok = ~skipped
    tot = int(ok.sum())
    span, arm = rows[..., 3] > 0, rows[..., 2] > 0
    cover = dict(spanning=int((span & ok).sum()), arm=int((arm & ~span & ok).sum()), light=int((~arm & ~span & ok).sum()), torsional=int(((tors > 0) & ok).sum()),
                 big=int(((rows[..., 1] >= 15) & ok).sum()))
    f_dev, f_tw, f5_tw = float((d_free[ok] > 1e-4).mean()), float((t_free[ok] > 1e-4).mean()), float((t5_free[ok] > 1e-4).mean())
    f3_dev, f3_tw, f53_tw = float((d_free[ok] > 1e-3).mean()), float((t_free[ok] > 1e-3).mean()), float((t5_free[ok] > 1e-3).mean())
    a_dev, a_tw = float((d_pos[ok] > 1e-4).mean()), float((t_pos[ok] > 1e-4).mean())
    g_dev = float(np.nanmax(gap[ok])) if np.isfinite(gap[ok]).any() else 0.0
    g_tw = float(np.nanmax(t_gap[ok])) if np.isfinite(t_gap[ok]).any() else 0.0
    held = int((obs['achieved_goal'][:, 2] > 0.05).sum()) if kind == 'P' else -1
    print('%s parameter lock-step, %d envs x %d steps, %d env-steps compared (%.3f); env-steps with spanning contacts %d, arm contacts only %d, neither %d, torsional rows %d, '
          '15 or more contacts %d%s' % (kind, n, steps, tot, tot / (n * steps), cover['spanning'], cover['arm'], cover['light'], cover['torsional'], cover['big'],
                                       '; the block in the air at the end in %d envs' % held if kind == 'P' else ''))
    print('    free bodies + scene joints, device vs oracle beyond 1e-4 in %.2f %%, beyond 1e-3 in %.2f %% (max %.1e); one-ulp twin %.2f %% / %.2f %%; 1e-5 twin %.2f %% / %.2f %%; '
          'all positions beyond 1e-4: device %.2f %%, twin %.2f %%; cached-point gap: device max %.1e, twin max %.1e; arm joints: median %.1e, beyond 1e-3 in %.2f %%; '
          'same manifolds / points / GJK pairs: device %.2f %%, twin %.2f %%'
          % (100 * f_dev, 100 * f3_dev, float(d_free[ok].max()), 100 * f_tw, 100 * f3_tw, 100 * f5_tw, 100 * f53_tw, 100 * a_dev, 100 * a_tw, g_dev, g_tw,
             float(np.median(d_arm[ok])), 100 * float((d_arm[ok] > 1e-3).mean()), 100 * float(same[ok].mean()), 100 * float(t_same[ok].mean())))
    env.close()
    sup.close()
    assert tot >= 0.9 * n * steps, tot
    if kind == 'U':
        assert cover['light'] > 0, cover
    if kind == 'P':
        assert cover['spanning'] > 0 and cover['torsional'] > 0 and held >= 1, (cover, held)
    if kind == 'V':
        assert cover['arm'] > 0 and cover['torsional'] > 0 and cover['big'] > 0, cover
    assert f_dev <= 3.0 * max(f_tw, f5_tw) + 0.005, (f_dev, f_tw, f5_tw)
    assert f3_dev <= 3.0 * max(f3_tw, f53_tw) + 0.005, (f3_dev, f3_tw, f53_tw)
    assert a_dev <= 2.0 * a_tw + 0.01, (a_dev, a_tw)
    assert g_dev <= max(3.0 * g_tw, 1e-3), (g_dev, g_tw)
    assert np.median(d_arm[ok]) <= 1e-5, np.median(d_arm[ok])
    assert (d_arm[ok] > 1e-3).mean() <= 0.01, (d_arm[ok] > 1e-3).mean()
    assert same[ok].mean() >= min(TWIN_SAME[kind] - 0.03, 0.97), (same[ok].mean(), TWIN_SAME[kind])


def test_the_clamp_at_ten_on_the_device():
    """Three envs from one and the same state: the block thrown along the table at 2 m/s (tests/test_oracle_params.py's clamp scene), block frictions 24, 80 and 18 against the
    table's 0.5.  The products 12 and 40 are both 10 to the kernels: the two records are bit-identical after 10 steps; 9 is not 10: the third differs.  The oracle's
    contact list at a state on the way says the block - table pair was in contact, with the coefficient 10"""
    from gpu_debug import oracle_state_from_record
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    from test_gpu_dynamics import _park_arm
    env = VecPlayEnv('UR5Play1Obj-v0', 3, seed=2)
    hold = _park_arm(env, (0.15, 0.0, 0.25))
    names = env.dynamics_names['friction']
    fr = env.get_dynamics()['friction'].clone()
    assert float(fr[0, names.index('table')]) == 0.5
    fr[:, names.index('block')] = torch.tensor([24.0, 80.0, 18.0], device=env.device)
    env.set_dynamics(friction=fr)
    st = env.get_state().clone()
    st[1], st[2] = st[0], st[0]
    f0 = env.state_layout['free0'][0]
    st[:, f0:f0 + 13] = torch.tensor([-0.05, 0.25, 0.0, 0, 0, 0, 1.0, -2.0, 0, 0, 0, 0, 0], device=env.device)
    st[:, REC:] = 0.0
    env.set_state(st)
    hold[:] = hold[0].clone()
    mus, touched = set(), False
    o = OracleEnv('UR5Play1Obj-v0', seed=2, f32=True)
    o.reset()
    d = o.get_dynamics(); d['friction'] = fr[0].cpu().numpy().astype(np.float64)
    o.set_dynamics(**d)
    cols = o.collider_list()
    for t in range(10):
        env.step(hold)
        rec = env.get_state()
        if t < 3:
            o.set_state(oracle_state_from_record(o, rec[0].cpu().numpy()))
            o.set_cache_row(rec[0, REC:].cpu().numpy())
            con = o.contacts()
            pair = [i for i, c in enumerate(con) if cols[int(c[0])]['body'] == 1 + o.n_arm and cols[int(c[1])]['body'] == 0]
            touched |= len(pair) > 0
            mus |= set(o.contact_mu()[pair].tolist())
    assert touched and mus == {10.0}, (touched, mus)
    rec = env.get_state().view(torch.int32)
    assert torch.equal(rec[0], rec[1]), torch.nonzero(rec[0] != rec[1]).flatten().tolist()[:8]
    assert not torch.equal(rec[0], rec[2])
    env.close()
