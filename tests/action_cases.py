"""The action stage's cases, shared by tests/test_action_cases.py (CPU: the reference alone) and tests/test_gpu_action.py (the device against it).

One table per registered one-object play id (UR5: model U, chain 6, 4 x 20 IK iterations; Panda: model V, chain 7, 1 x 200; six action types each): about sixty cases
(kind, measured joints, action), built with numpy from a fixed seed.  The only thing taken from outside is the arm's forward kinematics (the fp64 CPU oracle's, to express
"the pose of joints x" in an id's action type); no file is read or written.  Every input is rounded to fp32 before anybody sees it; no action is non-finite.

kinds
    near / mid / wide   measured joints = rest +- 0.25 rad, the target is the pose (or the joint vector) of joints +- 0.05 / 0.5 / 1.5 rad from them; near cases keep
                        0.12 rad from the joint limits, so that neither clamp of goto_joint_poses acts and the clamped targets show the IK itself
    far                 U(action_space) pushed outwards: positions metres outside the workspace (the IK's last call must run out of iterations)
    clip                components exactly at action_space.high, one ulp inside it and well beyond it (6 for absolute_rpy's first six and absolute_joints' joints, else 1)
    orient              pose types: non-unit / all-zero / w < 0 quaternions, a target pi from the measured orientation, pitch at +- pi / 2, targets whose rotation matrix has
                        trace 0 (m3_to_quat's branch change), a relative_quat increment that nearly cancels the measured quaternion
    joint               measured joints within inc of a joint limit, inside and outside it, with actions that cross the limit, and joint actions exactly +- inc and
                        +- inc +- 1 ulp from the measured joint (the two clamps' order)
    grip                gripper commands -1, 0, 1 and beyond

reference(gid) runs the CPU oracles over a table once per process: fp64, fp32, and fp32 "followers" whose measured chain joints are 1 and 2 fp32 ulps up and down, and
classifies every case from them alone (exact / marginal / fuzzy / clean, see classify)."""
import functools

import numpy as np

SEED = 43                           # chosen so that the reference alone keeps the marginal share of every id at or below 8 %, no far case is fuzzy and every clean 99th percentile is below 1e-4
IDS = {'UR5PlayAbsRPY1Obj-v0': 'absolute_rpy', 'UR5PlayRelRPY1Obj-v0': 'relative_rpy', 'UR5Play1Obj-v0': 'absolute_quat', 'UR5PlayRel1Obj-v0': 'relative_quat',
       'UR5PlayAbsJoints1Obj-v0': 'absolute_joints', 'UR5PlayRelJoints1Obj-v0': 'relative_joints',
       'pandaPlayAbsRPY1Obj-v0': 'absolute_rpy', 'pandaPlayRelRPY1Obj-v0': 'relative_rpy', 'pandaPlay1Obj-v0': 'absolute_quat', 'pandaPlayRel1Obj-v0': 'relative_quat',
       'pandaPlayAbsJoints1Obj-v0': 'absolute_joints', 'pandaPlayRelJoints1Obj-v0': 'relative_joints'}
JOINT_TYPES = ('absolute_joints', 'relative_joints')
F32 = np.float32
PI = np.pi
# goto_joint_poses' tables (environments.py:1014-1021), as fp32 holds them
LIMITS = {'ur5': (np.full(6, -2 * PI), np.array([-0.7, 2 * PI, -0.5, 2 * PI, 2 * PI, 2 * PI]), np.array([0.1, 0.1, 0.2, 0.2, 0.2, 0.2])),
          'panda': (np.array([-0.6, -2.2, -3.0, -3.04878596, -PI, -PI, -PI]), np.array([3, 1.8, 0.5, -0.5002492, 3., 3.45266257, 2.40072908]),
                    np.array([0.1, 0.1, 0.2, 0.2, 0.2, 0.2, 0.2]))}
LIMITS = {k: tuple(x.astype(F32) for x in v) for k, v in LIMITS.items()}
NUDGES = (0, 1, -1, 2, -2)          # the fp32 followers' measured joints, in fp32 ulps from the case's
MARGINAL_CAP = 0.10                 # share of an id's cases
FUZZY_CAP = 0.10                    # share of an id's far cases, and of its other cases
FUZZY_GAP = 1e-3


def arm_of(gid):
    return 'panda' if gid.startswith('panda') else 'ur5'


def action_high(gid):
    """action_space.high (environments.py:88-113)"""
    at, nd = IDS[gid], 7 if arm_of(gid) == 'panda' else 6
    if at == 'absolute_rpy':
        return np.array([6] * 6 + [1], dtype=F32)
    if at == 'absolute_joints':
        return np.array([6] * nd + [1], dtype=F32)
    return np.ones({'relative_rpy': 7, 'absolute_quat': 8, 'relative_quat': 8, 'relative_joints': nd + 1}[at], dtype=F32)


def clip_action(gid, a):
    """step()'s np.clip, in fp32"""
    hi = action_high(gid)
    return np.clip(np.asarray(a, dtype=F32), -hi, hi)


def ulps(x, k):
    """x (fp32) moved k ulps"""
    x = np.asarray(x, dtype=F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def goto_clamps(gid, raw, q):
    """goto_joint_poses' two np.clip calls on fp32 values: the joint limits first, then q +- inc"""
    ll, ul, inc = LIMITS[arm_of(gid)]
    raw, q = np.asarray(raw, dtype=F32), np.asarray(q, dtype=F32)
    t = np.minimum(np.maximum(raw, ll), ul)
    return np.minimum(np.maximum(t, q - inc), q + inc)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


class _Arm:
    """forward kinematics of an id's arm: the fp64 oracle's EE link pose at given joints"""

    def __init__(self, gid):
        import oracle
        self.o = oracle.OracleEnv(gid)
        self.o.reset()
        self.oracle = oracle
        self.rest = self.o.rest_pose()

    def pose(self, q_full):
        self.o.set_arm_q(np.asarray(q_full, dtype=np.float64))
        p, q, _, _ = self.o.site_pose(0)
        return p.copy(), q.copy()

    def euler(self, quat):
        return self.oracle.euler_from_quat(quat)

    def quat(self, rpy):
        return self.oracle.quat_from_euler(rpy)


@functools.lru_cache(maxsize=None)
def build(gid):
    """{'kinds': [n] str, 'q': [n, n_arm] fp32 measured joints (the gripper's included), 'a': [n, n_action] fp32 actions, unclipped, 'trace0': {case: the trace of
    its target rotation} for the orient cases built to sit at trace 0}"""
    at, arm = IDS[gid], arm_of(gid)
    fk = _Arm(gid)
    n_arm, nd = fk.o.n_arm, fk.o.n_target
    na = fk.o.n_action
    ll, ul, inc = (x.astype(np.float64) for x in LIMITS[arm])
    rng = np.random.default_rng(SEED + 100 * sorted(IDS).index(gid))
    rest = fk.rest[:nd]
    kinds, Q, A, trace = [], [], [], {}

    def full(qc):
        """measured joints of the whole arm: the chain's, and the gripper's a little off zero (the Robotiq's 'left' target is its measured driver joint)"""
        q = np.zeros(n_arm)
        q[:nd] = qc
        q[nd:] = 0.02 * rng.random(n_arm - nd)
        return q.astype(F32)

    def grip():
        return 2 * rng.random() - 1

    def express(q, pos_t, quat_t, qt, g):
        """the action of this id's type that asks for pose (pos_t, quat_t) = the pose of chain joints qt, from measured joints q"""
        a = np.zeros(na)
        a[-1] = g
        if at in JOINT_TYPES:
            a[:nd] = qt - q[:nd].astype(np.float64) if at == 'relative_joints' else qt
            return a
        pc, qc = fk.pose(q)
        if at == 'absolute_rpy':
            a[0:3], a[3:6] = pos_t, fk.euler(quat_t)
        elif at == 'relative_rpy':
            a[0:3], a[3:6] = pos_t - pc, fk.euler(quat_t) - fk.euler(qc)
        elif at == 'absolute_quat':
            a[0:3], a[3:7] = pos_t, quat_t
        else:
            a[0:3], a[3:7] = pos_t - pc, (quat_t if np.dot(quat_t, qc) >= 0 else -quat_t) - qc
        return a

    def add(kind, q, a):
        kinds.append(kind); Q.append(np.asarray(q, dtype=F32)); A.append(np.asarray(a, dtype=F32))
        assert np.isfinite(A[-1]).all() and np.isfinite(Q[-1]).all()

    def pose_of(q, qt):
        qq = np.array(q, dtype=np.float64)
        qq[:nd] = qt
        return fk.pose(qq)

    def reach_case(kind, d, keep_off_limits):
        qc = rest + rng.uniform(-0.25, 0.25, nd)
        if keep_off_limits:
            qc = np.clip(qc, ll + 0.12, ul - 0.12)
        q = full(qc)
        qt = q[:nd].astype(np.float64) + rng.uniform(-d, d, nd)
        add(kind, q, express(q, *pose_of(q, qt), qt, grip()))
        return q, qt

    # near / mid / wide
    for kind, d, n in (('near', 0.05, 10), ('mid', 0.5, 9), ('wide', 1.5, 9)):
        for _ in range(n):
            reach_case(kind, d, kind == 'near')
    # far: U(action_space), its position (joint types: every joint) pushed to the outer part of the box
    hi = action_high(gid).astype(np.float64)
    for _ in range(8):
        q = full(rest + rng.uniform(-0.25, 0.25, nd))
        a = rng.uniform(-hi, hi)
        if at not in JOINT_TYPES:
            sgn = rng.choice([-1.0, 1.0], 3)
            if at in ('relative_rpy', 'relative_quat'):      # away from the base, whatever the measured pose
                pc, _ = fk.pose(q)
                sgn = np.where(pc >= 0, 1.0, -1.0)
            a[0:3] = sgn * hi[0:3] * rng.uniform(0.8, 1.0, 3)
        add('far', q, a)
    # clip edges, on reachable targets: at the bound, one ulp inside, beyond (the same as at the bound, after the clip), everything beyond
    hi32 = action_high(gid)
    inside = np.nextafter(hi32, F32(0))
    q, qt = reach_case('clip', 0.05, True)
    base_a = A[-1].copy()
    i0, i1 = (3, 5) if at not in JOINT_TYPES else (1, nd - 1)
    for k, (v0, v1) in enumerate(((hi32[i0], -hi32[i1]), (inside[i0], -inside[i1]), (3 * hi32[i0], -7 * hi32[i1]))):
        a = base_a.copy()
        a[i0], a[i1] = v0, v1
        a[-1] = (1.0, float(inside[-1]), 3.0)[k]
        add('clip', q, a)
    add('clip', q, np.where(rng.random(na) < 0.5, -10.0, 10.0) * hi)
    if at not in JOINT_TYPES:
        # orientation edges
        def q_near():
            return full(np.clip(rest + rng.uniform(-0.25, 0.25, nd), ll + 0.12, ul - 0.12))

        def near_target(q):
            qt = q[:nd].astype(np.float64) + 0.05 * rng.choice([-1.0, 1.0], nd) * rng.uniform(0.5, 1.0, nd)
            return pose_of(q, qt) + (qt,)

        def trace0(q):
            """joints close to q whose EE rotation has trace 0 (angle 120 deg): scan a wrist joint for a sign change of the trace, then bisect"""
            for j in range(nd - 1, nd - 5, -1):
                def tr(x):
                    qt = q[:nd].astype(np.float64); qt[j] = x
                    w = pose_of(q, qt)[1][3]
                    return 4 * w * w - 1           # trace of the rotation of a unit quaternion
                xs = q[j] + np.linspace(-1.5, 1.5, 61)
                v = [tr(x) for x in xs]
                for i in range(60):
                    if v[i] * v[i + 1] < 0:
                        lo, hi_ = xs[i], xs[i + 1]
                        for _ in range(60):
                            mid = 0.5 * (lo + hi_)
                            if tr(lo) * tr(mid) <= 0:
                                hi_ = mid
                            else:
                                lo = mid
                        qt = q[:nd].astype(np.float64); qt[j] = lo
                        return qt
            raise AssertionError('no trace-0 pose within 1.5 rad of %s' % (q[:nd],))

        for _ in range(2):                       # m3_to_quat's branch change at the target
            q = q_near()
            qt = trace0(q)
            pt, qq = pose_of(q, qt)
            add('orient', q, express(q, pt, qq, qt, grip()))
            trace[len(kinds) - 1] = 4 * qq[3] * qq[3] - 1
        for sgn in (1.0, -1.0):                  # a target pi from the measured orientation, about a random axis
            q = q_near()
            pc, qc = fk.pose(q)
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            qq = _qmul(qc, np.array([ax[0], ax[1], ax[2], 0.0])) * sgn
            a = express(q, pc, qq, None, grip())
            if at == 'relative_quat':
                a[3:7] = qq - qc                 # (as given: express would pick the nearer sign)
            add('orient', q, a)
        if at in ('absolute_rpy', 'relative_rpy'):
            for pitch in (PI / 2, -PI / 2, float(F32(PI / 2)), -1.5707):       # euler_from_quat's clamp, quat_from_euler at the pole
                q = q_near()
                pt, qq, qt = near_target(q)
                e = fk.euler(qq); e[1] = pitch
                a = express(q, pt, fk.quat(e), qt, grip())
                if at == 'absolute_rpy':
                    a[3:6] = e
                else:
                    a[3:6] = e - fk.euler(fk.pose(q)[1])
                add('orient', q, a)
        else:
            q = q_near()
            pt, qq, qt = near_target(q)
            pc, qc = fk.pose(q)
            a = express(q, pt, qq, qt, grip())
            if at == 'absolute_quat':
                for qv in (2 * qq, np.zeros(4), -qq if qq[3] > 0 else qq, np.array([1.0, 1.0, 1.0, 1.0]), 0.5 * qq):      # norm 2 clips componentwise; zero; w < 0; norm 2; norm 1/2
                    b = a.copy(); b[3:7] = qv
                    add('orient', q, b)
            else:
                for qv in (-qc, -qc * (1 - 1e-3), qq - qc + qq, -2 * qc, np.array([1.0, 1.0, 1.0, 1.0])):                 # cancels, nearly cancels, norm 2, flips, clips to norm ~2
                    b = a.copy(); b[3:7] = qv
                    add('orient', q, b)
    # joint edges: measured joints within inc of a limit, inside and outside, the action across it / away from it
    lims = [(0, ul[0]), (2, ul[2])] if arm == 'ur5' else [(0, ll[0]), (3, ul[3])]
    for j, lim in lims:
        up = lim == ul[j]
        out = 1.0 if up else -1.0
        for off in (-0.5 * inc[j], 0.5 * inc[j], 1.5 * inc[j]):      # inside by inc / 2, outside by inc / 2 and by 3 inc / 2 (the clamps then disagree: q +- inc wins)
            qc = np.clip(rest + rng.uniform(-0.25, 0.25, nd), ll + 0.12, ul - 0.12)
            qc[j] = lim + out * off
            q = full(qc)
            qt = q[:nd].astype(np.float64) + 0.05 * rng.choice([-1.0, 1.0], nd) * rng.uniform(0.5, 1.0, nd)
            qt[j] = q[j] + out * (0.08 if off < 0 else -0.08) * inc[j] / 0.1      # across the limit from inside, back towards it from outside
            add('joint', q, express(q, *pose_of(q, qt), qt, grip()))
    if at in JOINT_TYPES:
        inc32 = LIMITS[arm][2]
        for k in (0, 1, -1):                      # exactly q +- inc and an ulp either side, as fp32 computes q +- inc
            for sgn in (1, -1):
                q = full(np.clip(rest + rng.uniform(-0.25, 0.25, nd), ll + 0.25, ul - 0.25))
                if at == 'absolute_joints':
                    t = ulps(q[:nd] + F32(sgn) * inc32, k)
                else:
                    t = ulps(F32(sgn) * inc32, k)
                a = np.zeros(na); a[:nd] = t; a[-1] = grip()
                add('joint', q, a)
        for sgn in (1.0, -1.0):                   # every joint far across its limits
            q = full(rest + rng.uniform(-0.25, 0.25, nd))
            a = np.zeros(na); a[-1] = grip()
            a[:nd] = (sgn if at == 'relative_joints' else sgn * 6.0) * np.ones(nd)
            add('joint', q, a)
    # gripper
    for g in (-1.0, 0.0, 1.0, -0.0, 2.5, -7.0, float(np.nextafter(F32(1), F32(2))), 0.2):
        q, _ = reach_case('grip', 0.05, True)
        A[-1][-1] = F32(g)
    out = {'kinds': tuple(kinds), 'q': np.stack(Q), 'a': np.stack(A), 'trace0': dict(trace)}
    assert out['a'].shape[1] == na and out['q'].shape[1] == n_arm and len(kinds) <= 64, (out['a'].shape, out['q'].shape)
    out['q'].setflags(write=False); out['a'].setflags(write=False)
    return out


def run_oracle(gid, q, a_clipped, f32):
    """one oracle over measured joints q [n, n_arm] and clipped actions [n, n_action]: {'raw' [n, nd] (before goto_joint_poses' clamps), 'tp' [n, nd] (after),
    'motor' [n, n_arm] (every motor target), 'passes', 'capped', 'window' [n], 'tp_of_raw' [n, nd]: rpo_goto_joint_poses on the raw solution}"""
    import oracle
    o = oracle.OracleEnv(gid, f32=f32)
    o.reset()
    res = {k: [] for k in ('raw', 'tp', 'motor', 'passes', 'capped', 'window', 'tp_of_raw')}
    for qi, ai in zip(q, a_clipped):
        o.set_arm_q(qi.astype(np.float64))
        raw, rep = o.perform_action_raw(ai.astype(np.float64))
        o.set_arm_q(qi.astype(np.float64))
        tp = o.perform_action(ai.astype(np.float64))
        motor = o.get_motor()[1]
        o.set_arm_q(qi.astype(np.float64))
        res['tp_of_raw'].append(o.goto_joint_poses(raw))
        res['raw'].append(raw); res['tp'].append(tp); res['motor'].append(motor.copy())
        res['passes'].append(rep['passes']); res['capped'].append(rep['capped']); res['window'].append(rep['window'])
    return {k: np.array(v) for k, v in res.items()}


def classify(gid, kinds, ref64, followers):
    """per case 'exact' (the joint action types: an add and two clamps), 'fuzzy' (the followers are more than FUZZY_GAP from fp64: the reference itself does not know
    the answer), 'marginal' (a follower's stopping test fell in the device's window of 0.5 % around the residual threshold, or the followers took different numbers of
    loop passes), 'clean'.

    Fuzzy is looked at first and on every kind, not on far cases alone: a target exactly pi from the measured orientation (the sign of the pose error's angle is a
    rounding matter) or a wide one that the iteration budget does not reach leaves fp32 and fp64 radians apart just as a far one can, and such a case among the clean
    ones would put its radians into the id's clean percentile - the floor of the device's bound.  A fuzzy case is held to three times its followers' gap and nothing
    else, which is never more than a clean or marginal case gets; the far cases keep their own cap (FUZZY_CAP), the others get the same share of theirs."""
    n = len(kinds)
    gap = np.max([np.abs(f['raw'] - ref64['raw']) for f in followers], axis=0)      # [n, nd]
    cls = []
    for i in range(n):
        if IDS[gid] in JOINT_TYPES:
            cls.append('exact')
        elif gap[i].max() > FUZZY_GAP:
            cls.append('fuzzy')
        elif any(f['window'][i] for f in followers) or len({int(f['passes'][i]) for f in followers}) > 1:
            cls.append('marginal')
        else:
            cls.append('clean')
    return cls, gap


@functools.lru_cache(maxsize=None)
def reference(gid):
    """the CPU oracles' account of build(gid): {'cases', 'clipped' actions, 'f64', 'f32' (run_oracle), 'followers' (fp32, measured chain joints NUDGES ulps off; the
    first is 'f32'), 'cls' per case, 'gap' [n, nd]: the followers' largest distance from fp64 in the raw solution}"""
    c = build(gid)
    nd = 7 if arm_of(gid) == 'panda' else 6
    ac = clip_action(gid, c['a'])
    f64 = run_oracle(gid, c['q'], ac, False)
    fol = []
    for k in NUDGES:
        q = c['q'].copy()
        q[:, :nd] = ulps(q[:, :nd], k)
        fol.append(run_oracle(gid, q, ac, True))
    cls, gap = classify(gid, c['kinds'], f64, fol)
    return {'cases': c, 'clipped': ac, 'f64': f64, 'f32': fol[0], 'followers': fol, 'cls': cls, 'gap': gap}


GAPS_FILE = 'profiles/action_stage_cpu_gaps.txt'
GAPS_COLUMNS = ('cases', 'clean', 'marginal', 'fuzzy', 'clean_median', 'clean_p99', 'clean_max', 'marginal_max')


def gap_row(gid):
    """the id's line of GAPS_FILE: counts per class, then |fp32 oracle - fp64 oracle| of the raw solution (per case: its largest joint) over the clean cases (median, 99th
    percentile, maximum) and the followers' largest gap over the marginal ones"""
    r = reference(gid)
    cls = np.array(r['cls'])
    g32 = np.abs(r['f32']['raw'] - r['f64']['raw']).max(axis=1)
    clean = g32[cls == 'clean']
    marg = r['gap'].max(axis=1)[cls == 'marginal']
    z = lambda x, f: float(f(x)) if len(x) else 0.0
    return (len(cls), int((cls == 'clean').sum()), int((cls == 'marginal').sum()), int((cls == 'fuzzy').sum()),
            z(clean, np.median), z(clean, lambda x: np.percentile(x, 99)), z(clean, np.max), z(marg, np.max))


def format_gaps(rows):
    """GAPS_FILE's text from {gid: gap_row}"""
    lines = ['# the CPU oracles on tests/action_cases.py: fp32 against fp64, raw (unclamped) joint solution of the action stage, rad.  Held to a fresh run by tests/test_action_cases.py (RP_WRITE_ACTION_GAPS=1 rewrites it);',
             '# tests/test_gpu_action.py takes its bounds from here (4 x clean_p99 per id; 3 x marginal_max).',
             '# %-28s %s' % ('id', ' '.join('%12s' % c for c in GAPS_COLUMNS))]
    for gid in IDS:
        r = rows[gid]
        lines.append('%-30s %s' % (gid, ' '.join(['%12d' % v for v in r[:4]] + ['%12.3e' % v for v in r[4:]])))
    return '\n'.join(lines) + '\n'


def parse_gaps(text):
    """{gid: {column: value}} of GAPS_FILE's text"""
    out = {}
    for line in text.splitlines():
        if line.startswith('#') or not line.strip():
            continue
        f = line.split()
        out[f[0]] = dict(zip(GAPS_COLUMNS, [float(x) for x in f[1:]]))
    return out
