"""Seeded crowded scenes for the narrowphase's shared caps (tests/test_contact_caps.py, tests/test_gpu_contact_caps.py).

Every substep the narrowphase keeps its work in fixed-size arrays, on the device (rp_kernels.cuh) and in the CPU oracle (rp_oracle.c collide_persistent)
alike, and both cut at the same caps in the same order:
    pairs       MAXACT / MAX_ACTIVE_PAIRS    AABB-overlapping pairs examined, in pair order
    candidates  CANDMAX / MAX_CANDIDATES     candidate points, pairs in order
    manifolds   PM_MAX                       cached manifolds: an object pair beyond them gets no slot
    contacts    MAXC / MAX_CONTACTS          contacts passed to the solver, in the four-tier order
    torsional   MAXT / MAX_TORS              spinning-friction rows
Rollout poses never reach most of them.  A crowded scene does: the arm near its rest posture, each free body at a face of a random collider (arm links
included, and preferred: that is where pairs pile up) with a gap in [-4, +4] mm along the face's normal, the scene joints anywhere in their ranges.
Scenes whose deepest contact lies beyond 6 mm are set apart (`deep`): there overlapping Panda cores meet a rounding-decided EPA face choice.

A scene is the oracle's state vector; the caps it crosses come from the fp32 oracle's counters (OracleEnv.collide_counts) on a history-free substep.
The contact-fuzz scenes (tools/contact_fuzz.py) are the same construction with one block at any collider and the arm within 0.35 rad: `fuzz=True`."""
import numpy as np

IDS = {'U': 'UR5PlayAbsRPY1Obj-v0', 'V': 'pandaPlayAbsRPY1Obj-v0', 'P': 'pandaPick-v0', 'W': 'pandaPlay-v0'}
CAPS = {'pairs': 64, 'candidates': 64, 'manifolds': 11, 'contacts': 21, 'torsional': 4}      # pinned against both sources by test_contact_caps.py
DEEP = 0.006


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _quat(R):
    """[x, y, z, w] of a rotation matrix"""
    w = 0.5 * np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2]))
    if w > 0.1:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        r = np.sqrt(max(1e-12, 1 + R[i, i] - R[j, j] - R[k, k]))
        q = np.zeros(4)
        q[i] = 0.5 * r
        q[j] = (R[j, i] + R[i, j]) / (2 * r)
        q[k] = (R[k, i] + R[i, k]) / (2 * r)
        q[3] = (R[k, j] - R[j, k]) / (2 * r)
    return q / np.linalg.norm(q)


def drawer_slot(kind, nf):
    """the free body that is the drawer (it keeps its rails), or -1"""
    return {'U': 1, 'V': 1, 'W': 2}.get(kind, -1) if nf > 1 else -1


def _deepest(o, s, bodies):
    """the deepest contact of the state s that touches one of `bodies` (0.0 without one); the cache is left empty"""
    o.set_state(s)
    oc = o.contacts()
    o.set_state(s)
    if not len(oc):
        return 0.0
    cols = o.collider_list()
    hit = [float(r[8]) for r in oc if cols[int(r[0])]['body'] in bodies or cols[int(r[1])]['body'] in bodies]
    return -min(hit, default=0.0)


def _scene(o, kind, s0, arm, rng, t, fuzz, tries):
    """one scene.  Unless fuzz: the arm and scene-joint posture is drawn again (up to `tries` times) while the arm or a scene-joint body lies deeper than 6 mm
    in something, and each free body's placement while the body does (the free bodies not placed yet wait at their start poses)"""
    na = o.n_arm
    nf = (len(s0) - 2 * na) // 13
    nj = (len(s0) - 2 * na - 13 * nf) // 2
    rest = o.rest_pose() if not fuzz else s0[:na]
    spread = 0.35 if fuzz else 0.6
    o.set_state(s0)
    cols = o.collider_list()
    nbody = 1 + max(c['body'] for c in cols)
    fixed = set(range(1, na + 1)) | set(range(1 + na + nf, nbody))      # arm links, scene-joint bodies
    for _ in range(1 if fuzz else tries):
        s = s0.copy()
        if not fuzz or t % 3:
            for i in range(na):
                lo, hi = arm[i][1], arm[i][2]
                v = rest[i] + rng.uniform(-spread, spread)
                s[i] = min(max(v, lo), hi) if lo < hi else v
        for k in range(nj):                              # the scene joints anywhere in their ranges (the button's travel: 3 cm)
            s[2 * na + 13 * nf + k] = rng.uniform(-1.5, 0.3) if k != 1 else rng.uniform(0.0, 0.03)
        s[na:2 * na] = 0.0
        if fuzz or _deepest(o, s, fixed) <= DEEP:
            break
    o.set_state(s)
    cols = o.collider_list()
    arm_cols = [c for c in cols if 1 <= c['body'] <= na]
    drawer = drawer_slot(kind, nf)
    for k in range(nf):
        base = 2 * na + 13 * k
        if k == drawer:
            s[base + 1] = s0[base + 1] + rng.uniform(-0.06, 0.075)
            continue
        own = [c for c in cols if c['body'] == 1 + na + k]
        hb = np.array(own[0]['he'], dtype=np.float64) if own else np.full(3, 0.025)
        for _ in range(1 if fuzz else tries):
            pool = arm_cols if (not fuzz and arm_cols and rng.random() < 0.6) else [c for c in cols if c['body'] != 1 + na + k]
            c = pool[rng.integers(len(pool))]
            if not fuzz and c['body'] > na and rng.random() < 0.5:      # face to face with a movable box (a box pair's four-point manifold).  Not with an arm
                # link: a hull face parallel to the block's ties its vertices, and rounding picks the point
                Rb = c['R'].copy()
                q = _quat(Rb)
            else:
                q = rng.normal(size=4) if t % 4 else np.array([0.0, 0.0, 0.0, 1.0])
                q /= np.linalg.norm(q)
                Rb = _rot(q)
            ax, sg = rng.integers(3), rng.choice([-1.0, 1.0])      # beside one of the collider's six faces (or over an edge), the gap in [-4, +4] mm along its normal
            nrm = c['R'][:, ax] * sg
            ext = float(np.abs(Rb.T @ nrm) @ hb)
            loc = (2 * rng.random(3) - 1) * (np.minimum(c['he'], 0.3) + 0.02)
            loc[ax] = sg * (c['he'][ax] + ext + rng.uniform(-0.004, 0.004))
            s[base:base + 3] = c['p'] + c['R'] @ loc
            s[base + 3:base + 7] = q
            s[base + 7:base + 13] = 0.0
            if fuzz or _deepest(o, s, {1 + na + k}) <= DEEP:
                break
    o.set_state(s)
    return s


def generate(kind, n, seed=0, fuzz=False, tries=12):
    """n scenes of `kind` (U, V, P, W), seeded: a list of dict(state, contacts [k, 9] of the fp32 oracle, counts (collide_counts), crossed (names of the caps
    the scene crosses), deep (its deepest contact beyond 6 mm)).  Every state is history-free: the oracle's cache is empty before and after."""
    from oracle import OracleEnv
    o = OracleEnv(IDS[kind], seed=7, env_index=0, f32=True)
    o.reset()
    s0 = o.get_state()
    arm = o.arm_table()
    rng = np.random.default_rng([seed, ord(kind), int(fuzz)])
    out = []
    for t in range(n):
        s = _scene(o, kind, s0, arm, rng, t, fuzz, tries)
        oc = o.contacts()
        counts = o.collide_counts()
        o.set_state(s)                                   # (contacts() advanced the cache: empty it again)
        deep = bool(len(oc) and float(oc[:, 8].min()) < -DEEP)
        out.append(dict(state=s, contacts=oc, counts=counts, deep=deep, crossed=frozenset(k for k, cap in CAPS.items() if counts[k] > cap)))
    return out


def coverage(scenes):
    """{cap: number of (shallow) scenes that cross it}"""
    return {k: sum(k in sc['crossed'] for sc in scenes if not sc['deep']) for k in CAPS}


def hold_action(o):
    """an absolute-RPY action that holds the arm's current end-effector pose (the gripper half open)"""
    from oracle import euler_from_quat
    p, q, _, _ = o.site_pose(0)
    return np.concatenate([p, euler_from_quat(q), [0.0]])
