"""Deterministic poses for the contact truth (tests/contact_truth.py): oracle states built from the model's own geometry (collider list, hull vertices, forward
kinematics) with a seeded generator, set by set_state and therefore without history on both sides.  Every pose is one env's record (tools/gpu_debug.record_from_oracle).

Families (the tag each pose carries; `poses(kind)` returns [(tag, state)] - 192 per id, which rp_step cuts into three env groups):
  flat        the block flat on the table top, with and without yaw, from 5 mm deep to 0.1 mm above (a box pair makes points only on overlap: its threshold is 0)
  edge45      the block on an edge, rolled by exactly 45 degrees (two incident faces tie)
  corner      the block on a corner, body diagonal vertical, and a little off it
  overhang    the block over the table's edges and corners with parallel edges
  crossed     an edge of the block across an edge of the table (the box detector's edge-edge branch)
  blocks      block against block, face to face, exactly aligned (two-block id only)
  link_face   a face of the block against the outermost vertex of a robot link's hull - arm links, fingers, the static base - at the pair's threshold -+ 1e-4 and
              pushed in by 1, 5 and 20 mm (vertex over a face; hull_face)
  link_rim    the same with the vertex within -+ 1e-4 of the face's boundary: the hand-over between vertex contacts and GJK
  link_edge   an edge / a corner of the block toward the link: GJK beside the faces, EPA where the cores overlap (1, 5, 20 mm)
  grasp       the block between the fingers, finger joints swept
  sphere      the block against the sphere collider, where the id has one: face, edge, corner, centre inside
  arm_table   the arm itself turned from its start pose along a random joint direction until a hull vertex is a given depth below the table top / behind the nearest
              static wall (bisection on forward kinematics): threshold -+ 1e-4, 1, 5 and 20 mm
"""
import ctypes as C

import numpy as np

N_POSES = 192
SEED = 20240607
KINDS = {'U': 'UR5PlayAbsRPY1Obj-v0', 'P': 'pandaPick-v0', 'V': 'pandaPlayAbsRPY1Obj-v0', 'W': 'pandaPlay-v0'}

# The fp32 oracle's worst gap per check on these poses (metres), asserted by tests/test_contact_truth.py against its own run (at most these, and no less than a
# quarter of them: the block follows the measurement).  The device's bounds are max(3 x these, 2e-6) - tests/test_gpu_contact_truth.py.
FP32_WORST = {
    'U': {'C1': 1.7e-07, 'C2': 1.2e-07, 'C3': 1.8e-07, 'C4': 0.0, 'P1': 8.8e-08, 'P2': 1.5e-07, 'P3': 0.0},
    'P': {'C1': 2.0e-07, 'C2': 8.7e-08, 'C3': 3.4e-07, 'C4': 0.0, 'P1': 2.8e-08, 'P2': 9.9e-08, 'P3': 0.0},
    'V': {'C1': 1.6e-07, 'C2': 1.2e-07, 'C3': 1.2e-07, 'C4': 0.0, 'P1': 3.6e-08, 'P2': 1.2e-07, 'P3': 0.0},
    'W': {'C1': 1.8e-07, 'C2': 5.9e-08, 'C3': 6.2e-08, 'C4': 0.0, 'P1': 4.0e-08, 'P2': 5.9e-08, 'P3': 0.0},
}


def contact_list(o, s):
    """history-free contact list of state s, with the EPA / GJK counters of that one collision phase and its cap counts"""
    se, sg = (C.c_long * 4)(), (C.c_long * 8)()
    o.lib.rpo_epa_stats.argtypes = [C.POINTER(C.c_long), C.c_int]
    o.set_state(s)
    o.lib.rpo_epa_stats(se, 1)
    o.lib.rpo_gjk_stats(sg, 1)
    oc = o.contacts()
    o.lib.rpo_epa_stats(se, 1)
    o.lib.rpo_gjk_stats(sg, 1)
    counts = o.collide_counts() if not o.bullet_ref else {}
    o.set_state(s)
    # a call has at least one round: with `calls` calls and `rounds` rounds no single call had 8 rounds (EPA_ITERS) unless rounds - (calls - 1) >= 8.  (The other caps
    # cannot come first: a closed triangulated polytope of V vertices has 2 V - 4 faces, and V <= 4 + 7 before the eighth round: 18 faces of 20, 11 vertices of 12)
    capped = se[0] > 0 and se[1] - (se[0] - 1) >= 8
    return oc, dict(epa_calls=se[0], epa_rounds=se[1], epa_gave_up=se[3], gjk_calls=sg[0], gjk_contacts=sg[3], capped=bool(capped)), counts


def epa_may_cap(oracles, s, n_arm, nudges=12, size=1e-7):
    """does an expanding-polytope call of this pose end at its round cap on any of `oracles` - at the pose or at one of `nudges` seeded nudges of `size` of the arm
    joints and the first free body's position?  Which tetrahedron GJK hands to EPA, and with it the number of rounds, turns on rounding-level differences of the
    inputs: on pandaPlayAbsRPY1Obj pose 99 the fp32 oracle needs 6 rounds and returns D* = -27.860 mm, and at 1e-7 nudges of the same pose 8 rounds and -27.839 mm
    (DESIGN.md section 2).  A device whose forward kinematics rounds differently is such a nudge."""
    rng = np.random.default_rng(SEED)
    calls = 0
    for k in range(nudges + 1):
        s2 = s.copy()
        if k:
            s2[:n_arm] += size * rng.normal(size=n_arm)
            s2[2 * n_arm:2 * n_arm + 3] += size * rng.normal(size=3)
        for o in oracles:
            st = contact_list(o, s2)[1]
            calls += st['epa_calls']
            if st['capped']:
                return True
        if not calls:
            return False                                     # (no EPA call at the pose itself: nothing to cap)
    return False


def _quat(R):
    """rotation matrix -> quaternion (x, y, z, w)"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[i] = 0.25 * s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
        q[3] = (R[k, j] - R[j, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def _rot(axis, ang):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _frame(x):
    """a right-handed frame whose first column is x"""
    x = x / np.linalg.norm(x)
    h = np.array([0.0, 0.0, 1.0]) if abs(x[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    y = np.cross(h, x)
    y /= np.linalg.norm(y)
    return np.stack([x, y, np.cross(x, y)], axis=1)


class _Builder:
    def __init__(self, o, kind):
        self.o, self.kind = o, kind
        self.na = o.n_arm
        self.s0 = o.get_state()
        self.s0[self.na:2 * self.na] = 0.0
        for k in range(o.n_free):
            self.s0[2 * self.na + 13 * k + 7:2 * self.na + 13 * k + 13] = 0.0
        nj = len(self.s0) - 2 * self.na - 13 * o.n_free
        if nj:
            self.s0[len(self.s0) - nj // 2:] = 0.0
        o.set_state(self.s0)
        self.cols = o.collider_list()
        self.hulls = {c: o.hull_vertices(c) for c in range(len(self.cols))}
        free_bodies = [self.na + 1 + k for k in range(o.n_free)]
        self.block_c = [[c for c, d in enumerate(self.cols) if d['body'] == fb] for fb in free_bodies]
        self.he = self.cols[self.block_c[0][0]]['he'].copy()
        static = [c for c, d in enumerate(self.cols) if d['body'] == 0 and d['type'] == 0 and self.hulls[c] is None and d['he'][0] < 1.0]
        self.table = max(static, key=lambda c: self.cols[c]['he'][0] * self.cols[c]['he'][1] * (self.cols[c]['he'][2] < 0.02))
        self.static = static
        self.out = []

    # -- the block
    def block(self, p, R, k=0, base=None):
        s = (self.s0 if base is None else base).copy()
        i = 2 * self.na + 13 * k
        s[i:i + 3] = p
        s[i + 3:i + 7] = _quat(R)
        s[i + 7:i + 13] = 0.0
        return s

    def add(self, tag, s):
        self.out.append((tag, s))

    def on_table(self, R, gap, xy=None):
        """the block with orientation R, its lowest point `gap` above the table top, over xy (table coordinates; default: a spot clear of the fixtures)"""
        t = self.cols[self.table]
        top = t['p'][2] + t['he'][2]
        reach = np.abs(R[2, :]) @ self.he
        xy = self.spot if xy is None else xy
        return np.array([xy[0], xy[1], top + gap + reach])

    # -- a box face / edge / corner against the outermost hull vertex of collider c along u
    def against(self, V, u, R, pen, lateral=None):
        """centre of the block (orientation R) whose extreme point along -u sits at the support vertex of V along u, pushed in by pen (negative: apart)"""
        v = V[int(np.argmax(V @ u))]
        sg = np.where(u @ R > 0, -1.0, 1.0)                    # the block's corner farthest along -u ... as an offset from its centre
        off = R @ (sg * self.he)
        hb = -(off @ u)                                        # support of the block along -u
        on_face = np.abs(u @ R) > 1 - 1e-9
        if on_face.any():                                      # face-on: the vertex meets the face's centre unless a lateral offset is asked for
            c = v + u * (hb - pen)
            if lateral is not None:
                c = c + R @ lateral
            return c
        return v - pen * u - off


def _arm_depth(b, box, axis, sign):
    """lowest hull vertex of the arm against the face (axis, sign) of static box `box`: signed gap to the face's plane, over all arm links with a hull"""
    d = b.cols[box]
    n = d['R'][:, axis] * sign
    best = np.inf
    for c, cd in enumerate(b.o.collider_list()):
        if 1 <= cd['body'] <= b.na:
            V = b.o.hull_vertices(c)
            if V is not None:
                best = min(best, float(((V - d['p']) @ n).min() - d['he'][axis]))
    return best


def poses(kind, o):
    """[(tag, state)]: `o` is an OracleEnv of the id after reset() (any precision; only forward kinematics and tables are read, in float64 on return)"""
    rng = np.random.default_rng(SEED + ord(kind))
    b = _Builder(o, kind)
    he = b.he
    t = b.cols[b.table]
    # a spot on the table clear of everything else: the candidate farthest from every other collider's centre
    cand = [np.array([t['p'][0] + fx * t['he'][0], t['p'][1] + fy * t['he'][1]]) for fx in (-0.6, -0.3, 0.0, 0.3, 0.6) for fy in (-0.7, -0.4, 0.0, 0.4)]
    others = [d for c, d in enumerate(b.cols) if c != b.table and c not in b.block_c[0] and d['he'][0] < 1.0]
    b.spot = max(cand, key=lambda xy: min(np.linalg.norm(d['p'][:2] - xy) - np.linalg.norm(d['he'][:2]) for d in others))
    Rz = lambda a: _rot([0, 0, 1], a)

    for yaw in (0.0, 0.3, np.pi / 4, 1.1):
        for gap in (-5e-3, -1e-3, -1e-4, -1e-5, 1e-5, 1e-4):
            b.add('flat', b.block(b.on_table(Rz(yaw), gap), Rz(yaw)))
    for yaw in (0.0, 0.7):
        for ax in ([1, 0, 0], [0, 1, 0]):
            for gap in (-1e-3, -1e-4, 1e-4):
                R = Rz(yaw) @ _rot(ax, np.pi / 4)
                b.add('edge45', b.block(b.on_table(R, gap), R))
    diag = he / np.linalg.norm(he)
    Rc = _frame(np.array([0.0, 0.0, 1.0])) @ _frame(diag).T      # takes the body diagonal to +z
    for yaw in (0.0, 0.9):
        for tilt in (0.0, 0.05):
            for gap in (-1e-3, -1e-4, 1e-4):
                R = Rz(yaw) @ _rot([1, 0, 0], tilt) @ Rc
                b.add('corner', b.block(b.on_table(R, gap), R))
    # over the table's edges: the block's centre on the edge line (half of it overhangs), a quarter in, and over the table's corners
    ex, ey = t['p'][0] + t['he'][0], t['p'][1] - t['he'][1]
    for yaw, gap in ((0.0, -1e-3), (np.pi / 2, -1e-4), (0.4, -1e-3)):
        if True:
            for xy in ((ex, b.spot[1]), (ex - 0.5 * he[1], b.spot[1]), (b.spot[0], ey), (ex, ey)):
                b.add('overhang', b.block(b.on_table(Rz(yaw), gap, xy), Rz(yaw)))
    # crossed edges: the block rolled 45 degrees about its long axis, that edge pitched down across the table's +x edge
    for th in (0.3, 0.6, 1.0):
        for skew in (0.0, 0.5):
            for gap in ((-2e-3, 2e-4) if skew == 0.0 else (-2e-4, -5e-3)):
                d = Rz(skew) @ np.array([np.cos(th), 0.0, -np.sin(th)])
                n = np.cross(np.array([0.0, 1.0, 0.0]), d)
                n /= np.linalg.norm(n)
                if n[2] < 0:
                    n = -n
                m = np.cross(d, n)
                R = np.stack([d, (n - m) / np.sqrt(2), (n + m) / np.sqrt(2)], axis=1)
                E = np.array([ex, b.spot[1], t['p'][2] + t['he'][2]])
                c = E + gap * n + he[1] * R[:, 1] + he[2] * R[:, 2] + 0.2 * he[0] * d
                b.add('crossed', b.block(c, R))
    # block against block (two-block id), in the air away from everything; the other ids: the block tumbled on the table
    for i in range(16):
        yaw, gap = (0.0, 0.5, np.pi / 2, 2.0)[i % 4], (-5e-3, -1e-3, -1e-4, 1e-4)[i // 4]
        if o.n_free >= 3 and len(b.block_c[1]) == 1 and np.allclose(b.cols[b.block_c[1][0]]['he'], he):
            R = Rz(yaw)
            c0 = np.array([b.spot[0], b.spot[1], t['p'][2] + t['he'][2] + 0.25])
            s = b.block(c0, R)
            ax = i % 3
            b.add('blocks', b.block(c0 + R[:, ax] * (2 * he[ax] + gap), R, k=1, base=s))
        else:
            q = rng.normal(size=4)
            R = _frame(q[:3])
            R = R @ _rot([1, 0, 0], q[3])
            b.add('tumbled', b.block(b.on_table(R, gap), R))
    # the block against the robot's links: the arm's largest links, the fingers, the static base
    hull_cols = [c for c in range(len(b.cols)) if b.hulls[c] is not None]
    arm_hulls = [c for c in hull_cols if b.cols[c]['body'] >= 1]
    base_hulls = [c for c in hull_cols if b.cols[c]['body'] == 0]
    fingers = [c for c in arm_hulls if b.cols[c]['body'] >= b.na - 1]
    targets = fingers[:1] + base_hulls[:1] + arm_hulls[3:5]
    blk = b.block_c[0][0]
    for ti, c in enumerate(targets):
        V = b.hulls[c]
        thr = min(b.cols[c]['threshold'], b.cols[blk]['threshold'])
        ctr = V.mean(0)
        for j in range(1):
            # the direction, of twelve drawn, that leaves the block (20 mm in, face-on) farthest from every OTHER robot link: the pose is about this pair
            best = None
            for _ in range(12):
                u = V[int(rng.integers(len(V)))] - ctr
                u /= np.linalg.norm(u)
                F = _frame(-u)                                   # face-on: the block's +x face looks along -u
                cc = b.against(V, u, F, 2e-2)
                clear = np.inf
                for c2 in hull_cols:
                    if c2 != c:
                        q = np.abs((b.hulls[c2] - cc) @ F) - he
                        clear = min(clear, float((np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)).min()))
                if best is None or clear > best[0]:
                    best = (clear, u, F)
            _, u, F = best
            for pen in (-(thr + 2e-3 + 1e-4), -(thr + 2e-3 - 1e-4), 1e-3 - 2e-3, 5e-3, 2e-2)[:(5 if j == 0 else 2)]:
                # (pen counts from the CORES: the two 0.001 margins make the shapes touch 2 mm earlier)
                b.add('link_face', b.block(b.against(V, u, F, pen), F))
            for dl in (-1e-4, 1e-4):
                lat = np.array([0.0, he[1] + dl, 0.3 * he[2]])
                b.add('link_rim', b.block(b.against(V, u, F, 1e-3 - 2e-3, lateral=lat), F))
            Re = F @ _rot([0, 0, 1], np.pi / 4)                  # an edge toward the link
            Rk = F @ _rot([0, 0, 1], 0.6) @ _rot([0, 1, 0], 0.5)   # a corner toward the link
            for R2, pens in ((Re, (-1e-3, 1e-3, 5e-3)), (Rk, (-(thr + 2e-3 - 1e-4), 1e-3, 5e-3, 2e-2))):
                for pen in (pens if j == 0 else pens[:2]):
                    b.add('link_edge', b.block(b.against(V, u, R2, pen), R2))
    # a grasp: the block between the two fingertips, its thin side along the line between them, the finger joints swept
    if len(fingers) >= 2:
        f1, f2 = fingers[0], fingers[-1]
        lo, hi = o.arm_table()[:, 1], o.arm_table()[:, 2]
        for i in range(8):
            s = b.s0.copy()
            fj = [k for k in range(b.na) if b.cols[f1]['body'] - 1 == k or b.cols[f2]['body'] - 1 == k]
            for k in fj:
                s[k] = lo[k] + (hi[k] - lo[k]) * (i / 7.0)
            o.set_state(s)
            cl = o.collider_list()
            p1, p2 = cl[f1]['p'], cl[f2]['p']
            e = (p2 - p1) / max(np.linalg.norm(p2 - p1), 1e-9) if np.linalg.norm(p2 - p1) > 1e-6 else cl[f1]['R'][:, 1]
            zh = cl[f1]['R'][:, 2] - (cl[f1]['R'][:, 2] @ e) * e
            zh /= np.linalg.norm(zh)
            R = np.stack([np.cross(e, zh), e, zh], axis=1)
            b.add('grasp', b.block(0.5 * (p1 + p2), R, base=s))
        o.set_state(b.s0)
    # the sphere collider
    sph = [c for c, d in enumerate(b.cols) if d['type'] == 1]
    if sph:
        d = b.cols[sph[0]]
        r, thr = d['he'][0], min(d['threshold'], b.cols[blk]['threshold'])
        u = np.array([0.0, -0.6, 0.8])
        for R2, gaps in ((_frame(-u), (thr - 1e-4, thr + 1e-4, -1e-3)), (_frame(-u) @ _rot([0, 0, 1], np.pi / 4), (thr - 1e-4, -1e-3)),
                         (_frame(-u) @ _rot([0, 0, 1], 0.6) @ _rot([0, 1, 0], 0.5), (thr - 1e-4, -1e-3))):
            for g in gaps:
                sg = np.where(u @ R2 > 0, -1.0, 1.0)
                off = R2 @ (sg * he)
                face = np.abs(u @ R2) > 1 - 1e-9
                c = d['p'] + u * (r + g) + (u * -(off @ u) if face.any() else -off)
                b.add('sphere', b.block(c, R2))
        b.add('sphere', b.block(d['p'] + np.array([0.3 * he[0], 0.1 * he[1], 0.2 * he[2]]), np.eye(3)))
    # the arm itself into the table top and into the nearest static wall
    n_main = 6 if kind == 'U' else 7
    lo, hi = o.arm_table()[:, 1], o.arm_table()[:, 2]
    walls = [c for c in b.static if c != b.table and b.cols[c]['he'][2] > 0.05]
    faces = [(b.table, 2, 1.0)]
    if walls:
        w = min(walls, key=lambda c: np.linalg.norm(b.cols[c]['p'] - b.cols[arm_hulls[-1]]['p']))
        ax = int(np.argmin(b.cols[w]['he']))
        sgn = 1.0 if (b.cols[arm_hulls[-1]]['p'] - b.cols[w]['p']) @ b.cols[w]['R'][:, ax] > 0 else -1.0
        faces.append((w, ax, sgn))
    tries = 0
    arm_added = 0
    while arm_added < 24 and tries < 200:
        box, ax, sgn = faces[tries % len(faces)]
        tries += 1
        dq = np.zeros(b.na)
        dq[:n_main] = rng.normal(size=n_main)
        dq /= np.linalg.norm(dq)
        depth = (5e-4, 1e-3 + 2e-3, 5e-3, 2e-2)[arm_added % 4]

        def f(tt):
            s = b.s0.copy()
            s[:b.na] = np.clip(b.s0[:b.na] + tt * dq, lo, hi)
            o.set_state(s)
            return _arm_depth(b, box, ax, sgn) + depth, s
        t0, t1 = 0.0, None
        for tt in np.arange(0.05, 3.0, 0.05):
            if f(tt)[0] < 0:
                t1 = tt
                break
            t0 = tt
        if t1 is None or f(0.0)[0] < 0:
            continue
        for _ in range(40):
            tm = 0.5 * (t0 + t1)
            if f(tm)[0] < 0:
                t1 = tm
            else:
                t0 = tm
        s = f(t1)[1]
        o.contacts()
        cc = o.collide_counts()                                  # (a pose that runs into a shared cap says nothing about the narrowphase: another direction)
        o.set_state(s)
        if cc['pairs'] > 48 or cc['candidates'] > 48 or cc['manifolds'] > 9 or cc['contacts'] > 17 or cc['torsional'] > 4:
            continue
        b.add('arm_table', s)
        arm_added += 1
    o.set_state(b.s0)
    # fill to N_POSES with the block tumbled on the table at random depths
    while len(b.out) < N_POSES:
        q = rng.normal(size=4)
        R = _frame(q[:3]) @ _rot([1, 0, 0], q[3])
        b.add('tumbled', b.block(b.on_table(R, float(rng.choice([-3e-3, -1e-3, -1e-4, 1e-4]))), R))
    assert len(b.out) == N_POSES, len(b.out)
    return b.out
