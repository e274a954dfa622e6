"""The cases and the float64 truth of closest_points (rp_closest_points): per collider an exact shape WITHOUT margin - the convex hull for a link that has one, the
exact box otherwise, point plus radius for a sphere - built from the oracle's collider list (contact_truth.Scene.from_oracle), and per asked pair the exact signed
distance D* through contact_truth.signed_distance (the facets of the Minkowski difference; sphere against box in closed form), extended by closed forms where that
function asserts: sphere against sphere and sphere against hull.  No GJK runs here.

Asked pairs of an id (`asked_pairs`): every pair of the model's baked pair table, every pair of arm-link colliders, and the block's colliders against every collider
that belongs neither to the arm nor to the block; the wide build's two-block id, checked for distances only, asks its two blocks against everything (`pairs_of`).  Poses: a fixed subset of contact_poses.poses(kind) (`POSES`; `WIDE_POSES` for the wide build's two-block id), chosen so that regenerating an id takes well under
a minute: D* of a pair depends on the two shapes alone, so it is cached by the shapes' vertices, and most poses move only the block.

`python tests/closest_cases.py --write` regenerates tests/golden/closest_points.json (D* per id, pose and asked pair; needs scipy) and prints the fp32 allowance
figures that FP32_WORST records."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import contact_poses as cp  # noqa: E402
import contact_truth as ct  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'closest_points.json')
IDS = {'U': 'UR5PlayAbsRPY1Obj-v0', 'P': 'pandaPick-v0', 'V': 'pandaPlayAbsRPY1Obj-v0', 'W': 'pandaPlay-v0'}      # W: the wide build's id, one pose set
BAND = ct.BAND
# indices into contact_poses.poses(kind), by family: flat (5 mm deep, 0.1 mm above), link_face (5 mm in), link_edge (5 mm in), grasp (the fingers move), and
# 159: on the ids with a sphere the block's centre inside it, on pandaPick an arm_table pose (the arm in the table).  The same list for every id: the families sit at
# the same places.  Few enough that the golden, which keeps the first pose whole and the later ones as differences, stays a file one can read.
POSES = (0, 5, 91, 97, 146, 159)
WIDE_POSES = (97,)      # pandaPlay-v0: a block's edge 5 mm into a link


def poses_of(kind):
    return WIDE_POSES if kind == 'W' else POSES

# The worst |D*(fp32 inputs) - D*| per id over POSES and the asked pairs (metres): every pose record (R, p, he) and every hull vertex rounded to float32 before the
# float64 distance.  tests/test_closest_reference.py asserts its own run reproduces the entry (at most it, no less than a quarter of it: contact_poses.FP32_WORST's
# convention).  The device's bound is max(3 x entry, 2e-6 m) - `device_bound`.
FP32_WORST = {'U': 3.3e-08, 'P': 1.9e-08, 'V': 2.9e-08, 'W': 2.8e-08}


def device_bound(kind):
    return max(3.0 * FP32_WORST[kind], 2e-6)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def shape_of(scene, c, rounded=False):
    """collider c of a scene as its exact shape, margin 0 (a sphere: the point with margin = radius); rounded: its inputs through float32 first"""
    d = scene.cols[c]
    r = f32 if rounded else (lambda x: np.asarray(x, dtype=np.float64))
    if d['type'] == 1:
        return ct.Shape('point', float(r(d['he'][0])), p=r(d['p']))
    if scene.hulls[c] is not None:
        return ct.Shape('hull', 0.0, V=r(scene.hulls[c]))
    return ct.Shape('box', 0.0, R=r(d['R']), p=r(d['p']), he=r(d['he']))


def pair_class(A, B):
    k = sorted((A.kind, B.kind))
    return {('box', 'box'): 'box-box', ('box', 'hull'): 'hull-box', ('hull', 'hull'): 'hull-hull', ('box', 'point'): 'sphere-box', ('hull', 'point'): 'sphere-hull',
            ('point', 'point'): 'sphere-sphere'}[tuple(k)]


def point_hull_signed(V, x):
    """signed distance of point x to conv(V): outside, Wolfe's minimum-norm point (contact_truth.point_hull_distance); inside, minus the depth below the nearest facet"""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(V).equations
    s = float((eq[:, :3] @ x + eq[:, 3]).max())
    if s <= 0.0:
        return s
    return ct.point_hull_distance(V, x)[0]


def signed_distance(A, B):
    """D* of two shapes: contact_truth.signed_distance, and closed forms for the two classes it asserts on"""
    if A.kind == 'point' and B.kind == 'point':
        return float(np.linalg.norm(A.V[0] - B.V[0])) - A.margin - B.margin
    if (A.kind, B.kind) in (('point', 'hull'), ('hull', 'point')):
        s, o = (A, B) if A.kind == 'point' else (B, A)
        return point_hull_signed(o.V, s.V[0]) - A.margin - B.margin
    return ct.signed_distance(A, B)


def asked_pairs(scene, n_free):
    """[(a, b)]: the model's pair table, every pair of arm-link colliders, the block (the first free body, where the id has one) against every scene collider;
    each unordered pair once, in this order"""
    t = scene.t
    n = len(scene.cols)
    arm = [c for c in range(n) if scene.is_arm(c)]
    block = [c for c in range(n) if n_free > 0 and scene.cols[c]['body'] == t['n_arm'] + 1]
    out, seen = [], set()
    cand = [tuple(p) for p in t['pairs']] + [(a, b) for i, a in enumerate(arm) for b in arm[i + 1:]] + [(a, b) for a in block for b in range(n) if b not in arm and b not in block]
    for a, b in cand:
        key = (min(a, b), max(a, b))
        if a != b and key not in seen:
            seen.add(key)
            out.append((a, b))
    return out


class Truth:
    """D* per pose and asked pair of one id, with a cache by the two shapes' vertices"""

    def __init__(self, kind):
        from oracle import OracleEnv
        self.kind = kind
        self.tables = ct.model_tables(kind)
        self.o = OracleEnv(kind, seed=7, env_index=0)
        self.o.reset()
        self.all_poses = cp.poses(kind, self.o)
        self.cache = {}

    def scene(self, i):
        self.o.set_state(self.all_poses[i][1])
        return ct.Scene.from_oracle(self.tables, self.o)

    def dstar(self, scene, pairs, rounded=False):
        shapes = {}
        out = []
        for a, b in pairs:
            for c in (a, b):
                if c not in shapes:
                    s = shape_of(scene, c, rounded)
                    shapes[c] = (s, (s.kind, s.margin, s.V.tobytes()))
            key = (shapes[a][1], shapes[b][1])
            if key not in self.cache:
                self.cache[key] = signed_distance(shapes[a][0], shapes[b][0])
            out.append(self.cache[key])
        return out


def pairs_of(kind, scene, n_free):
    """the pairs asked of an id: asked_pairs; on the wide build's two-block id, whose one pose set checks distances only, the two blocks against each other and
    against every other collider"""
    if kind != 'W':
        return asked_pairs(scene, n_free)
    n = len(scene.cols)
    blocks = [c for c in range(n) if scene.cols[c]['body'] in (scene.t['n_arm'] + 1, scene.t['n_arm'] + 2)]
    return [(a, b) for a in blocks for b in range(n) if b not in blocks or b > a]


UNIT = 1e-10      # the golden keeps D* as integers of 0.1 nm: 300 times finer than the fp32 allowance, 20 000 times finer than the device's bound


def load_golden():
    """{kind: dict(id, poses, tags, n_pairs, dstar [pose][pair] in metres)}.  The file keeps the first pose's row whole and of every later pose the entries that differ
    from it (most poses move only the block); the pair list is pairs_of's and is not stored"""
    with open(GOLDEN) as f:
        raw = json.load(f)
    out = {}
    for kind, e in raw.items():
        base = np.array(e['first'], dtype=np.int64)
        rows = [base]
        for idx, val in e['later']:
            r = base.copy()
            r[idx] = val
            rows.append(r)
        out[kind] = dict(id=e['id'], poses=e['poses'], tags=e['tags'], n_pairs=len(base), dstar=[(r * UNIT).tolist() for r in rows])
    return out


def write_golden():
    import time
    lines = []
    for kind in IDS:
        t0 = time.time()
        tr = Truth(kind)
        P = poses_of(kind)
        pairs = pairs_of(kind, tr.scene(P[0]), tr.o.n_free)
        rows, worst = [], 0.0
        for i in P:
            sc = tr.scene(i)
            d = np.array(tr.dstar(sc, pairs))
            rows.append(np.round(d / UNIT).astype(np.int64))
            d32 = np.array(tr.dstar(sc, pairs, rounded=True))
            worst = max(worst, float(np.abs(rows[-1] * UNIT - d32).max()))
        later = []
        for r in rows[1:]:
            idx = np.nonzero(r != rows[0])[0]
            later.append('[%s,%s]' % (json.dumps(idx.tolist(), separators=(',', ':')), json.dumps(r[idx].tolist(), separators=(',', ':'))))
        lines.append('"%s":{"id":"%s","poses":%s,"tags":%s,\n"first":%s,\n"later":[%s]}' % (
            kind, IDS[kind], json.dumps(list(P)), json.dumps([tr.all_poses[i][0] for i in P]), json.dumps(rows[0].tolist(), separators=(',', ':')), ',\n'.join(later)))
        print('%s: %d poses x %d pairs in %.1f s, fp32 worst |dD*| %.3e' % (kind, len(P), len(pairs), time.time() - t0, worst))
    with open(GOLDEN, 'w') as f:
        f.write('{' + ',\n'.join(lines) + '}\n')
    print('wrote %s (%d bytes)' % (GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == '__main__':
    if '--write' in sys.argv:
        write_golden()
