"""The scenes of tests/test_gpu_prep2_tail.py and the CPU check of what they cover (tests/test_prep2_tail_coverage.py): crowded scenes (tests/crowded_scenes.py,
unchanged) of the UR5 and the Panda one-object play ids, 64 each, picked from the seeded pool so that the set meets the places where the tail of k_prep2's collision
wave takes another path - and each with a SECOND pose for the substep after the history-free one: the same arm, drawer and scene joints, the free block where the
pool's next scene has it, so that the block's manifolds of the first substep leave and others are created while the rest of the cache goes on.

What the fp32 oracle says of a scene (its counters, its contact lists, its cache rows after either collision phase) is computed here once and shared."""
import functools

import numpy as np

import cache_rows
import crowded_scenes as cs

POOL, PICK, PER_CASE = 1500, 64, 3
# the cases and what decides them: lengths of a contact list (0; 8 | 9: the end of k_prep2's first chunk of PREP_CH contact rows), manifolds that want a slot
# (PM_MAX = 11), torsional rows (MAXT = 4), a manifold created / leaving in the second substep
CASES = ('contacts 0', 'contacts 8', 'contacts 9', 'manifolds 11', 'torsional 4', 'created', 'left')
# ... and the long lists, which the crowded scenes of these ids do not reach (their longest: 12): 16 | 17 contacts (the end of the second chunk of contact rows)
# and 21 with more wanted, MAXC's cut falling INSIDE a manifold.  Two sources, both seeded and checked by the oracle's own counters:
#   seeded()  the persistent model (the default): states of a random-action rollout on the oracle, each with its own contact cache PADDED - every manifold that holds
#             a point holds k = 2, 3 or 4, the extra slots filled with copies of its points (a legal cache: a copy is refreshed and kept like its original, a
#             candidate replaces one point only) - so that the collision phase that follows wants up to 4 contacts of every touching object pair;
#   wide()    the stateless model that a uniform contact margin selects on the device and in the oracle alike (margin 0.05: tests/test_gpu_boundary.py), on the
#             crowded scenes: its merge is sequential, its lists run through the same solver order, chunks and copy-out.
LONG_CASES = ('contacts 16', 'contacts 17', 'contacts 21 cut')
WIDE_MARGIN = 0.05


def _keys(row):
    return [m[0] for m in cache_rows.manifolds(row)]


def cases_of(sc):
    n1, n2 = len(sc['contacts']), len(sc['contacts2'])
    out = set()
    for n in (0, 8, 9):
        if n in (n1, n2):
            out.add('contacts %d' % n)
    if 11 in (sc['counts']['manifolds'], sc['counts2']['manifolds']):
        out.add('manifolds 11')
    if 4 in (sc['counts']['torsional'], sc['counts2']['torsional']):
        out.add('torsional 4')
    if sc['created']:
        out.add('created')
    if sc['left']:
        out.add('left')
    return out


@functools.lru_cache(maxsize=None)
def select(kind):
    """PICK scenes of `kind` ('U', 'V'): crowded_scenes' dicts plus state2, contacts2, counts2 (the second collision phase, on the first one's cache), row1 / row2
    (the oracle's cache row after either phase), created / left (manifold keys that appear / disappear in the second phase)"""
    from oracle import OracleEnv
    pool = [sc for sc in cs.generate(kind, POOL, seed=0) if not sc['deep']]
    o = OracleEnv(cs.IDS[kind], seed=7, env_index=0, f32=True)
    o.reset()
    na = o.n_arm
    nf = (len(pool[0]['state']) - 2 * na) // 13
    drawer = cs.drawer_slot(kind, nf)
    out = []
    for i, sc in enumerate(pool):
        s1, nxt = sc['state'], pool[(i + 1) % len(pool)]['state']
        s2 = s1.copy()
        for k in range(nf):
            if k != drawer:
                s2[2 * na + 13 * k:2 * na + 13 * k + 7] = nxt[2 * na + 13 * k:2 * na + 13 * k + 7]
        o.set_state(s1)
        o.contacts()
        row1 = o.get_cache_row()
        o.set_state(s2)
        o.set_cache_row(row1)
        oc2 = o.contacts()
        counts2 = o.collide_counts()
        row2 = o.get_cache_row()
        o.set_state(s1)
        if len(oc2) and float(oc2[:, 8].min()) < -cs.DEEP:      # (as the pool's own rule: beyond 6 mm rounding picks the EPA face)
            continue
        k1, k2 = _keys(row1), _keys(row2)
        out.append(dict(sc, state2=s2, contacts2=oc2, counts2=counts2, row1=row1, row2=row2, created=[k for k in k2 if k not in k1], left=[k for k in k1 if k not in k2]))
    picked, seen = [], set()
    for case in CASES:                                          # the first PER_CASE scenes of every case, then the pool in its order
        for j, sc in enumerate(out):
            if case in cases_of(sc) and sum(case in cases_of(out[t]) for t in picked) < PER_CASE and j not in seen:
                picked.append(j)
                seen.add(j)
    for j in range(len(out)):
        if len(picked) >= PICK:
            break
        if j not in seen:
            picked.append(j)
            seen.add(j)
    return [out[j] for j in sorted(picked[:PICK])]


def coverage(scenes):
    """{case: scenes that show it}"""
    return {case: sum(case in cases_of(sc) for sc in scenes) for case in CASES}


def pad_cache(row, k):
    """the cache row with every non-empty manifold filled up to k points by copies of its own"""
    row = np.array(row, dtype=np.float32)
    w = row.view(np.int32)
    for i in range(int(w[0])):
        b = cache_rows.HDR + cache_rows.MAN * i
        n = int(w[b + 1])
        for q in range(n, k if n else 0):
            row[b + 8 + cache_rows.PT * q:b + 8 + cache_rows.PT * (q + 1)] = row[b + 8 + cache_rows.PT * (q % n):b + 8 + cache_rows.PT * (q % n + 1)]
        if n:
            w[b + 1] = max(n, k)
    return row


def cut_inside_a_manifold(oc, counts, row):
    """MAXC contacts listed, more wanted, and some manifold of the cache `row` (as the phase left it) has at least two but not all of its points in the list
    (a rotation-locked body's manifold against the world lists one point whatever it holds: two listed points rule that out)"""
    if len(oc) != cs.CAPS['contacts'] or counts['contacts'] <= cs.CAPS['contacts']:
        return False
    listed = [int(r[0]) | (int(r[1]) << 8) for r in oc]
    for m in cache_rows.decode(row)['manifolds']:
        hit = sum(listed.count(ab) for ab in set(m['ab']))
        if 2 <= hit < m['n'] and len(set(m['ab'])) == 1:
            return True
    return False


def long_cases_of(sc):
    out = set()
    n = len(sc['contacts'])
    if n in (16, 17):
        out.add('contacts %d' % n)
    if sc['cut']:
        out.add('contacts 21 cut')
    return out


def _pick_long(found):
    picked = []
    for case in LONG_CASES:
        picked += [sc for sc in found if case in long_cases_of(sc)][:PER_CASE]
    seen, out = set(), []
    for sc in picked:
        if id(sc) not in seen:
            seen.add(id(sc))
            out.append(sc)
    return out


@functools.lru_cache(maxsize=None)
def seeded(kind, envs=32, steps=60):
    """persistent model: dict(state, seed_row (the padded cache), contacts / counts / row2 (the oracle's collision phase on state + seed_row), cut)"""
    from oracle import OracleEnv
    found = []
    for e in range(envs):
        o = OracleEnv(cs.IDS[kind], seed=11, env_index=e, f32=True)
        o.reset()
        hi = np.asarray(o.action_high())
        rng = np.random.default_rng([3, e])
        for _ in range(steps):
            o.step(rng.uniform(-1, 1, len(hi)) * hi)
            s, row = o.get_state(), o.get_cache_row()
            for k in (2, 3, 4):
                seed_row = pad_cache(row, k)
                o.set_state(s)
                o.set_cache_row(seed_row)
                oc = o.contacts()
                counts, row2 = o.collide_counts(), o.get_cache_row()
                sc = dict(state=s, seed_row=seed_row, contacts=oc, counts=counts, row2=row2, cut=cut_inside_a_manifold(oc, counts, row2))
                if long_cases_of(sc) and not (len(oc) and float(oc[:, 8].min()) < -cs.DEEP):
                    found.append(sc)
            o.set_state(s)
            o.set_cache_row(row)
    return _pick_long(found)


@functools.lru_cache(maxsize=None)
def wide(kind):
    """stateless model at WIDE_MARGIN on the crowded pool: dict(state, contacts, counts, cut (21 listed, more wanted))"""
    from oracle import OracleEnv
    o = OracleEnv(cs.IDS[kind], seed=7, env_index=0, f32=True, margin=WIDE_MARGIN)
    o.reset()
    found = []
    for sc in cs.generate(kind, 300, seed=0):
        if sc['deep']:
            continue
        o.set_state(sc['state'])
        oc = o.contacts()
        counts = o.collide_counts()
        o.set_state(sc['state'])
        found.append(dict(state=sc['state'], contacts=oc, counts=counts, cut=len(oc) == cs.CAPS['contacts'] and counts['contacts'] > cs.CAPS['contacts']))
    return _pick_long(found)
