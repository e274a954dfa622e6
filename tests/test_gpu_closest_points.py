"""closest_points (rp_closest_points, k_closest_points) against the float64 truth of tests/closest_cases.py: per id the golden's poses are written into a row buffer
and ONE call with all asked pairs answers them; status, distance, witnesses, normal, the max_distance cut, the group reduction, the live path, bad indices and the
call's side effects are then checked on that call's results.  D* comes from tests/golden/closest_points.json; the bound per id is closest_cases.device_bound:
max(3 x the fp32 allowance the CPU test measures, 2e-6 m).  Each id's device calls are made once and shared by the tests of that id.

Measured on an MI355X (bound 2e-6 m for every id): worst |distance - D*| over the separated cases 1.0e-7 (U), 1.2e-7 (P), 1.3e-7 (V), 4.2e-8 (W); witnesses off their
shapes by at most 1.9e-7, an overlapping pair's common point outside a shape by at most 3.4e-8; no CAPPED pair."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, 'oracle'), os.path.join(REPO, 'tools'), HERE) if p not in sys.path]
import closest_cases as cc  # noqa: E402
import contact_truth as ct  # noqa: E402

SEP, OVERLAP, FAR, SKIPPED, CAPPED = 0, 1, 2, 3, 4
CUT = 0.02
G = 6            # groups 0 .. 4 take the pairs in turn, group 5 stays empty
KINDS = ('U', 'P', 'V')
_SHARED = {}


def _record(o, kind):
    if kind == 'W':
        from test_gpu_parity import wide_record_from_oracle
        return wide_record_from_oracle(o)
    from gpu_debug import record_from_oracle
    return record_from_oracle(o)


def _env(kind):
    from roboticsplayroompybullet_amd import VecPlayEnv
    return VecPlayEnv(cc.IDS[kind], 2, seed=7)


def shared(kind):
    """once per id, left unchanged: the golden, the scenes (float64 shapes), the row buffer, and the results of the stored-rows calls with and without the cut"""
    if kind not in _SHARED:
        from oracle import OracleEnv
        import contact_poses as cp
        e = cc.load_golden()[kind]
        o = OracleEnv(cc.IDS[kind], seed=7)
        o.reset()
        poses = cp.poses(kind, o)
        tables = ct.model_tables(kind)
        scenes, recs = [], []
        pairs_ab = None
        for i in e['poses']:
            o.set_state(poses[i][1])
            scenes.append(ct.Scene.from_oracle(tables, o))
            pairs_ab = pairs_ab or cc.pairs_of(kind, scenes[0], o.n_free)
            recs.append(_record(o, kind))
            o.set_state(poses[i][1])
        env = _env(kind)
        rows = torch.tensor(np.stack(recs), device=env.device)
        pairs = np.array([[a, b, k % (G - 1)] for k, (a, b) in enumerate(pairs_ab)], dtype=np.int32)
        assert len(pairs) == e['n_pairs']
        pairs_t = torch.tensor(pairs, device=env.device)
        state0 = env.get_state().clone()
        img0 = {k: v.clone() for k, v in env.render_layers(48, 48).items()}
        res = env.closest_points(pairs_t, states=rows, n_groups=G)
        cut = env.closest_points(pairs_t, states=rows, max_distance=CUT, n_groups=G)
        img1 = env.render_layers(48, 48)
        state1 = env.get_state()
        torch.cuda.synchronize()
        _SHARED[kind] = dict(env=env, golden=e, ab=pairs_ab, D=np.array(e['dstar']), scenes=scenes, rows=rows, pairs=pairs, pairs_t=pairs_t, bound=cc.device_bound(kind),
                             res={k: v.cpu().numpy() for k, v in res.items()}, cut={k: v.cpu().numpy() for k, v in cut.items()}, res_t=res,
                             untouched=bool(torch.equal(state0, state1)) and all(torch.equal(img0[k], img1[k]) for k in img0))
    return _SHARED[kind]


@pytest.mark.parametrize('kind', KINDS)
def test_status_and_distance(kind):
    sh = shared(kind)
    D, r, bound = sh['D'], sh['res'], sh['bound']
    st, dist = r['status'], r['distance'].astype(np.float64)
    assert st.shape == D.shape
    capped = (st & CAPPED) != 0
    base = st & 3
    print('%s: %d cases, %d separated, %d overlapping, %d capped' % (kind, D.size, int((base == SEP).sum()), int((base == OVERLAP).sum()), int(capped.sum())))
    assert not capped.any(), 'CAPPED on %d cases' % int(capped.sum())
    assert set(np.unique(base)) <= {SEP, OVERLAP}
    out = np.abs(D) >= cc.BAND
    wrong = out & (base != np.where(D > 0, SEP, OVERLAP))
    assert not wrong.any(), [(int(p), sh['ab'][int(k)], float(D[p, k]), int(st[p, k])) for p, k in np.argwhere(wrong)[:8]]
    sep = base == SEP
    gap = np.abs(dist - D)[sep & (D > 0)]
    print('%s: |distance - D*| over %d separated cases: worst %.3e (bound %.1e)' % (kind, gap.size, gap.max(), bound))
    assert gap.max() <= bound
    assert (dist[sep & (D <= 0)] <= bound).all()      # (within the band: separated by the device, touching by the truth)
    assert (dist[capped] >= D[capped] - bound).all()
    # OVERLAP: distance exactly 0, the normal exactly 0, both witnesses the same point
    ov = base == OVERLAP
    assert (r['distance'][ov] == 0.0).all() and (r['normal'][ov] == 0.0).all() and (r['point_a'][ov] == r['point_b'][ov]).all()


@pytest.mark.parametrize('kind', KINDS)
def test_witnesses_lie_on_their_shapes(kind):
    sh = shared(kind)
    r, bound, pairs = sh['res'], sh['bound'], sh['ab']
    st = r['status'] & 3
    pa, pb, nr, dist = (r[k].astype(np.float64) for k in ('point_a', 'point_b', 'normal', 'distance'))
    sep = st == SEP
    span = np.abs(pa - pb - nr * dist[..., None]).max(-1)[sep].max()
    unit = np.abs(np.linalg.norm(nr, axis=-1) - 1.0)[sep].max()
    print('%s: |point_a - point_b - normal distance| worst %.3e, | |normal| - 1 | worst %.3e' % (kind, span, unit))
    assert span <= bound and unit <= 1e-6
    worst = {SEP: 0.0, OVERLAP: 0.0}
    for p, sc in enumerate(sh['scenes']):
        shapes = {}
        for k, (a, b) in enumerate(pairs):
            for c, x in ((a, pa[p, k]), (b, pb[p, k])):
                if c not in shapes:
                    shapes[c] = cc.shape_of(sc, c)
                d, slack = shapes[c].core_distance(x)
                # separated: ON the shape (a sphere's witness at its radius from the centre); overlapping: the common point IN the shape
                off = abs(d - shapes[c].margin) if st[p, k] == SEP else d - shapes[c].margin
                worst[int(st[p, k])] = max(worst[int(st[p, k])], off - slack)
    print('%s: witness off its shape: separated worst %.3e, common point outside its shape worst %.3e (bound %.1e)' % (kind, worst[SEP], worst[OVERLAP], bound))
    assert worst[SEP] <= bound and worst[OVERLAP] <= bound


@pytest.mark.parametrize('kind', KINDS)
def test_the_cut_and_the_groups(kind):
    sh = shared(kind)
    D, r, c, bound = sh['D'], sh['res'], sh['cut'], sh['bound']
    far = (c['status'] & 3) == FAR
    print('%s: max_distance %.2f: %d of %d cases FAR, least D* among them %.4f' % (kind, CUT, int(far.sum()), D.size, D[far].min() if far.any() else np.inf))
    assert far.any() and (D[far] > CUT - bound).all()
    assert (c['distance'][far] == np.float32(CUT)).all() and (c['point_a'][far] == 0).all() and (c['point_b'][far] == 0).all() and (c['normal'][far] == 0).all()
    near = (D <= CUT - bound) & ~far & ((c['status'] & 3) != OVERLAP)
    assert near.any()
    for k in ('distance', 'point_a', 'point_b', 'normal', 'status'):
        assert np.array_equal(c[k][near].view(np.int32), r[k][near].view(np.int32)), k
    # (in fact every pair that is not FAR keeps its bits)
    for k in ('distance', 'point_a', 'point_b', 'normal', 'status'):
        assert np.array_equal(c[k][~far].view(np.int32), r[k][~far].view(np.int32)), k
    # groups: a reduction of the same call's distance / status in pair order, the lowest index among equals; group G - 1 is empty
    grp = torch.tensor(sh['pairs'][:, 2].astype(np.int64))
    for name, x in (('no cut', r), ('cut', c)):
        dist, st = torch.tensor(x['distance']), torch.tensor(x['status'])
        for g in range(G):
            idx = torch.nonzero(grp == g)[:, 0]
            if len(idx) == 0:
                assert np.isposinf(x['group_min'][:, g]).all() and (x['group_pair'][:, g] == -1).all()
                continue
            d = dist[:, idx]
            assert ((st[:, idx] & 3) != SKIPPED).all()
            m, j = d.min(1)
            first = (d == m[:, None]).to(torch.int8).argmax(1)      # the first of the equals
            assert np.array_equal(x['group_min'][:, g].view(np.int32), m.numpy().view(np.int32)), (name, g)
            assert np.array_equal(x['group_pair'][:, g], idx[first].numpy().astype(np.int32)), (name, g)


@pytest.mark.parametrize('kind', KINDS)
def test_the_live_envs_give_the_stored_rows_bits_and_nothing_else_moves(kind):
    sh = shared(kind)
    assert sh['untouched'], 'get_state() or render_layers() changed across the stored-rows calls'
    env, rows, r = sh['env'], sh['rows'], sh['res']
    state0 = env.get_state().clone()
    for lo in range(0, rows.shape[0], 2):
        cnt = min(2, rows.shape[0] - lo)      # (an odd last row: set_state gives it to both envs)
        env.set_state(rows[lo:lo + cnt])
        live = env.closest_points(sh['pairs_t'], n_groups=G)
        for k, v in live.items():
            assert np.array_equal(v.cpu().numpy()[:cnt].view(np.int32), r[k][lo:lo + cnt].view(np.int32)), (k, lo)
    env.set_state(state0)


def test_chunks_of_rows_give_the_same_bits():
    """the rows walked in chunks of 4 and of 5 pose-table slots (rp_debug_render_states_chunk: the call shares rp_render_states' chunks), with and without an index:
    every output is moved to the chunk's first row on the host"""
    sh = shared('P')
    env, rows, r = sh['env'], sh['rows'], sh['res']
    n = rows.shape[0]
    assert n % 5 != 0
    perm = torch.tensor([(5 * i + 2) % n for i in range(n)], dtype=torch.int32, device=env.device)
    try:
        for chunk in (4, 5):
            env._call('rp_debug_render_states_chunk', chunk)
            plain = env.closest_points(sh['pairs_t'], states=rows, n_groups=G)
            gathered = env.closest_points(sh['pairs_t'], states=rows, index=perm, n_groups=G)
            for k in plain:
                assert np.array_equal(plain[k].cpu().numpy().view(np.int32), r[k].view(np.int32)), (chunk, k)
                assert np.array_equal(gathered[k].cpu().numpy().view(np.int32), r[k][perm.cpu().numpy()].view(np.int32)), (chunk, k)
    finally:
        env._call('rp_debug_render_states_chunk', 0)


@pytest.mark.parametrize('kind', KINDS)
def test_bad_indices_are_skipped_cells(kind):
    """a row index of -1 or past the buffer, a pair with a == b, a collider number of 64: status SKIPPED in those cells, their prefilled outputs untouched, everything
    else written as the plain call writes it.  Specified early exits."""
    sh = shared(kind)
    env, rows, r = sh['env'], sh['rows'], sh['res']
    n = rows.shape[0]
    index = torch.tensor([1, -1, 0, n, n - 1], dtype=torch.int32, device=env.device)
    good = [0, 2, 4]
    src = [1, 0, n - 1]
    K = 12
    pairs = sh['pairs'][:K].copy()
    pairs[3] = [5, 5, 0]
    pairs[7] = [0, 64, 1]
    pairs[9] = [-1, 2, 1]
    bad_k = [3, 7, 9]
    pairs[:, 2] = [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2]
    out = {'distance': torch.full((5, K), 7.5, device=env.device), 'point_a': torch.full((5, K, 3), 7.5, device=env.device),
           'point_b': torch.full((5, K, 3), 7.5, device=env.device), 'normal': torch.full((5, K, 3), 7.5, device=env.device),
           'status': torch.full((5, K), -9, dtype=torch.int32, device=env.device)}
    res = env.closest_points(torch.tensor(pairs, device=env.device), states=rows, index=index, n_groups=4, out=out)
    x = {k: v.cpu().numpy() for k, v in res.items()}
    ok_k = [k for k in range(K) if k not in bad_k]
    for k in ('distance', 'point_a', 'point_b', 'normal', 'status'):
        assert np.array_equal(x[k][good][:, ok_k].view(np.int32), r[k][src][:, ok_k].view(np.int32)), k
    skipped = np.ones((5, K), dtype=bool)
    for g in good:
        skipped[g, ok_k] = False
    assert (x['status'][skipped] == SKIPPED).all()
    for k in ('distance', 'point_a', 'point_b', 'normal'):
        assert (x[k][skipped] == 7.5).all(), k
    # the groups leave the skipped pairs out; a row that is all skipped has empty groups
    assert np.isposinf(x['group_min'][[1, 3]]).all() and (x['group_pair'][[1, 3]] == -1).all()
    assert np.isposinf(x['group_min'][:, 3]).all() and (x['group_pair'][:, 3] == -1).all()
    for row, s in zip(good, src):
        for g in range(3):
            ks = [k for k in ok_k if pairs[k, 2] == g]
            d = r['distance'][s][ks]
            assert x['group_min'][row, g] == d.min() and x['group_pair'][row, g] == ks[int(np.argmax(d == d.min()))]


def test_the_wide_build_s_distances():
    """pandaPlay-v0, served by the wide build: one pose set, distances only"""
    sh = shared('W')
    D, r, bound = sh['D'], sh['res'], sh['bound']
    base = r['status'] & 3
    out = np.abs(D) >= cc.BAND
    assert not (out & (base != np.where(D > 0, SEP, OVERLAP))).any() and not (r['status'] & CAPPED).any()
    gap = np.abs(r['distance'].astype(np.float64) - D)[(base == SEP) & (D > 0)]
    print('W: |distance - D*| over %d separated cases: worst %.3e (bound %.1e)' % (gap.size, gap.max(), bound))
    assert gap.max() <= bound
