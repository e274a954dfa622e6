"""Every camera path and moved scene of the render code on the MI355X against the float64 ray cast of tests/camera_cases.py over the oracle's collider poses: the three
layers at every (id, state, camera) of the table - aspect != 1, fov 170, per-env rows each against its own row, a moved arm, moved fixtures, a tumbled block, the Panda's
hulls, the wide build -, the gripper camera against the reference's own formula, where every ghost is drawn and which sub-goal entry moves it, rp_ray_test at its edges,
and camera() against cameras().  tests/test_camera_cases.py shows on the CPU that the reference alone stays under 0.002 of the pixels.  Run with -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytest.importorskip('scipy')

import camera_cases as cc      # noqa: E402

pytestmark = pytest.mark.gpu
_HANDLES = {}


def handle(gid):
    """one 3-env handle per id for the whole module, reset with the table's seed"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    if gid not in _HANDLES:
        env = VecPlayEnv(gid, cc.NUM_ENVS, seed=cc.SEEDS[gid])
        env.reset()
        torch.cuda.synchronize()
        _HANDLES[gid] = env
    return _HANDLES[gid]


def put(gid, state):
    """the handle of the id with every env in the state: the oracle's numbers through record_from_oracle + set_state.  The wide id stays as reset() left it (env e = the
    oracle with env_index e): record_from_oracle knows the narrow record only."""
    from gpu_debug import record_from_oracle
    env = handle(gid)
    if gid != cc.W2:
        rec = record_from_oracle(cc.oracle_of(gid, state))
        env.set_state(torch.tensor(np.tile(rec, (cc.NUM_ENVS, 1))))
    else:
        assert state == 'reset'
    return env


def device_camera(env, name, o):
    kw = cc.camera_kwargs(name, o)
    return env.camera(**kw)


def hold(got, ref, far, label):
    """the comparison of check (a): got = dict(rgb [h, w, 3], depth [h, w], segmentation [h, w]) of one env as numpy arrays, ref = reference_layers' dict"""
    seg, z, rgb = got['segmentation'], got['depth'], got['rgb']
    h, w = seg.shape
    agree = seg == ref['seg']
    hit = agree & (ref['who'] >= 0)
    firm = hit & (ref['ndotd'] >= cc.GRAZE)
    zerr = np.where(firm, np.abs(z - ref['z']), 0.0)
    cerr = np.where(agree, np.abs(rgb.astype(int) - cc.to_bytes(ref['rgb']).astype(int)).max(axis=2), 0)
    print(label, '%d x %d' % (w, h), 'segmentation agrees on %.5f' % agree.mean(), 'hits %.3f' % (ref['who'] >= 0).mean(), 'max depth error %.2e' % zerr.max(),
          'pixels over 2e-4: %d' % (zerr > cc.DEPTH_TOL).sum(), 'max colour error', cerr.max(), 'pixels over 1 count: %d' % (cerr > 1).sum())
    for k in np.argsort(zerr.ravel())[-2:]:
        y, x = divmod(int(k), w)
        print('   depth  pixel', (x, y), 'collider', ref['who'][y, x], 'depth', z[y, x], 'want', ref['z'][y, x], 'error', zerr[y, x], '|n . d|', ref['ndotd'][y, x])
    for k in np.argsort(cerr.ravel())[-2:]:
        y, x = divmod(int(k), w)
        print('   colour pixel', (x, y), 'collider', ref['who'][y, x], 'rgb', rgb[y, x], 'want', cc.to_bytes(ref['rgb'])[y, x], '|n . d|', ref['ndotd'][y, x])
    assert agree.mean() >= cc.SEG_CAP, (label, agree.mean())
    assert zerr.max() <= cc.DEPTH_TOL, (label, zerr.max())
    assert cerr.max() <= 1, (label, cerr.max(), int((cerr > 1).sum()))
    miss = agree & (ref['who'] < 0)
    assert (z[miss] == np.float32(far)).all() and (seg[miss] == -1).all(), label


def one_env(layers, e):
    return {k: v[e].cpu().numpy() for k, v in layers.items()}


LAYER_CASES = [(gid, state, name) for gid in cc.IDS for state in cc.STATES[gid] for name in cc.CAMERA_NAMES]


@pytest.mark.parametrize('gid,state,name', LAYER_CASES)
def test_layers_match_the_float64_ray_cast(gid, state, name):
    """(a): render_layers(depth='metres') at both sizes.  Segmentation agrees on at least 0.995 of the pixels; on agreeing hits with |n . d| >= 0.02 the depth is within
    2e-4 m; on agreeing pixels rgb is within 1 count; misses read far and -1.  Per-env rows: each env against its own row's reference."""
    env = put(gid, state)
    envs = range(cc.NUM_ENVS) if (name == 'rows' or gid == cc.W2) else (0,)
    for w, h in cc.SIZES:
        if name == 'rows':
            rows = env.cameras(**cc.ROWS)
            got = env.render_layers(width=w, height=h, cameras=rows, depth='metres', near=cc.NEAR, far=cc.FAR)
            cams = [cc.camera_values(r) for r in rows.cpu().numpy()]
        elif gid == cc.W2 and name in ('fov170', 'close'):          # aimed at the first block, which lies elsewhere in every env: one call per env
            got, cams = None, None
        else:
            cam = device_camera(env, name, cc.oracle_of(gid, state))
            got = env.render_layers(width=w, height=h, camera=cam, depth='metres', near=cc.NEAR, far=cc.FAR)
            cams = [cc.camera_values(cam)] * cc.NUM_ENVS
        for e in envs:
            o = cc.oracle_of(gid, state, e)
            if got is None:
                cam = device_camera(env, name, o)
                mine, c = one_env(env.render_layers(width=w, height=h, camera=cam, depth='metres', near=cc.NEAR, far=cc.FAR, envs=(e, e + 1)), 0), cc.camera_values(cam)
            else:
                mine, c = one_env(got, e), cams[e]
            hold(mine, cc.reference_layers(o, c, w, h, cc.NEAR, cc.FAR), cc.FAR, '%s %s %s env %d' % (gid, state, name, e))


GRIPPER_CASES = [(gid, state) for gid in (cc.U, cc.V) for state in cc.GRIPPER_STATES]


@pytest.mark.parametrize('gid,state', GRIPPER_CASES)
def test_gripper_camera_is_the_references(gid, state):
    """(b): the gripper camera at the reset pose, at an EE roll of about pi and at two general orientations, through render() and render_layers(), against the reference's
    formula (camera_cases.gripper_basis).  Away from roll = pi the reference's picture and the picture of the link-frame basis (-z, +x) - what the library drew for every
    pose before - differ on more than 20 % of the pixels, so a camera that points the wrong way cannot pass."""
    env = put(gid, state)
    o = cc.oracle_of(gid, state)
    cam = env.camera(gripper=True)
    c = cc.camera_values(cam)
    for w, h in ((cc.SIZES[0], cc.GRIPPER_SIZE_UR5) if gid == cc.U else (cc.SIZES[0],)):
        ref = cc.reference_layers(o, c, w, h, cc.NEAR, cc.FAR)
        if state != 'grip_pi':
            other = cc.reference_layers(o, dict(c, basis='link'), w, h, cc.NEAR, cc.FAR)
            apart = (cc.to_bytes(ref['rgb']) != cc.to_bytes(other['rgb'])).any(axis=2).mean()
            print(gid, state, w, h, 'reference and link-frame pictures differ on', apart)
            assert apart > 0.2, apart
        layers = env.render_layers(width=w, height=h, camera=cam, depth='metres', near=cc.NEAR, far=cc.FAR)
        image = env.render('rgb_array', width=w, height=h, camera=cam)
        assert torch.equal(image, layers['rgb'])
        mine = one_env(layers, 0)
        hold(mine, ref, cc.FAR, '%s %s gripper render_layers' % (gid, state))
        hold(dict(mine, rgb=image[0].cpu().numpy()), ref, cc.FAR, '%s %s gripper render' % (gid, state))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (c) ghosts

def region_matches(mine, want):
    """two changed-pixel sets are the same region: intersection over union at least 0.98, or - for a region of a few dozen pixels, where one silhouette pixel is more than
    2 % - no more than two pixels apart (one silhouette pixel either way)"""
    union, both = int((mine | want).sum()), int((mine & want).sum())
    return both >= 0.98 * union or union - both <= 2


def ghost_picture(env, gid, o, w, h, sub_goal=None, ghost_arm=None):
    """(device image of env 0, reference image) with these ghosts"""
    kw, ghosts = {}, []
    if sub_goal is not None:
        kw['sub_goal'] = torch.tensor(np.tile(sub_goal, (cc.NUM_ENVS, 1)), dtype=torch.float32)
        ghosts.append(cc.ghost_records(cc.sub_goal_oracle(gid, o, sub_goal)))
    if ghost_arm is not None:
        kw['ghost_arm'] = torch.tensor(np.tile(ghost_arm, (cc.NUM_ENVS, 1)), dtype=torch.float32)
        ghosts.append(cc.ghost_records(cc.ghost_arm_oracle(gid, o, ghost_arm), arm=True))
    got = env.render('rgb_array', width=w, height=h, **kw)[0].cpu().numpy()
    ref = cc.to_bytes(cc.reference_layers(o, cc.camera_values(env.camera()), w, h, ghosts=ghosts)['rgb'])
    return got, ref


def bare_picture(env, o, w, h):
    return env.render('rgb_array', width=w, height=h)[0].cpu().numpy(), cc.to_bytes(cc.reference_layers(o, cc.camera_values(env.camera()), w, h)['rgb'])


def hold_ghosts(label, got, ref, bare_got, bare_ref):
    close = (np.abs(got.astype(int) - ref.astype(int)) <= 1).all(axis=2)
    mine, want = (got != bare_got).any(axis=2), (ref != bare_ref).any(axis=2)
    iou = (mine & want).sum() / max((mine | want).sum(), 1)
    print(label, 'rgb within 1 count on %.5f' % close.mean(), 'changed pixels', int(mine.sum()), 'reference', int(want.sum()), 'intersection over union %.4f' % iou)
    assert close.mean() >= cc.SEG_CAP, (label, close.mean())
    assert want.sum() > 0 and iou >= 0.98, (label, iou)


@pytest.mark.parametrize('gid,arm,goal', [(cc.U, False, True), (cc.V, True, False), (cc.V, True, True), (cc.W2, False, True)])
def test_ghosts_are_drawn_where_the_reference_draws_them(gid, arm, goal):
    """(c): the UR5's sub-goal (block 12 cm aside, drawer -0.05, door 0.1, button 0.01, dial 0.8), the Panda's ghost arm alone and with a sub-goal, the wide id's sub-goal
    that moves the second object only.  render()'s rgb is within 1 count of the ghost reference - the nearest ghost nearer than the solid hit blends half and half - on at
    least 0.995 of the pixels, and the pixels the ghosts change are the reference's (intersection over union at least 0.98)."""
    env, o = put(gid, 'reset'), cc.oracle_of(gid, 'reset')
    w, h = cc.GHOST_SIZE
    got, ref = ghost_picture(env, gid, o, w, h, sub_goal=cc.sub_goal_vector(gid, o, cc.GHOST_COMBINED[gid]) if goal else None, ghost_arm=cc.ghost_arm_pose(o) if arm else None)
    hold_ghosts('%s arm %s sub-goal %s' % (gid, arm, goal), got, ref, *bare_picture(env, o, w, h))


@pytest.mark.parametrize('gid', [cc.U, cc.W2])
def test_every_sub_goal_entry_moves_its_own_body(gid):
    """(c): each entry of the sub-goal moved alone.  The reference's changed region is not empty and is disjoint from another entry's, and the device's region is that
    region - a wrong index into the sub-goal vector would move another body."""
    env, o = put(gid, 'reset'), cc.oracle_of(gid, 'reset')
    w, h = cc.GHOST_SIZE
    bare_got, bare_ref = bare_picture(env, o, w, h)
    mine, want = {}, {}
    for k in cc.GHOST_ENTRIES[gid]:
        got, ref = ghost_picture(env, gid, o, w, h, sub_goal=cc.sub_goal_vector(gid, o, (k,)))
        mine[k], want[k] = (got != bare_got).any(axis=2), (ref != bare_ref).any(axis=2)
        print(gid, k, 'changed pixels', int(mine[k].sum()), 'reference', int(want[k].sum()), 'in both', int((mine[k] & want[k]).sum()))
    for k in want:
        assert want[k].sum() > 0, k
        assert any(not (want[k] & want[j]).any() for j in want if j != k), k
        assert region_matches(mine[k], want[k]), (k, int(mine[k].sum()), int(want[k].sum()), int((mine[k] & want[k]).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (d) rp_ray_test

def edge_rays(o, k):
    """(from [k, 3], to [k, 3], tangent = the indices of the tangent pair, the table's collider, the block's) in float32 values: the edge rays in the order of the docstring below, then random ones"""
    R, p, tab = o.colliders()
    body = np.array([c['body'] for c in o.collider_list()])
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)      # noqa: E731
    straight = [c for c in range(len(tab)) if body[c] == 0 and tab[c, 0] == 0 and np.array_equal(R[c], np.eye(3))]
    table = max(straight, key=lambda c: np.prod(tab[c, 1:4]))          # the largest static box that stands square to the world: the table
    block = int(np.flatnonzero(body == o.n_arm + 1)[0])
    globe = int(np.flatnonzero(tab[:, 0] == 1)[0])
    pt, ht, pb, pg, rg = f32(p[table]), f32(tab[table, 1:4]), f32(p[block]), f32(p[globe]), float(tab[globe, 1])
    air = f32([0.3, -0.3, 0.5])
    rays = [(air, air), (pt, pt), (pg, pg),                                                          # zero length: outside, inside a box, inside the globe
            (pt, pt + [0.0, 0.0, 1.0]), (pb, pb + [0.0, 0.0, 0.3]),                                  # starting inside the table's box and inside the block
            (pt - [ht[0] + 0.2, 0, 0], pt + [ht[0] + 0.2, 0, 0]),                                    # along x through the table: parallel to four of its faces
            (pt - [ht[0] + 0.2, ht[1] + 0.01, 0], pt + [ht[0] + 0.2, -(ht[1] + 0.01), 0]),           # ... and past it, 1 cm outside its y slab
            (pt + [0.01, -0.02, ht[2] + 0.05], pt + [0.01, -0.02, -ht[2] - 0.1]),                     # along z down onto it
            (pt + [ht[0] + 0.01, -0.02, ht[2] + 0.05], pt + [ht[0] + 0.01, -0.02, -ht[2] - 0.1]),     # ... and down beside it
            (pb + [0, 0, 0.3], pb + [0, 0, 0.026]), (pb + [0, 0, 0.3], pb + [0, 0, 0.024]),          # ending 1 mm short of the block's top (2.5 cm up) and 1 mm past it
            (pg + [-0.3, 0, rg + 1e-4], pg + [0.3, 0, rg + 1e-4]), (pg + [-0.3, 0, rg - 1e-4], pg + [0.3, 0, rg - 1e-4])]      # tangent to the globe's top, either side
    tangent = (len(rays) - 2, len(rays) - 1)
    rng = np.random.default_rng(0)
    n = k - len(rays)
    frm = np.concatenate([rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(0.3, 0.6, (n, 1))], axis=1)
    to = np.concatenate([rng.uniform(-0.4, 0.5, (n, 2)), rng.uniform(-0.3, 0.0, (n, 1))], axis=1)
    frm = np.concatenate([np.array([r[0] for r in rays]), frm])[:k]
    to = np.concatenate([np.array([r[1] for r in rays]), to])[:k]
    return f32(frm), f32(to), tangent, table, block


def firm_decisions(R, p, tab, hulls, frm, to):
    """(t, collider, normal) of the float64 cast and where its decision has a margin: the same collider (or the same miss) with the ray moved by 1e-4 m along each axis
    either way and with the segment 1e-5 shorter and longer"""
    t, who, nrm = cc.cast(R, p, tab, frm, to - frm, 1.0, hulls)
    firm = np.ones(len(who), dtype=bool)
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            shift = np.zeros(3)
            shift[axis] = sgn * 1e-4
            firm &= cc.cast(R, p, tab, frm + shift, to - frm, 1.0, hulls)[1] == who
    for tmax in (1.0 - 1e-5, 1.0 + 1e-5):
        firm &= cc.cast(R, p, tab, frm, to - frm, tmax, hulls)[1] == who
    return t, who, nrm, firm


@pytest.mark.parametrize('k', [65, 1])
def test_ray_test_edges(k):
    """(d): K = 65 rays per env - the 64-lane stride loop wraps once - and K = 1.  In this order: zero length (from == to) outside, inside a box and inside the globe;
    starting inside the table's box and inside the block; exactly parallel to the table's faces, passing and missing (the |d| < 1e-12 branch); ending 1 mm short of the
    block's top and 1 mm past it; tangent to the globe within 1e-4 m on either side; the rest random.  Collider and link are the float64 cast's wherever its decision has a
    margin (the tangent pair only has to be finite), the fraction is within 2e-5, every output is finite, and a miss reports fraction 1, collider -1, link -1,
    hit_position == to and a zero normal."""
    env, o = put(cc.U, 'reset'), cc.oracle_of(cc.U, 'reset')
    frm, to, tangent, table, block = edge_rays(o, 65)
    if k == 1:          # the ray that ends 1 mm past the block's top
        frm, to, tangent = frm[10:11], to[10:11], ()
    out = env.ray_test(torch.tensor(np.tile(frm, (cc.NUM_ENVS, 1, 1)), dtype=torch.float32), torch.tensor(np.tile(to, (cc.NUM_ENVS, 1, 1)), dtype=torch.float32))
    torch.cuda.synchronize()
    R, p, tab = o.colliders()
    t, who, nrm, firm = firm_decisions(R, p, tab, cc.oracle_hulls(o), frm, to)
    for e in range(cc.NUM_ENVS):
        got = {key: v[e].cpu().numpy() for key, v in out.items()}
        assert all(np.isfinite(v).all() for v in got.values())
        held = firm.copy()
        held[list(tangent)] = False
        want_link = np.where(who >= 0, tab[np.maximum(who, 0), 8].astype(int), -1)
        print('env', e, 'firm', int(held.sum()), 'of', k, 'colliders', got['collider'][:13], 'want', who[:13])
        assert held.sum() >= k - 8
        assert (got['collider'][held] == who[held]).all(), (got['collider'], who, held)
        assert (got['link'][held] == want_link[held]).all()
        want_t = np.where(who >= 0, t, 1.0)
        same = held & (got['collider'] == who)
        print('   max fraction error', np.abs(got['hit_fraction'][same] - want_t[same]).max())
        np.testing.assert_allclose(got['hit_fraction'][same], want_t[same], rtol=0, atol=2e-5)
        miss = got['collider'] < 0
        assert (got['hit_fraction'][miss] == 1.0).all() and (got['link'][miss] == -1).all()
        assert np.array_equal(got['hit_position'][miss], to[miss].astype(np.float32)) and (got['hit_normal'][miss] == 0.0).all()
        if k == 65:
            assert (who[[0, 1, 2, 9, 11]] == -1).all() and (who[[5, 7]] == table).all() and (who[[3, 6, 8]] != table).all() and who[10] == block and tab[who[12], 0] == 1      # the edge rays are the cases they are meant to be


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (e) camera() and cameras()

def test_camera_and_cameras_agree_bit_for_bit():
    """(e): eye / target / up of camera() and of a cameras() row are the same float32 values for five (yaw, pitch, roll, distance), roll != 0 among them, and at roll = 0
    they are computeViewMatrixFromYawPitchRoll's (upAxis 2) in numpy to 1e-6.  Which way a non-zero roll turns the camera has no reference value without PyBullet, so
    roll's own convention is not asserted: only that the two paths share it."""
    env = handle(cc.U)
    target = (0.1, 0.2, 0.05)
    for yaw, pitch, roll, dist in ((-30.0, -30.0, 0.0, 1.3), (20.0, -40.0, 0.0, 2.0), (75.0, -10.0, 15.0, 0.8), (-160.0, -89.0, -40.0, 3.0), (123.4, 35.0, 170.0, 0.09)):
        cam = env.camera(target=target, distance=dist, yaw=yaw, pitch=pitch, roll=roll, fov=42.0, aspect=1.25)
        row = env.cameras(target=target, distance=dist, yaw=yaw, pitch=pitch, roll=roll, fov=42.0, aspect=1.25)[0].cpu().numpy()
        mine = np.array(list(cam.eye) + list(cam.target) + list(cam.up) + [cam.fov_deg, cam.aspect], dtype=np.float32)
        assert mine.tobytes() == row.tobytes(), (yaw, pitch, roll, dist, mine, row)
        if roll == 0.0:
            y, pt = np.radians(yaw), np.radians(pitch)
            Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
            Rx = np.array([[1, 0, 0], [0, np.cos(pt), -np.sin(pt)], [0, np.sin(pt), np.cos(pt)]])
            tg = np.array(target, dtype=np.float32).astype(np.float64)
            np.testing.assert_allclose(mine[0:3], tg + Rz @ Rx @ np.array([0, -dist, 0]), atol=1e-6)
            np.testing.assert_allclose(mine[6:9], Rz @ Rx @ np.array([0, 0, 1.0]), atol=1e-6)
