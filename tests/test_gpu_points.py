"""rp_render_points / rp_set_image_points on the MI355X: per-env point clouds compacted by k_point_cloud from a view's depth and segmentation layers.  Run with -m gpu.

The yardstick is never the code under test:
  layers       render_layers with the same camera arguments - the path tests/test_gpu_camera_cases.py holds to a float64 ray cast; the layers render_points hands
               back must be those bytes
  selection    the numpy rule of tests/point_cloud_cases.py applied to those layers: segmentation, rgb, count and padding EXACT, no tolerance
  coordinates  a float64 evaluation of the rule's formula, the float32 camera numbers the device was given read as float64 and the rays built as
               camera_cases.pixel_rays builds them: |delta| <= XYZ_TOL per component; the camera-frame z is the depth value bit for bit
XYZ_TOL = 2e-5 m: coordinates are at most ~12 m, where one float32 ulp is 9.5e-7; there are fewer than ten roundings; the basis and the tangent are rounded to float32,
6e-8 relative at z <= 10 m; the sum is under 1e-5, doubled.

The gripper camera in the world frame has its own yardstick: the same call's camera-frame cloud, mapped through camera_cases.camera_basis at the ORACLE's EE link; the
gap is the device-vs-oracle EE pose gap times the lever arm (GRIPPER_WORLD_GAP below).

In the step: the clouds written by step, calc_state, masked resets and both passes of the autoreset step are held, byte for byte, to render_points of the same or a
twin handle in that state, with test_gpu_image_obs' sentinel pattern for the rows that must not be written."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
import point_cloud_cases as pc
from reset_rows import reset_rows
from test_gpu_autoreset import actions, end_masks, make
from test_gpu_image_obs import fill_sentinel, is_sentinel, per_env_cameras, same_bytes
from test_gpu_reset_table import start_table

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

U, P, W = 'UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'pandaPlay-v0'
ALL = ('rgb', 'depth', 'segmentation')
XYZ_TOL = 2e-5
# the worst |device world-frame point - camera-frame point mapped through the oracle's EE basis| over the grip_a / grip_b states of the UR5 and the Panda play ids
# (70 x 45, every real point), metres; measured on the MI355X on 2026-10-21.  The test asserts 4 x this: the margin covers another float32 arm state.
GRIPPER_WORLD_GAP = 1.5548e-07          # UR5 grip_a 7.26e-08, grip_b 1.08e-07; Panda grip_a 1.29e-07, grip_b 1.55e-07
GRIPPER_WORLD_CAP = 1e-3          # the bound must stay under this, or the feature's world frame is not good enough to ship
POINT_KEYS = ('xyz', 'segmentation', 'count')


def to_np(t):
    return {k: (to_np(v) if isinstance(v, dict) else v.cpu().numpy()) for k, v in t.items()}


def camera_list(env, n, kw):
    """camera_values of every env of a call: float64 of the float32 numbers the device got"""
    if kw.get('cameras') is not None:
        return [cc.camera_values(r) for r in kw['cameras'].cpu().numpy()]
    cam = kw.get('camera')
    if cam is None:
        cam = env.camera()
    return [cc.camera_values(cam)] * n


def drop_bits(env, names):
    return pc.drop_mask(c for c, nm in enumerate(env.visual_names) if nm in names)


def hold_cloud(env, w, h, n_points, kw, frame, max_depth=None, drop=(), colour=False, envs=None, xyz=True):
    """render_points(...) against the three yardsticks of the header.  Returns (the cloud as numpy, the reference selections per env, the worst coordinate error)"""
    got = env.render_points(w, h, n_points, envs=envs, frame=frame, max_depth=max_depth, drop=drop, colour=colour, **kw)
    lay = env.render_layers(width=w, height=h, envs=envs, depth='metres', layers=ALL, **kw)
    torch.cuda.synchronize()
    assert set(got) == set(POINT_KEYS) | {'layers'} | ({'rgb'} if colour else set())
    assert set(got['layers']) == {'depth', 'segmentation'} | ({'rgb'} if colour else set())
    for k, t in got['layers'].items():
        assert same_bytes(t, lay[k]), k
    n_env = lay['depth'].shape[0]
    assert got['xyz'].shape == (n_env, n_points, 3) and got['xyz'].dtype == torch.float32
    assert got['segmentation'].shape == (n_env, n_points) and got['segmentation'].dtype == torch.int32
    assert got['count'].shape == (n_env,) and got['count'].dtype == torch.int32
    g, L = to_np(got), to_np(lay)
    cams = camera_list(env, n_env, kw)
    refs, worst = [], 0.0
    for e in range(n_env):
        ref = pc.cloud(L['depth'][e], L['segmentation'][e], n_points, max_depth or 0.0, drop_bits(env, drop), rgb=L['rgb'][e] if colour else None)
        refs.append(ref)
        assert int(g['count'][e]) == ref['count'], (e, g['count'][e], ref['count'])
        assert (g['segmentation'][e] == ref['segmentation']).all(), e
        if colour:
            assert g['rgb'].dtype == np.uint8 and (g['rgb'][e] == ref['rgb']).all(), e
        real = ref['pixel'] >= 0
        assert (g['xyz'][e][~real].view(np.int32) == 0).all(), e                 # padding: +0.0 in every component
        pix = ref['pixel'][real]
        z = L['depth'][e].ravel()[pix]
        if frame == 'camera':
            assert (g['xyz'][e][real][:, 2].view(np.int32) == z.view(np.int32)).all(), e          # the depth value, bit for bit
        if not xyz or not real.any():
            continue
        c = cams[e]
        if frame == 'camera':
            want = pc.xyz_camera(pix, z, w, h, c['fov'], c['aspect'])
        else:
            assert not c['gripper']
            want = pc.xyz_world(pix, z, w, h, c['fov'], c['aspect'], c['eye'], c['target'], c['up'])
        err = float(np.abs(g['xyz'][e][real].astype(np.float64) - want).max())
        worst = max(worst, err)
        assert err <= XYZ_TOL, (e, err)
    return g, refs, worst


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1: the shapes where the kernel can go wrong

def fixed(env):
    return dict()


def rows(env):
    return dict(cameras=per_env_cameras(env))


def side(env):
    return dict(camera=env.camera(yaw=40.0, distance=1.1, fov=60.0, aspect=1.4))


SHAPES = ((U, 3, 1, 1, fixed), (P, 2, 15, 17, rows), (W, 3, 16, 16, side), (U, 4, 17, 16, rows), (U, 3, 70, 45, side), (P, 7, 70, 45, fixed), (W, 2, 70, 45, rows))


@pytest.mark.parametrize('gid,n_env,w,h,cams', SHAPES, ids=['%s-%dx%d' % (s[0][:6], s[2], s[3]) for s in SHAPES])
def test_every_chunk_shape_at_every_side_of_p(gid, n_env, w, h, cams):
    """1 x 1, 255, 256 and 272 pixels (a chunk less one, exactly one, one and a ragged second) and 70 x 45 (many chunks, ragged): n is read from the layers first, then
    P = 1, n - 1, n, n + 1 and more than width * height are asked for - n of env 0, asserted to lie on the intended side of P; the other envs' n differ - in the world
    frame, and P = n and the large P in the camera frame too, with colour"""
    env = make(gid, n_env, 5)
    env.reset()
    kw = cams(env)
    lay = env.render_layers(width=w, height=h, depth='metres', layers=('segmentation',), **kw)
    n = int((lay['segmentation'][0] != -1).sum())
    assert n >= 1, 'the view of env 0 must hit something'
    sides = {1: n >= 1, n - 1: n > n - 1, n: True, n + 1: n < n + 1, w * h + 5: n < w * h + 5}
    seen = set()
    for n_points, intended in sides.items():
        if n_points < 1:
            continue          # (n == 1: there is no P = n - 1)
        assert intended
        g, refs, worst = hold_cloud(env, w, h, n_points, kw, 'world')
        assert refs[0]['count'] == n
        seen.add('sub' if n > n_points else ('full' if n == n_points else 'pad'))
        if n_points in (n, w * h + 5):
            _, _, worst_c = hold_cloud(env, w, h, n_points, kw, 'camera', colour=True)
            worst = max(worst, worst_c)
        print(gid, '%d x %d' % (w, h), 'n', [r['count'] for r in refs], 'P', n_points, 'worst coordinate error %.2e' % worst)
    assert seen == ({'full', 'pad'} if n == 1 else {'sub', 'full', 'pad'}), seen
    env.close()


def test_a_camera_that_sees_nothing_gives_padding_alone():
    env = make(U, 3, 2)
    env.reset()
    up = dict(camera=env.camera(target=(0.0, 0.25, 3.0), distance=0.5, pitch=60.0))          # from below a point 3 m up, towards the sky
    for frame in ('world', 'camera'):
        g, refs, _ = hold_cloud(env, 17, 16, 40, up, frame, colour=True)
        assert all(r['count'] == 0 for r in refs) and (g['count'] == 0).all()
        assert (g['segmentation'] == -1).all() and (g['xyz'].view(np.int32) == 0).all() and (g['rgb'] == 0).all()
    env.close()


def test_drop_and_max_depth_each_remove_something_and_leave_something():
    env = make(U, 3, 7)
    env.reset()
    w, h, kw = 70, 45, dict()
    lay = to_np(env.render_layers(width=w, height=h, depth='metres', layers=('depth', 'segmentation'), **kw))
    hit = lay['segmentation'][0] != -1
    cut = float(np.median(lay['depth'][0][hit]))
    drop = ('table', 'floor')
    counts = {}
    for name, a in (('none', {}), ('drop', dict(drop=drop)), ('depth', dict(max_depth=cut)), ('both', dict(drop=drop, max_depth=cut))):
        for n_points in (64, w * h):
            g, refs, _ = hold_cloud(env, w, h, n_points, kw, 'world', colour=True, **a)
        counts[name] = refs[0]['count']
        col = g['segmentation'][0][g['segmentation'][0] != -1] & 0xFF
        if 'drop' in a:
            assert not np.isin(col, [c for c, nm in enumerate(env.visual_names) if nm in drop]).any()
    assert counts['none'] == hit.sum()
    assert 0 < counts['drop'] < counts['none'] and 0 < counts['depth'] < counts['none'] and 0 < counts['both'] < min(counts['drop'], counts['depth']), counts
    with pytest.raises(ValueError, match='render_points: drop'):
        env.render_points(8, 8, 16, drop=('tabel',))
    env.close()


def test_products_beyond_32_bits_at_300_by_300():
    """two envs, 300 x 300, P = 65536: n > P, so the ranks' products r * P pass 2^32 (90 000 * 65 536 = 5.9e9)"""
    env = make(U, 2, 3)
    env.reset()
    g, refs, worst = hold_cloud(env, 300, 300, 65536, dict(), 'world')
    for r in refs:
        assert r['count'] > 65536 and (r['count'] - 1) * 65536 > 2 ** 32, r['count']
        assert (np.diff(r['pixel']) > 0).all()
    print('300 x 300: n', [r['count'] for r in refs], 'worst coordinate error %.2e' % worst)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2: the gripper camera

def put(gid, state, n=3):
    """a handle with every env in a state of camera_cases' table: the oracle's numbers through record_from_oracle + set_state"""
    from gpu_debug import record_from_oracle
    env = make(gid, n, cc.SEEDS[gid])
    env.reset()
    env.set_state(torch.tensor(np.tile(record_from_oracle(cc.oracle_of(gid, state)), (n, 1))))
    return env


def gripper_world_gap(gid, state):
    """the gripper camera's two frames at one state (every check but the gap's bound); returns the worst world-frame gap, metres"""
    env = put(gid, state)
    o = cc.oracle_of(gid, state)
    cam = env.camera(gripper=True)
    w, h = cc.SIZES[0]
    kw = dict(camera=cam)
    worst_gap = 0.0
    for n_points in (500, w * h):
        gc, refs, worst = hold_cloud(env, w, h, n_points, kw, 'camera', colour=True)
        gw, refs_w, _ = hold_cloud(env, w, h, n_points, kw, 'world', colour=True, xyz=False)
        assert refs[0]['count'] > 0, 'the gripper camera must see the scene'
        for k in ('segmentation', 'count', 'rgb'):
            assert (gc[k] == gw[k]).all(), k
        eye, target, up = cc.camera_basis(o, cc.camera_values(cam))
        for e in range(env.num_envs):
            real = refs[e]['pixel'] >= 0
            want = pc.camera_to_world(gc['xyz'][e][real], eye, target, up)
            worst_gap = max(worst_gap, float(np.abs(gw['xyz'][e][real].astype(np.float64) - want).max()))
    print('gripper world gap', gid, state, '%.3e' % worst_gap, 'camera-frame error %.2e' % worst)
    env.close()
    return worst_gap


@pytest.mark.parametrize('state', ('grip_a', 'grip_b'))
@pytest.mark.parametrize('gid', (cc.U, cc.V))
def test_gripper_camera_camera_frame_and_world_frame(gid, state):
    """camera frame: the formula's float64 value within XYZ_TOL, z the depth value.  World frame: the SAME selection and count as the camera-frame call, and every
    point within 4 x GRIPPER_WORLD_GAP of the camera-frame point mapped through the reference's basis at the oracle's EE link"""
    gap = gripper_world_gap(gid, state)
    assert 4 * GRIPPER_WORLD_GAP <= GRIPPER_WORLD_CAP
    assert gap <= 4 * GRIPPER_WORLD_GAP, gap


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3: in the step

def cloud_kw(points):
    return dict(n_points=points['n'], frame=points.get('frame', 'world'), max_depth=points.get('max_depth'), drop=points.get('drop', ()),
                colour=points.get('colour', False))


def camera_kw(spec, e):
    kw = {}
    if spec.get('camera') is not None:
        kw['camera'] = spec['camera']
    if spec.get('cameras') is not None:
        kw['cameras'] = spec['cameras'][e:e + 1].contiguous()
    return kw


def assert_points_equal_render_points(env, got, spec, what, envs=None):
    """every row (of `envs`, default all) of a view's cloud = render_points(envs=(e, e + 1), the view's arguments) on env now, byte for byte"""
    points = spec['points']
    assert set(got) == set(POINT_KEYS) | ({'rgb'} if points.get('colour') else set()), what
    for e in (range(env.num_envs) if envs is None else envs):
        want = env.render_points(spec['width'], spec['height'], envs=(e, e + 1), **cloud_kw(points), **camera_kw(spec, e))
        for k in got:
            assert same_bytes(got[k][e:e + 1], want[k]), (what, k, e)


def configure(env, spec):
    """set_image_obs with the spec's view, then set_image_points with its cloud"""
    env.set_image_obs(**{k: v for k, v in spec.items() if k != 'points'})
    env.set_image_points(**spec['points'])


def obs_spec(env, gripper=False):
    if gripper:
        return dict(width=33, height=50, layers=ALL, depth='metres', camera=env.camera(gripper=True), points=dict(n=700, frame='camera', colour=True))
    return dict(width=33, height=50, layers=('depth', 'segmentation'), depth='metres', cameras=per_env_cameras(env),
                points=dict(n=300, max_depth=2.0, drop=('floor',)))


@pytest.mark.parametrize('gid,gripper', ((U, False), (W, True)), ids=('U-rows', 'W-gripper'))
def test_step_calc_state_and_masked_resets_write_the_clouds(gid, gripper):
    """after reset, two steps and calc_state every env's cloud equals render_points of the same handle; reset(mask) and reset(mask, o=...) rewrite the masked envs'
    rows and leave the sentinel in every other row; the tensors are the same objects call to call"""
    n = 5
    env = make(gid, n, 3)
    spec = obs_spec(env, gripper)
    configure(env, spec)
    obs = env.reset()
    start = obs['obs_quat'].clone()
    assert obs['points'] is env.image_points and env.image_points_final is None
    assert_points_equal_render_points(env, obs['points'], spec, 'reset')
    first = obs['points']['xyz'].clone()
    for t, a in enumerate(actions(env, 2, 5)):
        obs, _, _, _ = env.step(a)
        assert obs['points'] is env.image_points
        assert_points_equal_render_points(env, obs['points'], spec, 'step %d' % t)
    assert not same_bytes(first, obs['points']['xyz'])
    fill_sentinel(env.image_points)
    obs = env.calc_state()
    assert_points_equal_render_points(env, obs['points'], spec, 'calc_state')
    chosen = [1, 4]
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[chosen] = 1
    for what, o in (('reset(mask)', None), ('reset(mask, o)', start)):
        if o is not None and o.shape[1] < 28:          # (rp_reset_to reads 18 entries per env of the one-object ids, 28 of the wide one)
            o = torch.cat([o, torch.zeros((n, 28 - o.shape[1]), device=o.device)], 1)
        fill_sentinel(env.image_points)
        obs = env.reset(mask=mask, o=o)
        assert_points_equal_render_points(env, obs['points'], spec, what, envs=chosen)
        for k, t in obs['points'].items():
            for i in set(range(n)) - set(chosen):
                assert is_sentinel(k, t[i]), (what, k, i)
    env.close()


@pytest.mark.parametrize('gid,table', ((U, False), (P, True)), ids=('U-settle', 'P-table'))
def test_autoreset_terminal_clouds_against_a_twin(gid, table):
    """Handle A: autoreset, time limit 3, staggered counters, a random end_mask, a view with a cloud.  Twin B: same seed and actions, plain step, then the masked
    reset.  After each step the ended envs' terminal rows equal B's render_points taken between its step and its reset, every other terminal row keeps the sentinel,
    and A's observation cloud equals A's own render_points after the call.  Step 2 ends every env, step 3 none."""
    n, steps, seed, stagger = 5, 5, 21, 3
    B = make(gid, n, seed)
    tab = start_table(B, 4, seed + 100) if table else None
    A = make(gid, n, seed, autoreset=True, max_episode_steps=stagger, reset_table=tab)
    spec = dict(width=17, height=16, layers=ALL, depth='metres', cameras=per_env_cameras(A), points=dict(n=100, colour=True))
    configure(A, spec)
    assert set(A.image_points_final) == set(POINT_KEYS) | {'rgb'}
    for env in (A, B):
        env.reset()
    dev = A.device
    e = torch.arange(n, device=dev, dtype=torch.int32)
    A.episode_steps = e % stagger
    cnt = (e % stagger).clone()
    acts = actions(A, steps, seed)
    masks = end_masks(n, steps, seed + 1, dev, p=0.2)
    masks[2] = torch.ones(n, device=dev, dtype=torch.uint8)
    masks[3] = torch.zeros(n, device=dev, dtype=torch.uint8)
    cursor, ends = 0, []
    for t in range(steps):
        fill_sentinel(A.image_points_final)
        oa, _, da, ia = A.step(acts[t], end_mask=masks[t])
        B.step(acts[t])
        status = B.buf['status'].clone()
        c1 = cnt + 1
        mask = (c1 >= stagger) | (masks[t] != 0) | ((status & 3) != 0)
        cnt = torch.where(mask, torch.zeros_like(c1), c1)
        ended = [int(i) for i in mask.nonzero().flatten().cpu()]
        last = {i: B.render_points(spec['width'], spec['height'], envs=(i, i + 1), **cloud_kw(spec['points']), **camera_kw(spec, i)) for i in ended}
        if ended:
            if table:
                r, cursor = reset_rows(mask.cpu().numpy(), cursor, tab.shape[0])
                B.reset(mask=mask, o=tab[torch.from_numpy(r).to(dev).clamp(min=0).long()])
            else:
                B.reset(mask=mask)
        torch.cuda.synchronize()
        ends.append(len(ended))
        assert torch.equal(da, mask), t
        term = ia['terminal_observation']['points']
        assert term is A.image_points_final
        for k in term:
            for i in range(n):
                if i in last:
                    assert same_bytes(term[k][i:i + 1], last[i][k]), (t, k, i)
                else:
                    assert is_sentinel(k, term[k][i]), (t, k, i)
        assert_points_equal_render_points(A, oa['points'], spec, 'obs of step %d' % t)
        assert torch.equal(A.get_state(), B.get_state()), t
    assert ends[2] == n and ends[3] == 0 and 0 < ends[0] < n, ends
    for env in (A, B):
        env.close()


def three_views(env):
    """two views with clouds of different sizes around a one-pixel view without one"""
    return {'img': dict(width=33, height=50, layers=('depth', 'segmentation'), depth='metres', points=dict(n=300, drop=('table',))),
            'dot': dict(width=1, height=1, layers=('segmentation',), cameras=per_env_cameras(env)),
            'wrist': dict(width=70, height=45, layers=ALL, depth='metres', camera=env.camera(gripper=True), points=dict(n=4000, frame='camera', colour=True))}


def test_two_views_with_clouds_and_one_without_merged_and_per_view():
    """two autoreset handles with the same seed, one drawing its views in one k_render_views launch, one in a launch per view: the clouds of the observation and of
    the terminal pass are the same bytes, equal render_points view by view, and the view without a cloud has the keys it always had"""
    n = 5
    envs = []
    for on in (1, 0):
        env = make(U, n, 11, autoreset=True, max_episode_steps=2)
        env._call('rp_debug_image_views_merge', on)
        specs = three_views(env)
        env.set_image_views(specs)
        envs.append((env, specs))
    (M, specs), (S, _) = envs
    for env, _ in envs:
        env.reset()
        env.episode_steps = torch.arange(n, device=env.device, dtype=torch.int32) % 2
    assert set(M.image_views['dot']) == {'segmentation'} and set(M.image_views_final['dot']) == {'segmentation'}
    assert set(M.image_views['img']) == {'depth', 'segmentation', 'points'} and set(M.image_views['wrist']) == set(ALL) | {'points'}
    acts = actions(M, 2, 2)
    for t in range(2):
        for env, _ in envs:
            for name in ('img', 'wrist'):
                fill_sentinel(env.image_views_final[name]['points'])
        om, _, dm, im = M.step(acts[t])
        os_, _, ds, is_ = S.step(acts[t])
        torch.cuda.synchronize()
        assert torch.equal(dm, ds) and bool(dm.any()) and not bool(dm.all())
        for name in ('img', 'wrist'):
            assert_points_equal_render_points(M, om['views'][name]['points'], specs[name], 'merged, step %d, %s' % (t, name))
            for a, b in ((om['views'], os_['views']), (im['terminal_observation']['views'], is_['terminal_observation']['views'])):
                for k in a[name]['points']:
                    assert same_bytes(a[name]['points'][k], b[name]['points'][k]), (t, name, k)
            term = im['terminal_observation']['views'][name]['points']
            for i in range(n):          # written where the env ended, the sentinel elsewhere
                assert all(is_sentinel(k, v[i]) != bool(dm[i]) for k, v in term.items()), (t, name, i)
    for env, _ in envs:
        env.close()


def test_replacing_the_configuration_drops_the_cloud_and_no_cloud_changes_nothing():
    """a handle with a cloud and its twin without: same observation otherwise; after set_image_obs again (without points) the old cloud tensors stop changing and
    obs has no 'points'; views without points have exactly their layers"""
    n = 3
    X, Y = make(U, n, 1), make(U, n, 1)
    kw = dict(width=17, height=16, layers=ALL, depth='metres')
    X.set_image_obs(**kw)
    X.set_image_points(50)
    Y.set_image_obs(**kw)
    acts = actions(X, 3, 1)
    for env in (X, Y):
        env.reset()
    ox, _, _, _ = X.step(acts[0])
    oy, _, _, _ = Y.step(acts[0])
    assert set(ox) == set(oy) | {'points'} and 'points' not in oy and Y.image_points is None
    for k in oy:
        if oy[k] is not None:
            assert same_bytes(ox[k], oy[k]), k
    old = dict(X.image_points)
    assert int(old['count'].max()) > 0
    X.set_image_obs(**kw)
    assert X.image_points is None
    fill_sentinel(old)
    ox, _, _, _ = X.step(acts[1])
    torch.cuda.synchronize()
    assert 'points' not in ox and all(is_sentinel(k, t) for k, t in old.items())
    # set_image_views drops it as well, and switching off
    X.set_image_obs(**kw)
    X.set_image_points(50)
    old = dict(X.image_points)
    X.set_image_points(None)          # detached by hand: the tensors stop changing, the observation loses the key
    fill_sentinel(old)
    assert X.image_points is None and 'points' not in X.calc_state()
    torch.cuda.synchronize()
    assert all(is_sentinel(k, t) for k, t in old.items())
    X.set_image_points(50)
    old = dict(X.image_points)
    X.set_image_views({'a': dict(width=8, height=8), 'b': dict(width=8, height=8, layers=('depth',))})
    fill_sentinel(old)
    ox, _, _, _ = X.step(acts[2])
    torch.cuda.synchronize()
    assert set(ox['views']['a']) == {'rgb'} and set(ox['views']['b']) == {'depth'} and all(is_sentinel(k, t) for k, t in old.items())
    for env in (X, Y):
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4: refusals

def test_every_refusal_names_its_cause():
    from roboticsplayroompybullet_amd._lib import RpPointsSpec
    n, w, h, pts = 2, 8, 8, 16
    env = make(U, n, 1)
    env.reset()
    dev = env.device
    depth, seg = torch.zeros((n, h, w), device=dev), torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    rgb = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=dev)
    xyz, count = torch.full((n, pts, 3), 7.0, device=dev), torch.full((n,), 7, dtype=torch.int32, device=dev)
    prgb = torch.zeros((n, pts, 3), dtype=torch.uint8, device=dev)
    good = RpPointsSpec(pts, 0, 0.0, 0)
    cam, cam_rows = env.camera(), env.cameras()

    def render(spec=good, cam=None, cam_rows=None, width=w, height=h, first=0, num=n, rgb=None, depth=depth, seg=seg, xyz=xyz, prgb=None, count=count):
        env._call('rp_render_points', C.byref(cam) if cam is not None else None, cam_rows.data_ptr() if cam_rows is not None else None, width, height, first, num,
                  C.byref(spec) if spec is not None else None,
                  *[t.data_ptr() if t is not None else None for t in (rgb, depth, seg, xyz, None, prgb, count)], env._stream())

    for match, kw in (('spec is NULL', dict(spec=None)), ('max_points', dict(spec=RpPointsSpec(0, 0, 0.0, 0))), ('max_points', dict(spec=RpPointsSpec(65537, 0, 0.0, 0))),
                      ('unknown frame', dict(spec=RpPointsSpec(pts, 2, 0.0, 0))), ('max_depth', dict(spec=RpPointsSpec(pts, 0, float('nan'), 0))),
                      ('depth and segmentation', dict(depth=None)), ('depth and segmentation', dict(seg=None)), ('xyz and count', dict(xyz=None, count=None)),
                      ('point_rgb needs the rgb', dict(prgb=prgb)), ('both cam and cam_rows', dict(cam=cam, cam_rows=cam_rows)), ('bad image size', dict(width=0)),
                      ('bad image size', dict(height=5000)), ('bad env range', dict(first=1, num=n)), ('bad env range', dict(num=0))):
        with pytest.raises(RuntimeError, match='rp_render_points: .*' + match):
            render(**kw)
    bad_cam = env.camera(fov=50.0)
    bad_cam.fov_deg = 180.0
    with pytest.raises(RuntimeError, match='rp_render_points: bad camera'):
        render(cam=bad_cam)
    torch.cuda.synchronize()
    assert bool((xyz == 7.0).all()) and bool((count == 7).all())          # no refused call wrote anything

    def attach(view=0, spec=good, xyz=xyz, prgb=None, count=count, fxyz=None, fprgb=None):
        env._call('rp_set_image_points', view, C.byref(spec) if spec is not None else None,
                  *[t.data_ptr() if t is not None else None for t in (xyz, None, prgb, count, fxyz, None, fprgb, None)])

    with pytest.raises(RuntimeError, match='rp_set_image_points: no image configuration is in force'):
        attach()
    env.set_image_obs(width=w, height=h, layers=('depth', 'segmentation'), depth='metres')
    for match, kw in (('view 1 lies outside 0 .. 0', dict(view=1)), ('view -1 lies outside', dict(view=-1)), ('max_points', dict(spec=RpPointsSpec(0, 0, 0.0, 0))),
                      ('xyz and count', dict(xyz=None, count=None)), ('point_rgb is given but the view has no rgb layer', dict(prgb=prgb)),
                      ('final_\\* output is given but the view has no final depth', dict(fxyz=xyz))):
        with pytest.raises(RuntimeError, match='rp_set_image_points: .*' + match):
            attach(**kw)
    env.set_image_obs(width=w, height=h, layers=('depth', 'segmentation'), depth='buffer')
    with pytest.raises(RuntimeError, match='rp_set_image_points: view 0: the view has no depth layer in RP_DEPTH_METRES'):
        attach()
    env.set_image_obs(width=w, height=h, layers=('segmentation',))
    with pytest.raises(RuntimeError, match='rp_set_image_points: view 0: the view has no depth layer in RP_DEPTH_METRES'):
        attach()
    env.set_image_obs(width=w, height=h, layers=('depth',), depth='metres')
    with pytest.raises(RuntimeError, match='rp_set_image_points: view 0: the view has no segmentation layer'):
        attach()
    env.set_image_views({'a': dict(width=w, height=h), 'b': dict(width=w, height=h, layers=('depth', 'segmentation'), depth='metres')})
    with pytest.raises(RuntimeError, match='rp_set_image_points: view 2 lies outside 0 .. 1'):
        attach(view=2)
    with pytest.raises(RuntimeError, match='rp_set_image_points: view 0: the view has no depth layer'):
        attach(view=0)
    attach(view=1)          # ... and the good one is taken, detached again by a NULL spec
    env.calc_state()
    torch.cuda.synchronize()
    assert not bool((count == 7).any())
    attach(view=1, spec=None)
    count.fill_(7)
    env.calc_state()
    torch.cuda.synchronize()
    assert bool((count == 7).all())
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="set_image_points: view 'a': points need"):
        env.set_image_points(16, view='a')
    with pytest.raises(ValueError, match="set_image_points: view is one of 'a', 'b'"):
        env.set_image_points(16)
    env.set_image_points(16, view='b')
    assert set(env.calc_state()['views']['b']) == {'depth', 'segmentation', 'points'}
    env.set_image_views(None)
    with pytest.raises(ValueError, match='set_image_points: no image configuration is in force'):
        env.set_image_points(16)
    for view, kw in ((dict(layers=('depth',)), {}), (dict(depth='buffer'), {}), ({}, dict(colour=True)), ({}, dict(drop=('tabel',)))):
        env.set_image_obs(**{'width': w, 'height': h, 'layers': ('depth', 'segmentation'), 'depth': 'metres', **view})
        with pytest.raises(ValueError, match='set_image_points: points'):
            env.set_image_points(16, **kw)
    with pytest.raises(ValueError, match="set_image_views: view 'b': points"):
        env.set_image_views({'a': dict(width=w, height=h), 'b': dict(width=w, height=h, points=dict(n=16))})
    env.close()
