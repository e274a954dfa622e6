"""rp_render_layers / VecPlayEnv.render_layers on the MI355X: the colour layer against rp_render bit for bit, the tile shortlist against the same kernel without it, depth
and segmentation against the numpy ray cast of tests/test_gpu_render.py over the oracle's collider poses and against rp_ray_test, the two depth modes against each other,
per-env cameras against the one-camera path, the ghost rule and the errors.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from camera_cases import cast, oracle_hulls, pixel_rays      # noqa: E402
from test_gpu_render import default_camera      # noqa: E402

pytestmark = pytest.mark.gpu
U, V, W2 = 'UR5PlayAbsRPY1Obj-v0', 'pandaPlayAbsRPY1Obj-v0', 'pandaPlay-v0'
SIZES = ((200, 200), (70, 45), (1, 1), (3, 130))          # (width, height): ragged tiles on both axes, a one-pixel image, a three-pixel-wide one
CAMERAS = ('default', 'wide', 'gripper', 'fov170', 'fov1', 'close', 'away')
LAYERS = ('rgb', 'depth', 'segmentation')


@pytest.fixture(scope='module')
def ur5():
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = VecPlayEnv(U, 3, seed=4)
    obs = env.reset()
    torch.cuda.synchronize()
    return env, obs


def make_camera(env, name):
    if name == 'default':
        return None
    if name == 'wide':
        return env.camera(distance=2.0, yaw=20.0, pitch=-40.0, fov=60.0, aspect=320 / 240)
    if name == 'gripper':
        return env.camera(gripper=True)          # its eye is inside the boxes around the last links
    blk = env.get_state()[0, 24:27].cpu().numpy().astype(float)
    edge = (blk + [0.0, -0.025, 0.025]).tolist()          # the block's upper front edge (10 x 5 x 5 cm)
    if name == 'fov170':
        return env.camera(target=edge, distance=0.6, fov=170.0)
    if name == 'fov1':
        return env.camera(target=edge, fov=1.0)
    if name == 'close':
        return env.camera(target=blk.tolist(), distance=0.09, yaw=40.0, pitch=-35.0)          # about 5 cm from the block's faces
    assert name == 'away'
    cam = env.camera()
    for k in range(3):          # the default eye, looking the other way: up and out of the scene
        cam.target[k] = 2.0 * cam.eye[k] - cam.target[k]
    return cam


def cull(env, on):
    assert env.lib.rp_debug_render_cull(env.h, int(on)) == 0


def both_ways(env, **kw):
    """render_layers with the tile shortlist and without it"""
    try:
        culled = {k: v.clone() for k, v in env.render_layers(**kw).items()}
        cull(env, False)
        plain = {k: v.clone() for k, v in env.render_layers(**kw).items()}
    finally:
        cull(env, True)
    return culled, plain


@pytest.mark.parametrize('name', CAMERAS)
def test_rgb_is_rp_renders_and_culling_is_exact(ur5, name):
    """checks 1 and 2: at every size the colour layer is rp_render's image byte for byte, and all three layers are bitwise the same with every record on every tile's list"""
    env, _ = ur5
    cam = make_camera(env, name)
    for w, h in SIZES:
        want = env.render('rgb_array', width=w, height=h, camera=cam)
        for depth in ('buffer', 'metres'):
            culled, plain = both_ways(env, width=w, height=h, camera=cam, depth=depth)
            assert culled['rgb'].shape == (3, h, w, 3) and culled['depth'].shape == (3, h, w) and culled['segmentation'].shape == (3, h, w)
            assert culled['depth'].dtype == torch.float32 and culled['segmentation'].dtype == torch.int32
            assert torch.equal(culled['rgb'], want), (name, w, h, int((culled['rgb'] != want).any(dim=3).sum()))
            for k in LAYERS:
                assert torch.equal(culled[k], plain[k]), (name, w, h, depth, k, int((culled[k] != plain[k]).sum()))
        if name == 'away':          # nothing but background: one colour, no collider, the far plane
            assert len(torch.unique(culled['rgb'].reshape(-1, 3), dim=0)) == 1
            assert bool((culled['segmentation'] == -1).all()) and bool((culled['depth'] == 10.0).all())
            assert bool((env.render_layers(width=w, height=h, camera=cam, layers=('depth',))['depth'] == 1.0).all())
        elif (w, h) == (200, 200):          # the other cameras see the scene
            assert bool((culled['segmentation'] >= 0).any()), name


def test_single_layers_env_ranges_and_preallocated_outputs(ur5):
    """envs=(1, 3) on the 3-env handle - slot and env indices differ -, each layer asked for alone, and out="""
    env, _ = ur5
    full = env.render_layers(width=70, height=45)
    part, plain = both_ways(env, width=70, height=45, envs=(1, 3))
    assert torch.equal(part['rgb'], env.render('rgb_array', width=70, height=45, envs=(1, 3)))
    for k in LAYERS:
        assert part[k].shape[0] == 2 and torch.equal(part[k], full[k][1:3]) and torch.equal(part[k], plain[k]), k
        alone = env.render_layers(width=70, height=45, layers=(k,))
        assert list(alone) == [k] and torch.equal(alone[k], full[k]), k
    assert list(env.render_layers(width=70, height=45, layers='depth')) == ['depth']
    buf = {'rgb': torch.zeros((3, 45, 70, 3), dtype=torch.uint8, device=env.device), 'segmentation': torch.zeros((3, 45, 70), dtype=torch.int32, device=env.device)}
    res = env.render_layers(width=70, height=45, out=buf)
    assert res['rgb'] is buf['rgb'] and res['segmentation'] is buf['segmentation'] and torch.equal(res['rgb'], full['rgb']) and torch.equal(res['depth'], full['depth'])
    with pytest.raises(AssertionError):
        env.render_layers(width=70, height=45, out={'depth': torch.zeros((3, 45, 70), dtype=torch.float64, device=env.device)})


def test_ghosts_rgb_is_rp_renders_and_culling_is_exact(ur5):
    """checks 1 and 2 with ghosts: a sub-goal (more than 64 records: two ballot rounds), a ghost arm on the Panda, the wide build"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    env, obs = ur5
    sg = obs['achieved_goal'].clone()
    sg[:, 0] += 0.12
    sg[:, 7] = -0.05
    cases = [(env, dict(sub_goal=sg))]
    panda = VecPlayEnv(V, 2, seed=3)
    pobs = panda.reset()
    ee = pobs['obs_quat'][:, 0:7]
    away = torch.cat([ee[:, 0:3] + torch.tensor([0.15, 0.0, 0.05], device=ee.device), ee[:, 3:7], torch.zeros((2, 1), device=ee.device)], 1)
    psg = pobs['achieved_goal'].clone()
    psg[:, 0] -= 0.1
    cases += [(panda, dict(ghost_arm=away)), (panda, dict(ghost_arm=away, sub_goal=psg))]
    wide = VecPlayEnv(W2, 1, seed=2)
    wobs = wide.reset()
    wsg = wobs['achieved_goal'].clone()
    wsg[:, 0] += 0.1
    cases += [(wide, dict()), (wide, dict(sub_goal=wsg))]
    for e, kw in cases:
        for w, h in ((200, 200), (70, 45)):
            want = e.render('rgb_array', width=w, height=h, **kw)
            culled, plain = both_ways(e, width=w, height=h, **kw)
            assert torch.equal(culled['rgb'], want), (e.env_id, sorted(kw), w, h)
            for k in LAYERS:
                assert torch.equal(culled[k], plain[k]), (e.env_id, sorted(kw), w, h, k)
            if kw:
                bare = e.render_layers(width=w, height=h)
                assert not torch.equal(bare['rgb'], culled['rgb'])          # the ghosts are drawn ...
                assert torch.equal(bare['depth'], culled['depth']) and torch.equal(bare['segmentation'], culled['segmentation'])      # ... and are no obstacles


def test_depth_and_segmentation_match_the_numpy_ray_cast(ur5):
    """check 3: seed 4, 200 x 200, the default camera, two envs - the setting of test_image_matches_the_numpy_ray_cast...  The segmentation agrees with the float64 cast over
    the oracle's colliders on at least 0.995 of the pixels (the cap that test has for silhouette pixels), and there the depth in metres is t (d . f) to 2e-4 m (rp_ray_test's
    2e-5 of a ray fraction times the 10 m ray).

    The case that sets the pace is pixel (43, 64): its ray grazes the button's globe (collider 45, a sphere of 3 cm) at |n . d| = 0.0064, where rc_ray_sphere's float32
    discriminant b b - 4 a c cancels to 1.5e-7 out of two terms near 6 and its hit parameter - what rp_render shades with - is 2.8e-4 m off.  The depth layer evaluates a
    sphere's hit parameter through the point of closest approach instead, which keeps that pixel within 1e-5 m; the worst pixels are printed."""
    from oracle import OracleEnv
    env, _ = ur5
    got = env.render_layers(envs=(0, 2), depth='metres')
    torch.cuda.synchronize()
    eye, target, up = default_camera()
    d, f = pixel_rays(eye, target, up, 50.0, 1.0, 200, 200)
    worst = []
    for e in range(2):
        o = OracleEnv('U', seed=4, env_index=e, f32=True)
        o.reset()
        R, p, tab = o.colliders()
        t, who, nrm = cast(R, p, tab, np.tile(eye, (len(d), 1)), d, 10.0, oracle_hulls(o))
        seg_want = np.where(who >= 0, who | ((tab[np.maximum(who, 0), 8].astype(int) + 1) << 24), -1)
        z_want = t * (d @ f)
        seg = got['segmentation'][e].cpu().numpy().ravel()
        z = got['depth'][e].cpu().numpy().ravel()
        agree = seg == seg_want
        print('env', e, 'segmentation agrees on', agree.mean(), 'hits', (who >= 0).mean(), 'colliders', len(np.unique(who)))
        assert agree.mean() >= 0.995, agree.mean()
        hit = agree & (who >= 0)
        err = np.where(hit, np.abs(z - np.where(hit, z_want, 0.0)), 0.0)
        print('env', e, 'max depth error', err.max(), 'pixels over 2e-4:', int((err > 2e-4).sum()), 'over 1e-4:', int((err > 1e-4).sum()), 'of', int(hit.sum()))
        for k in np.argsort(err)[-4:]:          # the worst pixels: where, which collider, and how flat the ray meets the surface
            print('   pixel', (int(k % 200), int(k // 200)), 'collider', who[k], 'depth', z[k], 'want', z_want[k], 'error', err[k], '|n . d|', abs(nrm[k] @ d[k]))
        worst.append(err.max())
        assert (z[agree & (who < 0)] == 10.0).all()
        assert (who >= 0).mean() > 0.5 and len(np.unique(who[who >= 0])) > 15
    assert max(worst) <= 2e-4, worst


def test_depth_and_segmentation_match_rp_ray_test():
    """check 4: one env, 70 x 45; every pixel's ray as a 10 m segment through rp_ray_test"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = VecPlayEnv(U, 1, seed=6)
    env.reset()
    w, h = 70, 45
    got = env.render_layers(width=w, height=h, depth='metres')
    cam = env.camera()
    eye32, target, up = (np.array(list(v), dtype=np.float64) for v in (cam.eye, cam.target, cam.up))          # the camera the kernel has, float32 values
    np.testing.assert_allclose(eye32, default_camera()[0], atol=1e-6)
    d, f = pixel_rays(eye32, target, up, 50.0, 1.0, w, h)
    frm = torch.tensor(np.tile(eye32, (1, w * h, 1)), dtype=torch.float32)
    to = torch.tensor((eye32 + 10.0 * d)[None], dtype=torch.float32)
    rt = env.ray_test(frm, to)
    torch.cuda.synchronize()
    collider, link = env.unpack_segmentation(got['segmentation'][0].reshape(-1))
    agree = ((collider == rt['collider'][0]) & (link == rt['link'][0])).cpu().numpy()
    print('agree', agree.mean())
    assert agree.mean() >= 0.995, agree.mean()
    hit = agree & (rt['collider'][0].cpu().numpy() >= 0)
    assert hit.mean() > 0.5
    z_want = rt['hit_fraction'][0].cpu().numpy().astype(np.float64) * 10.0 * (d @ f)
    z = got['depth'][0].cpu().numpy().ravel()
    print('max depth error', np.abs(z[hit] - z_want[hit]).max())
    np.testing.assert_allclose(z[hit], z_want[hit], rtol=0, atol=2e-4)


@pytest.mark.parametrize('near,far,distance', [(0.01, 10.0, 1.3), (0.1, 3.0, 3.0)])
def test_the_two_depth_modes_agree(ur5, near, far, distance):
    """check 5: z recovered from the buffer value, far near / (far - (far - near) b), is the metres layer to four float32 ulps of a value near 1 (4 * 2^-24 z^2 (far - near)
    / (far near)) plus 1e-6 relative; the same rays hit and miss.  With far = 3 and the camera 3 m from its target, part of the scene lies beyond far and clamps to 1.0."""
    env, _ = ur5
    cam = env.camera(distance=distance)
    kw = dict(width=120, height=90, camera=cam, near=near, far=far, layers=('depth', 'segmentation'))
    b = env.render_layers(depth='buffer', **kw)
    m = env.render_layers(depth='metres', **kw)
    assert torch.equal(b['segmentation'], m['segmentation'])
    hit = (m['segmentation'] >= 0).cpu().numpy()
    bv, z = b['depth'].cpu().numpy().astype(np.float64), m['depth'].cpu().numpy().astype(np.float64)
    n32, f32 = float(np.float32(near)), float(np.float32(far))
    assert (bv[~hit] == 1.0).all() and (z[~hit] == f32).all()
    assert hit.mean() > 0.3 and (bv >= 0.0).all() and (bv <= 1.0).all() and (z[hit] > 0).all()
    beyond = hit & (z >= f32)
    assert (bv[beyond] == 1.0).all()
    inside = hit & ~beyond
    z_back = f32 * n32 / (f32 - (f32 - n32) * bv[inside])
    tol = 4 * 2.0 ** -24 * z[inside] ** 2 * (f32 - n32) / (f32 * n32) + 1e-6 * z[inside]
    print('near', near, 'far', far, 'worst error / tolerance', (np.abs(z_back - z[inside]) / tol).max(), 'beyond far', beyond.sum(), 'inside', inside.sum())
    assert (np.abs(z_back - z[inside]) <= tol).all()
    assert inside.sum() > 100
    if far == 3.0:
        assert beyond.sum() > 100


def test_per_env_cameras(ur5):
    """check 6: three envs, three cameras() rows, each env against a one-env call with the same numbers through the host-built basis: the device-built basis may differ by an
    ulp of tan / sqrt, which moves fewer silhouette pixels than the 0.995 cap allows; depth within 1e-5 m where rgb and segmentation agree"""
    env, _ = ur5
    yaw, dist, fov = [-30.0, 20.0, 75.0], [1.3, 2.0, 0.8], [50.0, 60.0, 35.0]
    rows = env.cameras(yaw=yaw, distance=dist, fov=fov)
    assert rows.shape == (3, 11) and rows.dtype == torch.float32 and rows.is_cuda
    got, plain = both_ways(env, cameras=rows, depth='metres')
    for k in LAYERS:
        assert torch.equal(got[k], plain[k]), k
    for e in range(3):
        one = env.render_layers(envs=(e, e + 1), camera=env.camera(yaw=yaw[e], distance=dist[e], fov=fov[e]), depth='metres')
        same = ((got['rgb'][e] == one['rgb'][0]).all(dim=2) & (got['segmentation'][e] == one['segmentation'][0])).cpu().numpy()
        err = (got['depth'][e] - one['depth'][0]).abs().cpu().numpy()
        print('env', e, 'identical pixels', same.mean(), 'max depth difference there', err[same].max())
        assert same.mean() >= 0.995, (e, same.mean())
        assert (err[same] <= 1e-5).all(), (e, err[same].max())
        assert bool((got['segmentation'][e] >= 0).any())
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not torch.equal(got['rgb'][a], got['rgb'][b]) and not torch.equal(got['depth'][a], got['depth'][b])
    single = env.render_layers(envs=(1, 2), cameras=rows[1:2], depth='metres')
    for k in LAYERS:
        assert torch.equal(single[k][0], got[k][1]), k
    same_rows = env.cameras()          # all scalars: num_envs rows of the default camera
    assert same_rows.shape == (3, 11)
    dflt, byrow = env.render_layers(), env.render_layers(cameras=same_rows)
    assert ((dflt['rgb'] == byrow['rgb']).all(dim=3) & (dflt['segmentation'] == byrow['segmentation'])).float().mean() >= 0.995


def test_ghosts_tint_rgb_only(ur5):
    """check 7: a sub-goal that moves the ghost block 12 cm aside changes rgb exactly as it changes rp_render's image; depth and segmentation are bitwise unchanged"""
    env, obs = ur5
    sg = obs['achieved_goal'].clone()
    sg[:, 0] += 0.12
    bare, ghost = env.render_layers(), env.render_layers(sub_goal=sg)
    assert torch.equal(bare['rgb'], env.render('rgb_array')) and torch.equal(ghost['rgb'], env.render('rgb_array', sub_goal=sg))
    changed = (bare['rgb'] != ghost['rgb']).any(dim=3)
    assert 50 < int(changed[0].sum()) < 8000
    assert torch.equal(bare['depth'], ghost['depth']) and torch.equal(bare['segmentation'], ghost['segmentation'])
    m0, m1 = env.render_layers(depth='metres', layers=('depth',)), env.render_layers(depth='metres', layers=('depth',), sub_goal=sg)
    assert torch.equal(m0['depth'], m1['depth'])


def test_errors(ur5):
    """check 8: every RP_ERR_ARG / RP_ERR_UNSUPPORTED case at the C level, with its text, and the Python value errors"""
    env, _ = ur5
    w, h = 8, 8
    rgb = torch.zeros((3, h, w, 3), dtype=torch.uint8, device=env.device)
    dep = torch.zeros((3, h, w), dtype=torch.float32, device=env.device)
    seg = torch.zeros((3, h, w), dtype=torch.int32, device=env.device)
    rows = env.cameras()
    ghost = torch.zeros((3, 8), dtype=torch.float32, device=env.device)
    cam = env.camera()
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def call(cam=None, rows=None, near=0.01, far=10.0, mode=0, width=w, height=h, first=0, num=3, rgb=p(rgb), dep=p(dep), seg=p(seg), ghost=None):
        rc = env.lib.rp_render_layers(env.h, C.byref(cam) if cam is not None else None, rows, near, far, mode, width, height, first, num, rgb, dep, seg, None, ghost, None)
        return rc, env.lib.rp_last_error(env.h).decode()

    assert call()[0] == 0 and call(cam=cam)[0] == 0 and call(rows=p(rows), mode=1)[0] == 0 and call(rgb=None, seg=None)[0] == 0
    bad_cam = env.camera()
    bad_cam.fov_deg = 180.0
    for kw in (dict(rgb=None, dep=None, seg=None), dict(cam=cam, rows=p(rows)), dict(near=0.0), dict(near=-1.0), dict(far=0.01), dict(near=2.0, far=1.0), dict(mode=2),
               dict(mode=-1), dict(width=0), dict(height=0), dict(width=4097), dict(height=4097), dict(first=-1), dict(num=0), dict(first=1, num=3), dict(first=3, num=1),
               dict(cam=bad_cam)):
        rc, text = call(**kw)
        assert rc == -1 and text.startswith('rp_render_layers: '), (kw, rc, text)
    rc, text = call(ghost=p(ghost))
    assert rc == -3 and 'Panda only' in text
    torch.cuda.synchronize()
    assert env.render_layers(width=w, height=h)['rgb'].shape == (3, h, w, 3)          # the handle still works
    for kw in (dict(layers=()), dict(layers=('rgb', 'normals')), dict(depth='meters'), dict(camera=cam, cameras=rows), dict(near=0.0), dict(near=1.0, far=1.0),
               dict(cameras=rows[:2]), dict(cameras=rows.cpu()), dict(cameras=rows.double()), dict(envs=(0, 2), cameras=rows)):
        with pytest.raises(ValueError):
            env.render_layers(width=w, height=h, **kw)
    with pytest.raises(RuntimeError, match='Panda only'):
        env.render_layers(width=w, height=h, ghost_arm=ghost)
    with pytest.raises(RuntimeError, match='rp_render_layers'):
        env.render_layers(width=0, height=h)
    with pytest.raises(ValueError):
        env.cameras(fov=[50.0, 60.0, 180.0])
