"""obs['img'] (environments.py:21-30, 841-845), sub-goal ghosts (environments.py:606-690), the gripper camera (environments.py:33-49) and
batched rayTest (environments.py:720-743) on the MI355X against a numpy restatement of the same ray casts over the oracle's collider
poses.  Run with -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from camera_cases import BACKGROUND, LIGHT, cast, cast_hull, hull_planes, oracle_hulls      # noqa: E402, F401 (the numpy ray cast lives in tests/camera_cases.py now)

pytestmark = pytest.mark.gpu
U = 'UR5PlayAbsRPY1Obj-v0'


def reference_image(orc, cam_eye, cam_target, cam_up, fov, w, h, button_q, dial01):
    R, p, tab = orc.colliders()
    f = cam_target - cam_eye
    f /= np.linalg.norm(f)
    s = np.cross(f, cam_up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(0.5 * np.radians(fov))
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    nx = (2 * (px.ravel() + 0.5) / w - 1) * th
    ny = (1 - 2 * (py.ravel() + 0.5) / h) * th
    d = f + nx[:, None] * s + ny[:, None] * u
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(cam_eye, (w * h, 1))
    t, who, nrm = cast(R, p, tab, o, d, 10.0, oracle_hulls(orc))
    rgb = tab[:, 4:7].copy()
    for c in range(len(tab)):
        if tab[c, 7] == 1:
            rgb[c] = [1, 0, 0] if button_q < 0.025 else [1, 1, 1]
        if tab[c, 7] == 2:
            rgb[c] = [1, 0, 0] if dial01 < 0.5 else [1, 1, 1]
    k = 0.45 + 0.55 * np.maximum(0, nrm @ LIGHT)
    col = np.where((who >= 0)[:, None], rgb[np.maximum(who, 0)] * k[:, None], BACKGROUND)
    return np.floor(np.clip(col, 0, 1) * 255 + 0.5).astype(np.uint8).reshape(h, w, 3), who.reshape(h, w)


def default_camera():
    y, pt = np.radians(-30.0), np.radians(-30.0)
    # computeViewMatrixFromYawPitchRoll, upAxis 2: eye = target + Rz(yaw) Rx(pitch) (0, -d, 0), up = Rz(yaw) Rx(pitch) (0, 0, 1)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(pt), -np.sin(pt)], [0, np.sin(pt), np.cos(pt)]])
    target = np.array([0.0, 0.25, 0.0])
    return target + Rz @ Rx @ np.array([0, -1.3, 0]), target, Rz @ Rx @ np.array([0, 0, 1.0])


def test_default_camera_is_the_references():
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = VecPlayEnv(U, 1, seed=0)
    cam = env.camera()
    eye, target, up = default_camera()
    np.testing.assert_allclose(list(cam.eye), eye, atol=1e-6)
    np.testing.assert_allclose(list(cam.target), target, atol=1e-7)
    np.testing.assert_allclose(list(cam.up), up, atol=1e-6)
    assert abs(np.linalg.norm(eye - target) - 1.3) < 1e-12 and eye[2] == pytest.approx(0.65)       # 30 degrees above the target plane
    assert cam.fov_deg == 50.0 and cam.aspect == 1.0 and cam.mode == 0


def test_image_matches_the_numpy_ray_cast_and_toggles_recolour():
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    n = 3
    env = VecPlayEnv(U, n, seed=4)
    obs = env.reset()
    img = env.render('rgb_array')
    torch.cuda.synchronize()
    assert img.shape == (n, 200, 200, 3) and img.dtype == torch.uint8
    eye, target, up = default_camera()
    for e in range(n):
        o = OracleEnv('U', seed=4, env_index=e, f32=True)
        oo = o.reset()
        ref, who = reference_image(o, eye, target, up, 50.0, 200, 200, oo['obs_quat'][17], oo['obs_quat'][18])
        got = img[e].cpu().numpy()
        close = (np.abs(got.astype(int) - ref.astype(int)) <= 1).all(axis=2)
        assert close.mean() > 0.995, close.mean()                  # silhouette pixels may fall on the other side of an edge in fp32
        assert (who >= 0).mean() > 0.5                             # the scene fills the view
        assert len(np.unique(who)) > 15                            # table, cabinet, arm links, block, fixtures are all in it
    # toggles (environments.py:469-483): with the button up (q = 0.03) the globe is white, with the dial at 0 (dial01 = 0 < 0.5) the grill is
    # red; pressing the button (q < 0.025) turns the globe red, turning the dial past 1.1 rad turns the grill white
    s = env.get_state()
    s[0, 50 + 1] = 0.03
    s[0, 50 + 2] = 0.0
    env.set_state(s)
    before = env.render('rgb_array', envs=(0, 1))[0].cpu().numpy()
    s[0, 50 + 1] = 0.01
    s[0, 50 + 2] = 1.5
    env.set_state(s)
    img2 = env.render('rgb_array', envs=(0, 1))[0].cpu().numpy()
    o = OracleEnv('U', seed=4, env_index=0, f32=True)
    o.reset()
    st = o.get_state()
    st[2 * 12 + 26 + 1] = 0.01
    st[2 * 12 + 26 + 2] = 1.5
    o.set_state(st)
    ref2, who2 = reference_image(o, eye, target, up, 50.0, 200, 200, 0.01, (1.5 % 2) / 2.2)
    assert ((np.abs(img2.astype(int) - ref2.astype(int)) <= 1).all(axis=2)).mean() > 0.995
    globe, grill = who2 == 45, who2 == 42
    assert globe.sum() > 5 and grill.sum() > 5
    assert (before[globe][:, 1] > 100).all() and (img2[globe][:, 1] < 5).all()        # white -> red: green channel drops to 0
    assert (before[grill][:, 1] < 5).all() and (img2[grill][:, 1] > 100).all()        # red -> white


def test_arm_links_are_drawn_as_the_hulls_they_collide_as():
    """Round 5 (verdict item 5): an arm link in img is the convex hull of its collision mesh - not the box around it.  Rays aimed at the links' boxes: every ray that hits
    a link's hull in the numpy cast hits it on the device too (same parameter to 2e-5), and a good part of the rays that would hit the BOX go past the hull - the corners a
    box has and a rounded link has not."""
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    n, k = 2, 512
    env = VecPlayEnv(U, n, seed=12)
    env.reset()
    rng = np.random.default_rng(5)
    for e in range(n):
        o = OracleEnv('U', seed=12, env_index=e, f32=True)
        o.reset()
        R, p, tab = o.colliders()
        hulls = oracle_hulls(o)
        links = sorted(hulls)
        to = np.stack([p[links[i % len(links)]] + R[links[i % len(links)]] @ (tab[links[i % len(links)], 1:4] * rng.uniform(-1, 1, 3)) for i in range(k)])      # points inside the links' boxes
        frm = to + rng.normal(size=(k, 3)) * 0.4 + np.array([0, 0, 0.5])
        to = frm + (to - frm) * 1.5
        if e == 0:
            f_all, t_all = np.zeros((n, k, 3)), np.zeros((n, k, 3))
        f_all[e], t_all[e] = frm, to
    out = env.ray_test(torch.tensor(f_all, dtype=torch.float32), torch.tensor(t_all, dtype=torch.float32))
    torch.cuda.synchronize()
    box_only = hull_hits = 0
    for e in range(n):
        o = OracleEnv('U', seed=12, env_index=e, f32=True)
        o.reset()
        R, p, tab = o.colliders()
        hulls = oracle_hulls(o)
        f32, t32 = np.float32(f_all[e]).astype(np.float64), np.float32(t_all[e]).astype(np.float64)
        t_h, who_h, _ = cast(R, p, tab, f32, t32 - f32, 1.0, hulls)
        t_b, who_b, _ = cast(R, p, tab, f32, t32 - f32, 1.0)
        got_c, got_t = out['collider'][e].cpu().numpy(), out['hit_fraction'][e].cpu().numpy()
        agree = got_c == who_h
        assert agree.mean() > 0.97, agree.mean()
        on_arm = agree & np.isin(who_h, list(hulls))
        np.testing.assert_allclose(got_t[on_arm], t_h[on_arm], atol=2e-5)
        hull_hits += int(on_arm.sum())
        box_only += int((np.isin(who_b, list(hulls)) & (who_b != who_h)).sum())
    assert hull_hits > 200 and box_only > 30, (hull_hits, box_only)


def test_rays_that_start_inside_a_links_box_but_outside_its_hull():
    """the box around a hull is a cull, not the collider - a ray whose origin lies inside a link's box (much larger than the rounded link) but outside the hull
    must still hit the hull straight ahead (the gripper camera at the EE link, rays cast from beside the arm).  Origins sampled in the links' boxes, kept where the numpy
    planes say "outside this hull", aimed through the hull's middle: the device agrees with the numpy polytope cast (same collider, same parameter to 2e-5)."""
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    n, k = 2, 256
    env = VecPlayEnv(U, n, seed=12)
    env.reset()
    rng = np.random.default_rng(9)
    f_all, t_all = np.zeros((n, k, 3)), np.zeros((n, k, 3))
    keep = []
    for e in range(n):
        o = OracleEnv('U', seed=12, env_index=e, f32=True)
        o.reset()
        R, p, tab = o.colliders()
        hulls = oracle_hulls(o)
        links = sorted(hulls)
        frm, to = [], []
        while len(frm) < k:
            c = links[int(rng.integers(len(links)))]
            x = p[c] + R[c] @ (tab[c, 1:4] * rng.uniform(-0.98, 0.98, 3))      # inside the link's box
            nn, w = hulls[c]
            if (x @ nn.T + w).max() < 2e-3:                                     # ... and inside (or within 2 mm of) its hull: not a case
                continue
            ctr = o.hull_vertices(c).mean(axis=0)
            frm.append(x); to.append(x + (ctr - x) * 3.0)
        f_all[e], t_all[e] = np.array(frm), np.array(to)
    out = env.ray_test(torch.tensor(f_all, dtype=torch.float32), torch.tensor(t_all, dtype=torch.float32))
    torch.cuda.synchronize()
    hits = 0
    for e in range(n):
        o = OracleEnv('U', seed=12, env_index=e, f32=True)
        o.reset()
        R, p, tab = o.colliders()
        hulls = oracle_hulls(o)
        f32, t32 = np.float32(f_all[e]).astype(np.float64), np.float32(t_all[e]).astype(np.float64)
        t_h, who_h, _ = cast(R, p, tab, f32, t32 - f32, 1.0, hulls)
        got_c, got_t = out['collider'][e].cpu().numpy(), out['hit_fraction'][e].cpu().numpy()
        agree = got_c == who_h
        assert agree.mean() > 0.97, (agree.mean(), got_c[~agree][:8], who_h[~agree][:8])
        on_arm = agree & np.isin(who_h, list(hulls))
        np.testing.assert_allclose(got_t[on_arm], t_h[on_arm], atol=2e-5)
        hits += int(on_arm.sum())
    assert hits > 0.8 * n * k, hits      # nearly every such ray hits a hull (before the fix: a miss whenever the origin was inside that link's box)


def test_sub_goal_ghosts_and_other_cameras():
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = VecPlayEnv(U, 2, seed=5)
    obs = env.reset()
    plain = env.render('rgb_array').cpu().numpy()
    sg = obs['achieved_goal'].clone()
    sg[:, 0] += 0.12                 # the ghost block 12 cm to the side
    sg[:, 7] = -0.05                 # and the ghost drawer pulled out
    ghost = env.render('rgb_array', sub_goal=sg).cpu().numpy()
    changed = (plain != ghost).any(axis=3)
    assert 50 < changed[0].sum() < 8000                           # something was drawn, the picture is not a different one
    same_goal = env.render('rgb_array', sub_goal=obs['achieved_goal']).cpu().numpy()
    assert (same_goal != plain).any(axis=3).mean() < 0.2          # ghosts on top of their bodies change the shade of those pixels only
    # ghosts are not obstacles: rays see the same world with or without them (rp_ray_test never takes a sub-goal)
    wide = env.render('rgb_array', width=320, height=240, camera=env.camera(distance=2.0, yaw=20.0, pitch=-40.0, fov=60.0, aspect=320 / 240))
    assert wide.shape == (2, 240, 320, 3)
    # the gripper camera against the reference's formula (camera_cases.gripper_basis) over the oracle's colliders - until the camera cases this asserted "more than three
    # colours", which a camera looking the wrong way passes; tests/test_gpu_camera_cases.py holds it at other EE orientations and on the Panda
    import camera_cases as cc
    from oracle import OracleEnv
    gcam = env.camera(gripper=True)
    grip = env.render('rgb_array', camera=gcam).cpu().numpy()
    assert grip.shape == (2, 200, 200, 3)
    for e in range(2):
        o = OracleEnv('U', seed=5, env_index=e, f32=True)
        o.reset()
        ref = cc.reference_layers(o, cc.camera_values(gcam), 200, 200)
        close = (np.abs(grip[e].astype(int) - cc.to_bytes(ref['rgb']).astype(int)) <= 1).all(axis=2)
        assert close.mean() >= 0.995, (e, close.mean())
        assert (ref['who'] >= 0).mean() > 0.01 and len(np.unique(ref['who'])) > 2          # it sees the arm's own wrist from the reset pose
    with pytest.raises(RuntimeError, match='rp_render'):
        env.render('rgb_array', width=0)


def test_batched_ray_test_against_the_numpy_ray_cast():
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd import VecPlayEnv
    n, k = 3, 64
    env = VecPlayEnv(U, n, seed=6)
    env.reset()
    rng = np.random.default_rng(0)
    frm = np.concatenate([rng.uniform(-0.4, 0.4, (n, k, 2)), rng.uniform(0.3, 0.6, (n, k, 1))], axis=2)
    to = np.concatenate([rng.uniform(-0.4, 0.5, (n, k, 2)), rng.uniform(-0.3, 0.0, (n, k, 1))], axis=2)
    out = env.ray_test(torch.tensor(frm, dtype=torch.float32), torch.tensor(to, dtype=torch.float32))
    torch.cuda.synchronize()
    hits = 0
    for e in range(n):
        o = OracleEnv('U', seed=6, env_index=e, f32=True)
        o.reset()
        R, p, tab = o.colliders()
        f32 = np.float32(frm[e]).astype(np.float64)
        t32 = np.float32(to[e]).astype(np.float64)
        t, who, nrm = cast(R, p, tab, f32, t32 - f32, 1.0, oracle_hulls(o))      # (rp_ray_test sees the arm's links as the hulls they collide as)
        got_t = out['hit_fraction'][e].cpu().numpy()
        got_c = out['collider'][e].cpu().numpy()
        want_t = np.where(who >= 0, t, 1.0)
        agree = got_c == who
        assert agree.mean() > 0.95                                 # a ray grazing an edge may go either way in fp32
        np.testing.assert_allclose(got_t[agree], want_t[agree], atol=2e-5)
        hp = out['hit_position'][e].cpu().numpy()
        np.testing.assert_allclose(hp[agree & (who >= 0)], (f32 + (t32 - f32) * t[:, None])[agree & (who >= 0)], atol=3e-5)
        np.testing.assert_allclose(out['hit_normal'][e].cpu().numpy()[agree & (who >= 0)], nrm[agree & (who >= 0)], atol=2e-3)      # (a hull facet's normal: baked in fp32, coplanar facets merged to 1e-5)
        link = out['link'][e].cpu().numpy()
        assert (link[who >= 0] == tab[who[who >= 0], 8].astype(int))[agree[who >= 0]].all()
        hits += int((who >= 0).sum())
    assert hits > n * k // 2
    # a vertical ray onto the block: hit at its top face
    blk = env.get_state()[:, 24:27].cpu().numpy()
    f = torch.tensor(blk + [0, 0, 0.3], dtype=torch.float32)[:, None, :]
    t = torch.tensor(blk - [0, 0, 0.1], dtype=torch.float32)[:, None, :]
    o2 = env.ray_test(f, t)
    assert (o2['collider'][:, 0].cpu().numpy() == 51).all()
    np.testing.assert_allclose(o2['hit_position'][:, 0, 2].cpu().numpy(), blk[:, 2] + 0.025, atol=1e-4)
    np.testing.assert_allclose(o2['hit_normal'][:, 0].cpu().numpy(), np.tile([0, 0, 1.0], (n, 1)), atol=1e-3)


def test_single_env_adapter_records_images():
    import roboticsplayroompybullet_amd as rp
    env = rp.make(U, seed=1)
    o = env.reset()
    assert o['img'] is None                                      # like the reference: no image until render('rgb_array')
    assert env.render('rgb_array') is None                       # environments.py:200-201: sets instance.record_images, returns nothing
    o, r, d, info = env.step(np.array([0.0, 0.2, 0.15, 0, 0, 0, 0.0]))
    assert o['img'].shape == (200, 200, 3) and o['img'].dtype == np.uint8 and len(np.unique(o['img'].reshape(-1, 3), axis=0)) > 10
    plain = o['img']
    sg = o['achieved_goal'].copy()
    sg[1] -= 0.15
    env.visualise_sub_goal(sg, sub_goal_state='achieved_goal')
    o2 = env.instance.calc_state()
    assert (o2['img'] != plain).any()
    env.delete_sub_goal()
    o3 = env.instance.calc_state()
    assert (o3['img'] == plain).all()
    with pytest.raises(NotImplementedError):
        env.visualise_sub_goal(o['controllable_achieved_goal'], sub_goal_state='controllable_achieved_goal')
    env.close()


def test_panda_ghost_arm_of_visualise_sub_goal():
    """visualise_sub_goal(sub_goal, 'controllable_achieved_goal' / 'full_positional_state') (environments.py:606-637, 671-674): a second, half-transparent Panda at the joints
    one default IK call from the rest pose finds for the sub-goal's EE pose (reset_arm, environments.py:575-590).  The ghost is drawn (pixels change), it is not an obstacle
    (rays do not see it), a ghost at the arm's own EE pose tints the arm's pixels - another set than the ghost beside it -, and the UR5 is refused as in the reference (NotImplementedError upstream,
    RP_ERR_UNSUPPORTED at the C ABI)."""
    import roboticsplayroompybullet_amd as rp
    from roboticsplayroompybullet_amd import VecPlayEnv
    V = 'pandaPlayAbsRPY1Obj-v0'
    env = VecPlayEnv(V, 2, seed=3)
    obs = env.reset()
    plain = env.render('rgb_array').cpu().numpy()
    ee = obs['obs_quat'][:, 0:7].clone()                              # EE position and orientation
    away = torch.cat([ee[:, 0:3] + torch.tensor([0.15, 0.0, 0.05], device=ee.device), ee[:, 3:7], torch.zeros((2, 1), device=ee.device)], 1)
    ghost = env.render('rgb_array', ghost_arm=away).cpu().numpy()
    changed = (plain != ghost).any(axis=3)
    assert 200 < changed[0].sum() < 15000, changed[0].sum()        # a second arm appeared, the picture is otherwise the same
    # the ghost's joints against the oracle's reset_arm arithmetic (round 6: until now only pixels were counted): the rest pose, ONE inverse-kinematics call of 20 iterations
    # towards the pose, joints [0:6] taken, the seventh keeps its rest value (environments.py:575-593)
    import ctypes as C
    from oracle import OracleEnv
    gq = (C.c_float * 16)()
    assert env.lib.rp_debug_ghost_joints(env.h, gq, 2) == 0
    gq = np.frombuffer(gq, dtype=np.float32).reshape(2, 8)
    for e in range(2):
        o = OracleEnv('V', seed=3, env_index=e, f32=True)
        o.reset()
        rest = o.rest_pose()
        a = away[e].cpu().numpy().astype(np.float64)
        sol = o.ik(a[0:3], a[3:7], rest, max_iter=20)
        want = np.concatenate([sol[:6], rest[6:7]])
        np.testing.assert_allclose(gq[e, :7], want, atol=2e-4)
    same = torch.cat([ee, torch.zeros((2, 1), device=ee.device)], 1)
    on_top = (env.render('rgb_array', ghost_arm=same).cpu().numpy() != plain).any(axis=3)
    assert 200 < on_top[0].sum() < 15000 and (on_top[0] != changed[0]).sum() > 500      # (the tinted ghost over the arm itself: other pixels than the ghost 15 cm away)
    ur5 = VecPlayEnv(U, 1, seed=3)
    ur5.reset()
    with pytest.raises(RuntimeError, match='Panda only'):
        ur5.render('rgb_array', ghost_arm=torch.zeros((1, 8)))
    single = rp.make(V, seed=1)
    o = single.reset()
    single.render('rgb_array')
    o, r, d, info = single.step(np.array([0.0, 0.1, 0.1, 0, 0, 0, 0.0]))
    before = o['img']
    sg = o['full_positional_state'].copy()
    sg[0] += 0.12
    single.visualise_sub_goal(sg, sub_goal_state='full_positional_state')
    with_ghost = single.instance.calc_state()['img']
    assert 100 < (with_ghost != before).any(axis=2).sum()
    single.delete_sub_goal()
    assert (single.instance.calc_state()['img'] == before).all()
    single.close()


def test_rp_render_bits_of_the_parent(golden):
    """VecPlayEnv.render (rp_render, rp_render_ex) draws through k_render_layers since the 256-pixel-run kernel it had was retired: every image of
    tools/render_goldens.py's cases - the cameras and sizes of tests/test_gpu_render_layers.py, after reset() and after five random steps, an env range, the ghosts on
    the UR5, the Panda and the wide build - keeps the bytes that kernel wrote at the commit the file names.  The state's checksum tells a scene that differs (not this
    test's subject) from a picture that does."""
    import render_goldens as g
    gold = golden('render_parent_checksums.json')
    assert (gold['steps'], gold['action_seed']) == (g.STEPS, g.ACTION_SEED) and len(gold['commit']) == 40
    got = g.run()
    assert [c['case'] for c in got] == gold['cases']
    for c in got:
        want = gold['sha256'][c['case']]
        assert c['state'] == want['state'], '%s: get_state() differs from commit %s: another scene, whatever the picture' % (c['case'], gold['commit'][:7])
        assert c['image'] == want['image'], '%s: the image differs from the one commit %s drew of the same state' % (c['case'], gold['commit'][:7])
