"""Per-env colours, light and background (rp_set_visuals) on the MI355X against the float64 ray cast of tests/visual_cases.py over the oracle's collider poses, at N = 3
and the sizes 70 x 45 and 33 x 50: the default rows against the constants the kernels draw with while there is no table, three rows that differ in every part - a light
from below, one of no unit length, one that saturates -, the toggles on top of the table, mask / broadcast / read-back, an env range, ghosts, the calls that move state
and must leave the rows alone, the unculled kernel and obs['img'].  The states are the oracle's, carried over as tests/test_gpu_camera_cases.py carries them.  Run with
-m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytest.importorskip('scipy')

import camera_cases as cc      # noqa: E402
import visual_cases as vc      # noqa: E402

pytestmark = pytest.mark.gpu
N = cc.NUM_ENVS
SIZES = cc.SIZES          # (70, 45), (33, 50)
_HANDLES = {}


def fresh(gid, **kw):
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = VecPlayEnv(gid, N, seed=cc.SEEDS[gid], **kw)
    env.reset()
    torch.cuda.synchronize()
    return env


def put(gid, state):
    """one handle per id for the whole module with every env in the state: the oracle's numbers through record_from_oracle + set_state (the wide id stays as reset()
    left it: env e = the oracle with env_index e).  The handle keeps whatever visuals the test before left: every test sets its own."""
    from gpu_debug import record_from_oracle
    if gid not in _HANDLES:
        _HANDLES[gid] = fresh(gid)
    env = _HANDLES[gid]
    if gid != cc.W2:
        env.set_state(torch.tensor(np.tile(record_from_oracle(cc.oracle_of(gid, state)), (N, 1))))
    return env


def set_rows(env, v):
    """the rows of visual_cases.random_visuals: colour and background as host arrays (checked), the light as a device tensor (used as it stands).  Returns what
    get_visuals reads back, as numpy: the float32 values the device holds"""
    env.set_visuals(colour=v['colour'], background=v['background'], light=torch.tensor(v['light']).to(env.device))
    return read(env)


def set_defaults(env, o):
    env.set_visuals(colour=vc.table_colours(o).astype(np.float32), light=torch.tensor(vc.DEVICE_LIGHT).to(env.device), background=vc.DEVICE_BACKGROUND)


def read(env):
    return {k: t.cpu().numpy() for k, t in env.get_visuals().items()}


def same_bits(a, b):
    return all(np.asarray(a[k], dtype=np.float32).tobytes() == np.asarray(b[k], dtype=np.float32).tobytes() for k in ('colour', 'light', 'background'))


def one_env(layers, e):
    return {k: v[e].cpu().numpy() for k, v in layers.items()}


def hold(label, rgb, seg, ref):
    """the hold rule of the camera tests for the colour layer: the segmentation agrees on at least cc.SEG_CAP of the pixels and on those rgb is within 1 count.  Without
    a segmentation (render()): rgb within 1 count on at least cc.SEG_CAP of the pixels, the ghost tests' rule.  Returns the pixels held."""
    want = cc.to_bytes(ref['rgb']).astype(int)
    cerr = np.abs(rgb.astype(int) - want).max(axis=2)
    if seg is None:
        close = cerr <= 1
        print(label, 'rgb within 1 count on %.5f' % close.mean(), 'tinted pixels', int(ref['tint'].sum()))
        assert close.mean() >= cc.SEG_CAP, (label, close.mean())
        return close
    agree = seg == ref['seg']
    worst = np.where(agree, cerr, 0)
    print(label, 'segmentation agrees on %.5f' % agree.mean(), 'hits %.3f' % (ref['who'] >= 0).mean(), 'max colour error', worst.max(), 'pixels over 1 count: %d' % (worst > 1).sum())
    for k in np.argsort(worst.ravel())[-2:]:
        y, x = divmod(int(k), seg.shape[1])
        print('   colour pixel', (x, y), 'collider', ref['who'][y, x], 'rgb', rgb[y, x], 'want', want[y, x])
    assert agree.mean() >= cc.SEG_CAP, (label, agree.mean())
    assert worst.max() <= 1, (label, worst.max(), int((worst > 1).sum()))
    return agree


def layers_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('gid', cc.IDS)
def test_defaults_are_the_constants(gid):
    """1: a fresh handle reads back the oracle collider table's rgb, the light (0.2672612, -0.5345225, 0.8017837, 0.45, 0.55) and the background (0.82, 0.88, 0.96);
    the three layers drawn before any set or get (no table: the kernels' constants) are byte for byte those drawn after set_visuals(**get_visuals()) (the table's
    path), at both sizes, through render() too, and on U with a sub-goal's ghosts"""
    env, o = fresh(gid), cc.oracle_of(gid, 'reset')
    sub_goal = torch.tensor(np.tile(cc.sub_goal_vector(gid, o, cc.GHOST_COMBINED[gid]), (N, 1)), dtype=torch.float32) if gid == cc.U else None
    draw = lambda: [env.render_layers(width=w, height=h, sub_goal=sg) for w, h in SIZES for sg in ((None, sub_goal) if sub_goal is not None else (None,))] + \
        [{'rgb': env.render(width=w, height=h)} for w, h in SIZES]      # noqa: E731
    before = draw()
    v = env.get_visuals()
    got = {k: t.cpu().numpy() for k, t in v.items()}
    assert got['colour'].shape == (N, len(env.visual_names), 3) and got['light'].shape == (N, 5) and got['background'].shape == (N, 3)
    for e in range(N):
        assert got['colour'][e].tobytes() == o.colliders()[2][:, 4:7].astype(np.float32).tobytes()
        assert got['light'][e].tobytes() == vc.DEVICE_LIGHT.tobytes() and got['background'][e].tobytes() == vc.DEVICE_BACKGROUND.tobytes()
    with_table = draw()          # the table exists now, with the default rows
    env.set_visuals(**v)
    written_back = draw()
    for a, b, c in zip(before, with_table, written_back):
        assert layers_equal(a, b) and layers_equal(a, c)
    assert same_bits(read(env), got)
    assert len(torch.unique(before[0]['rgb'].reshape(-1, 3), dim=0)) > 6
    env.close()


@pytest.mark.parametrize('gid,state', [(cc.U, 'scene'), (cc.V, 'arm')])
def test_rows_match_the_float64_ray_cast(gid, state):
    """2: three rows that differ in every part, per-env cameras ('rows') at 70 x 45, each env against reference_rgb with its own row and camera.  Depth and
    segmentation are byte for byte those of the default visuals; pixels of the toggle colliders are red or white by the state, not the table's colour."""
    env, o = put(gid, state), cc.oracle_of(gid, state)
    w, h = SIZES[0]
    rows = env.cameras(**cc.ROWS)
    set_defaults(env, o)
    plain = env.render_layers(width=w, height=h, cameras=rows)
    given = vc.random_visuals(N, len(env.visual_names), 11)
    env.set_visuals(colour=given['colour'], background=given['background'])
    env.set_visuals(light=given['light'][[0, 2]][[0, 0, 1]], mask=[1, 0, 1])                                     # host values: normalised (both are of unit length already)
    env.set_visuals(light=torch.tensor(given['light']).to(env.device), mask=torch.tensor([0, 1, 0]))             # a device tensor: as it stands
    v = read(env)
    assert v['light'][1].tobytes() == given['light'][1].tobytes() and abs(np.linalg.norm(v['light'][1, :3].astype(np.float64)) - 1.0) > 0.5
    assert v['light'][0].tobytes() == given['light'][0].tobytes()
    np.testing.assert_allclose(v['light'][2], given['light'][2], rtol=0, atol=1.2e-7)
    assert v['colour'].tobytes() == given['colour'].tobytes() and v['background'].tobytes() == given['background'].tobytes()
    got = env.render_layers(width=w, height=h, cameras=rows)
    assert torch.equal(got['depth'], plain['depth']) and torch.equal(got['segmentation'], plain['segmentation'])
    assert not torch.equal(got['rgb'], plain['rgb'])
    toggles, shown, toggle_pixels = vc.toggle_colliders(o), cc.collider_colours(o, o.colliders()[2]), 0
    for e in range(N):
        mine = one_env(got, e)
        ref = vc.reference_rgb(o, cc.camera_values(rows[e].cpu().numpy()), w, h, v['colour'][e], v['light'][e], v['background'][e])
        held = hold('%s %s env %d' % (gid, state, e), mine['rgb'], mine['segmentation'], ref)
        for c in toggles:
            px = mine['rgb'][held & (ref['who'] == c)].astype(int)
            toggle_pixels += len(px)
            if shown[c][1] == 0:          # red: the green and blue bytes are 0 whatever the light
                assert (px[:, 1:] == 0).all() and (px[:, 0] > 0).all(), (e, c)
            else:                         # white: three equal bytes
                assert (px[:, 0] == px[:, 1]).all() and (px[:, 1] == px[:, 2]).all(), (e, c)
        sat = held & (ref['who'] >= 0)
        print('   env', e, 'saturated bytes', int((mine['rgb'][sat] == 255).sum()), 'toggle pixels so far', toggle_pixels)
    assert toggle_pixels > 0
    assert (one_env(got, 2)['rgb'] == 255).any()          # ambient 0.7 + diffuse 0.6: the clamp is exercised


def test_mask_broadcast_and_read_back():
    """3: one row broadcast under a mask of env 1: get_visuals has that row bit for bit in env 1 and the old rows in envs 0 and 2, whose images keep their bytes; env 1
    meets the reference; a None part leaves that part alone"""
    from roboticsplayroompybullet_amd.vec_env import check_visual_values
    env, o = put(cc.U, 'scene'), cc.oracle_of(cc.U, 'scene')
    w, h = SIZES[1]
    old = set_rows(env, vc.random_visuals(N, len(env.visual_names), 5))
    before = env.render_layers(width=w, height=h)
    row = {k: a[0] for k, a in vc.random_visuals(1, len(env.visual_names), 6).items()}
    row['light'] = np.array([2.0, 1.0, 2.0, 0.3, 0.6], dtype=np.float32)
    env.set_visuals(mask=[0, 1, 0], **row)
    want = dict(row, light=check_visual_values('light', row['light']).numpy())
    assert np.abs(want['light'][:3].astype(np.float64) - [2 / 3, 1 / 3, 2 / 3]).max() <= 8e-8          # normalised on the host
    v = read(env)
    assert same_bits({k: a[1] for k, a in v.items()}, want)
    assert same_bits({k: a[[0, 2]] for k, a in v.items()}, {k: a[[0, 2]] for k, a in old.items()})
    after = env.render_layers(width=w, height=h)
    assert layers_equal({k: t[[0, 2]] for k, t in after.items()}, {k: t[[0, 2]] for k, t in before.items()})
    assert torch.equal(after['depth'], before['depth']) and not torch.equal(after['rgb'][1], before['rgb'][1])
    mine = one_env(after, 1)
    hold('masked env 1', mine['rgb'], mine['segmentation'], vc.reference_rgb(o, cc.camera_values(env.camera()), w, h, v['colour'][1], v['light'][1], v['background'][1]))
    env.set_visuals(background=[0.25, 0.5, 0.75])          # colour and light None: left as they are
    v2 = read(env)
    assert v2['colour'].tobytes() == v['colour'].tobytes() and v2['light'].tobytes() == v['light'].tobytes()
    assert (v2['background'] == np.array([0.25, 0.5, 0.75], dtype=np.float32)).all()
    env.set_visuals(colour=old['colour'][2], mask=torch.tensor([1, 0, 0], dtype=torch.uint8))          # ... and the other way round
    v3 = read(env)
    assert v3['colour'][0].tobytes() == old['colour'][2].tobytes() and v3['colour'][1:].tobytes() == v2['colour'][1:].tobytes()
    assert v3['light'].tobytes() == v2['light'].tobytes() and v3['background'].tobytes() == v2['background'].tobytes()
    with pytest.raises(ValueError):
        env.set_visuals()
    with pytest.raises(ValueError):
        env.set_visuals(colour=np.zeros((N, 3, 3)))
    with pytest.raises(KeyError, match='drawer'):
        env.set_colour('no such thing', [1, 0, 0])
    env.set_colour('drawer', [0.0, 1.0, 0.5], mask=[0, 0, 1])
    v4 = read(env)
    drawer = [c for c, nm in enumerate(env.visual_names) if nm == 'drawer']
    assert len(drawer) > 1 and (v4['colour'][2][drawer] == np.array([0.0, 1.0, 0.5], dtype=np.float32)).all()
    rest = [c for c in range(len(env.visual_names)) if c not in drawer]
    assert v4['colour'][2][rest].tobytes() == v3['colour'][2][rest].tobytes() and v4['colour'][:2].tobytes() == v3['colour'][:2].tobytes()


def test_the_default_light_as_host_values_draws_the_default_image():
    """the default light written as its formula, light=(1, -2, 3, 0.45, 0.55) from the host, is the default row bit for bit, so the image keeps its bytes"""
    env, o = put(cc.U, 'scene'), cc.oracle_of(cc.U, 'scene')
    w, h = SIZES[0]
    set_defaults(env, o)
    plain = env.render(width=w, height=h).clone()
    env.set_visuals(light=[0.0, 1.0, 0.0, 0.2, 0.9])
    assert not torch.equal(env.render(width=w, height=h), plain)
    env.set_visuals(light=[1.0, -2.0, 3.0, 0.45, 0.55])
    assert all(row.tobytes() == vc.DEVICE_LIGHT.tobytes() for row in read(env)['light'])
    assert torch.equal(env.render(width=w, height=h), plain)


def test_an_env_range_reads_its_own_rows():
    """4: with three different rows set, render_layers(envs=(1, 3)) and render(envs=(1, 3)) are rows 1 .. 2 of the full-batch images byte for byte"""
    env = put(cc.V, 'arm')
    set_rows(env, vc.random_visuals(N, len(env.visual_names), 21))
    for w, h in SIZES:
        full = env.render_layers(width=w, height=h)
        part = env.render_layers(width=w, height=h, envs=(1, 3))
        assert layers_equal(part, {k: t[1:3] for k, t in full.items()})
        assert torch.equal(env.render(width=w, height=h, envs=(1, 3)), full['rgb'][1:3])
        assert torch.equal(env.render(width=w, height=h, envs=(2, 3)), full['rgb'][2:3])
        assert not torch.equal(full['rgb'][1], full['rgb'][2]) and not torch.equal(full['rgb'][0], full['rgb'][1])          # same state, other rows


@pytest.mark.parametrize('gid,arm', [(cc.U, False), (cc.V, True)])
def test_ghosts_take_their_envs_colours(gid, arm):
    """5: U's combined sub-goal and the Panda's ghost arm with random rows set: rgb within 1 count of reference_rgb(..., ghosts=...) on at least cc.SEG_CAP of the
    pixels, per env with its own row; the ghosts show in neither depth nor segmentation"""
    env, o = put(gid, 'reset'), cc.oracle_of(gid, 'reset')
    w, h = SIZES[0]
    v = set_rows(env, vc.random_visuals(N, len(env.visual_names), 31))
    if arm:
        pose = cc.ghost_arm_pose(o)
        kw = dict(ghost_arm=torch.tensor(np.tile(pose, (N, 1)), dtype=torch.float32))
        ghosts = [cc.ghost_records(cc.ghost_arm_oracle(gid, o, pose), arm=True)]
    else:
        sub_goal = cc.sub_goal_vector(gid, o, cc.GHOST_COMBINED[gid])
        kw = dict(sub_goal=torch.tensor(np.tile(sub_goal, (N, 1)), dtype=torch.float32))
        ghosts = [cc.ghost_records(cc.sub_goal_oracle(gid, o, sub_goal))]
    bare = env.render_layers(width=w, height=h)
    got = env.render_layers(width=w, height=h, **kw)
    assert torch.equal(got['depth'], bare['depth']) and torch.equal(got['segmentation'], bare['segmentation'])
    assert torch.equal(env.render(width=w, height=h, **kw), got['rgb'])
    cam = cc.camera_values(env.camera())
    for e in range(N):
        ref = vc.reference_rgb(o, cam, w, h, v['colour'][e], v['light'][e], v['background'][e], ghosts=ghosts)
        assert ref['tint'].sum() > 4
        hold('%s ghosts env %d' % (gid, e), got['rgb'][e].cpu().numpy(), None, ref)
        changed = (got['rgb'][e] != bare['rgb'][e]).any(dim=2).cpu().numpy()
        assert changed.sum() > 0


def test_visuals_are_parameters_not_state():
    """6: reset(), set_state() of another handle's rows, clone_envs with a permutation and an autoreset step that ends an env all leave get_visuals bit for bit what was
    set; a cloned env draws with its own row"""
    env = put(cc.U, 'reset')
    w, h = SIZES[1]
    want = set_rows(env, vc.random_visuals(N, len(env.visual_names), 41))
    env.reset()
    assert same_bits(read(env), want)
    other = fresh(cc.U)
    other.reset()
    env.set_state(other.get_state())
    other.close()
    assert same_bits(read(env), want)
    env.reset()          # three envs in three states
    state, before = env.get_state().clone(), env.render(width=w, height=h).clone()
    perm = [2, 0, 1]
    env.clone_envs(torch.tensor(perm, dtype=torch.int32))
    assert same_bits(read(env), want)
    cloned = env.render(width=w, height=h).clone()
    env.set_state(state[perm])          # the same states put there by hand: rows untouched (above), so this is "state of env perm[e], row of env e"
    assert torch.equal(env.render(width=w, height=h), cloned)
    for e in range(N):
        assert not torch.equal(cloned[e], before[perm[e]]) and not torch.equal(cloned[e], before[e])
    ar = fresh(cc.U, autoreset=True, max_episode_steps=0, end_on_fault=False)
    ar.set_visuals(**{k: torch.tensor(a).to(ar.device) for k, a in want.items()})
    _, _, done, _ = ar.step(torch.zeros((N, ar.dims['action'])), end_mask=torch.tensor([0, 1, 0], dtype=torch.uint8))
    assert done.cpu().tolist() == [False, True, False]
    assert same_bits(read(ar), want)
    ar.close()


def test_the_unculled_kernel_and_obs_img():
    """7: with rp_debug_render_cull off the bytes are the same; obs['img'] of a record_images step is render()'s image, drawn with the rows"""
    env, o = put(cc.U, 'scene'), cc.oracle_of(cc.U, 'scene')
    set_defaults(env, o)
    plain = env.render().clone()
    set_rows(env, vc.random_visuals(N, len(env.visual_names), 51))
    rows = env.cameras(**cc.ROWS)
    for w, h in SIZES:
        culled = env.render_layers(width=w, height=h, cameras=rows)
        assert env.lib.rp_debug_render_cull(env.h, 0) == 0
        try:
            every = env.render_layers(width=w, height=h, cameras=rows)
        finally:
            assert env.lib.rp_debug_render_cull(env.h, 1) == 0
        assert layers_equal(culled, every)
    env.record_images = True
    try:
        obs = env.calc_state()
        img = obs['img'].clone()
        assert torch.equal(img, env.render())
        obs, _, _, _ = env.step(torch.zeros((N, env.dims['action'])))
        assert torch.equal(obs['img'].clone(), env.render())
    finally:
        env.record_images = False
    assert img.shape == plain.shape and not torch.equal(img, plain)
