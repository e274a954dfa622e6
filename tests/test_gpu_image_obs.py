"""rp_set_image_obs / VecPlayEnv.set_image_obs: camera images written by step, reset, calc_state and the autoreset step.  Run with -m gpu on the MI355X box.

The yardstick is the public path the project holds to a float64 ray cast, render_layers on a handle in the same state (tests/test_gpu_camera_cases.py), never the
code under test: the images of a call equal, by torch.equal, what render_layers with the same arguments draws right after it, and the terminal frames of an
autoreset step equal what a twin handle with the same seed draws between its plain step and its masked reset (the pattern of tests/test_gpu_autoreset.py).
Shapes: 5 and 7 envs (no multiple of four or of the wave), images of 33 x 50 and 70 x 45 (ragged 16 x 16 tiles on both axes) and 1 x 1.
"""
import ctypes as C

import numpy as np
import pytest

from reset_rows import reset_rows
from test_gpu_autoreset import actions, end_masks, make
from test_gpu_reset_table import start_table

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

U, P, W = 'UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'pandaPlay-v0'
ALL = ('rgb', 'depth', 'segmentation')
SIZES = ((33, 50), (70, 45), (1, 1))
SENTINEL_BYTE = 0xA5
SENTINEL_WORD = 0x5A5AA5A5          # depth and segmentation: a fixed bit pattern (as a float 1.5e16, as an int no packed collider)


def fill_sentinel(tensors):
    for k, t in tensors.items():
        if k == 'rgb':
            t.fill_(SENTINEL_BYTE)
        else:
            t.view(torch.int32).fill_(SENTINEL_WORD)


def is_sentinel(k, rows):
    """every byte of the rows is the sentinel's"""
    if k == 'rgb':
        return bool((rows == SENTINEL_BYTE).all())
    return bool((rows.contiguous().view(torch.int32) == SENTINEL_WORD).all())


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def images(obs, layers):
    """the image tensors of an observation (or of info['terminal_observation']) by layer name"""
    return {k: obs['img' if k == 'rgb' else k] for k in layers}


def assert_equal_to_render_layers(env, got, layers, kw, what):
    want = env.render_layers(layers=layers, **kw)
    torch.cuda.synchronize()
    for k in layers:
        assert same_bytes(got[k], want[k]), (what, k)
    return want


def per_env_cameras(env, shift=0.0):
    n = env.num_envs
    i = np.arange(n)
    return env.cameras(yaw=-60.0 + 25.0 * i + shift, distance=0.9 + 0.15 * i, fov=35.0 + 6.0 * i, aspect=0.7 + 0.12 * i, pitch=-25.0 - 3.0 * i)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1: step and calc_state

@pytest.mark.parametrize('layers', (('depth',), ALL), ids=('depth', 'all'))
@pytest.mark.parametrize('depth', ('buffer', 'metres'))
@pytest.mark.parametrize('gid', (U, P, W))
def test_step_and_calc_state_images_equal_render_layers(gid, depth, layers):
    """after reset, after each of 3 random-action steps and after calc_state, every requested layer equals render_layers(same arguments) called right after, byte for
    byte; the layers not asked for are absent (img: None); the output tensors are the same objects from call to call"""
    n = 5 if depth == 'buffer' else 7
    w, h = SIZES[0] if layers == ALL else SIZES[1]
    env = make(gid, n, 3)
    kw = dict(width=w, height=h, depth=depth, near=0.05, far=4.0)
    env.set_image_obs(layers=layers, **kw)
    obs = env.reset()
    assert_equal_to_render_layers(env, images(obs, layers), layers, kw, 'reset')
    assert ('rgb' in layers) == (obs['img'] is not None) and all((k in obs) == (k in layers) for k in ('depth', 'segmentation'))
    acts = actions(env, 3, 5)
    seen = []
    for t in range(3):
        obs, _, _, _ = env.step(acts[t])
        got = images(obs, layers)
        assert all(got[k] is env.image_obs[k] for k in layers)
        want = assert_equal_to_render_layers(env, got, layers, kw, 'step %d' % t)
        seen.append(want['depth'].clone())
        assert tuple(got['depth'].shape) == (n, h, w) and got['depth'].dtype == torch.float32
    assert not torch.equal(seen[0], seen[2])          # (the arm moved: the frames are not one picture)
    miss = 4.0 if depth == 'metres' else 1.0
    assert bool((seen[2] < miss).any())          # (something is hit)
    fill_sentinel(env.image_obs)
    obs = env.calc_state()
    assert_equal_to_render_layers(env, images(obs, layers), layers, kw, 'calc_state')
    env.close()


def test_one_pixel_images():
    """1 x 1: one tile per env, one live thread per block"""
    env = make(U, 7, 3)
    kw = dict(width=1, height=1)
    env.set_image_obs(layers=ALL, **kw)
    env.reset()
    obs, _, _, _ = env.step(actions(env, 1, 5)[0])
    assert tuple(obs['img'].shape) == (7, 1, 1, 3)
    assert_equal_to_render_layers(env, images(obs, ALL), ALL, kw, '1 x 1')
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2: cameras

@pytest.mark.parametrize('gid', (U, P))
def test_cameras_default_gripper_and_per_env_rows(gid):
    """the default camera, the gripper camera and per-env rows that differ in yaw, distance, fov and aspect; rows rewritten in place between two steps are the next
    step's cameras: its images equal render_layers with the new rows and differ from the ones the old rows give"""
    n, (w, h) = 5, SIZES[1]
    env = make(gid, n, 4)
    env.reset()
    acts = actions(env, 4, 6)
    pictures = {}
    for name, cam in (('default', {}), ('explicit', dict(camera=env.camera(yaw=40.0, distance=1.1, fov=60.0, aspect=1.4))), ('gripper', dict(camera=env.camera(gripper=True)))):
        kw = dict(width=w, height=h, **cam)
        env.set_image_obs(layers=ALL, **kw)
        assert env.image_cameras is None
        obs, _, _, _ = env.step(acts[0])
        pictures[name] = assert_equal_to_render_layers(env, images(obs, ALL), ALL, kw, name)['rgb'].clone()
    assert not torch.equal(pictures['default'], pictures['gripper']) and not torch.equal(pictures['default'], pictures['explicit'])
    rows = per_env_cameras(env)
    env.set_image_obs(width=w, height=h, layers=ALL, cameras=rows)
    assert env.image_cameras is rows
    obs, _, _, _ = env.step(acts[1])
    first = assert_equal_to_render_layers(env, images(obs, ALL), ALL, dict(width=w, height=h, cameras=rows), 'rows')
    assert len({first['rgb'][e].cpu().numpy().tobytes() for e in range(n)}) == n          # every env its own view
    old = rows.clone()
    env.image_cameras[:] = per_env_cameras(env, shift=70.0).flip(0)          # in place: the library reads the same memory at the next draw
    assert env.image_cameras.data_ptr() == rows.data_ptr()
    obs, _, _, _ = env.step(acts[2])
    got = {k: v.clone() for k, v in images(obs, ALL).items()}
    assert_equal_to_render_layers(env, got, ALL, dict(width=w, height=h, cameras=env.image_cameras), 'rewritten rows')
    stale = env.render_layers(width=w, height=h, cameras=old)
    for e in range(n):
        assert not torch.equal(got['rgb'][e], stale['rgb'][e]), e
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3: autoreset against a twin

@pytest.mark.parametrize('table', (False, True), ids=('settle', 'table'))
@pytest.mark.parametrize('gid', (U, P))
def test_autoreset_terminal_frames_against_a_twin(gid, table):
    """Handle A: autoreset with a time limit of 3, staggered counters, a random end_mask, image observations with terminal frames; once settling (k_autoreset), once
    from a reset table (k_autoreset_to).  Twin B: same seed and actions, plain step, then the masked reset that test_gpu_autoreset / test_gpu_reset_table prove equal.
    Before each step A's terminal tensors are filled with a sentinel.  After it: for the ended envs A's terminal rows equal B's render_layers(envs=(e, e + 1)) taken
    after B's step and before its reset; every other row keeps the sentinel in every byte; A's obs layers equal A's own render_layers after the call (the new
    episode's first frame for an ended env).  Step 2 ends every env (end_mask of ones), step 3 none.  C: A's configuration without image observations - same state."""
    n, (w, h) = (7, SIZES[0]) if table else (5, SIZES[1])
    steps, seed, stagger = 7, 21, 3
    B = make(gid, n, seed)
    tab = start_table(B, 4, seed + 100) if table else None
    A = make(gid, n, seed, autoreset=True, max_episode_steps=stagger, reset_table=tab)
    Cn = make(gid, n, seed, autoreset=True, max_episode_steps=stagger, reset_table=tab)
    cams = per_env_cameras(A)
    kw = dict(width=w, height=h, depth='metres', cameras=cams)
    A.set_image_obs(layers=ALL, **kw)
    assert set(A.image_final) == set(ALL)
    for env in (A, B, Cn):
        env.reset()
    dev = A.device
    e = torch.arange(n, device=dev, dtype=torch.int32)
    A.episode_steps = e % stagger
    Cn.episode_steps = e % stagger
    cnt = (e % stagger).clone()
    acts = actions(A, steps, seed)
    masks = end_masks(n, steps, seed + 1, dev, p=0.2)
    masks[2] = torch.ones(n, device=dev, dtype=torch.uint8)
    masks[3] = torch.zeros(n, device=dev, dtype=torch.uint8)
    cursor, ends, differs = 0, [], 0
    for t in range(steps):
        fill_sentinel(A.image_final)
        oa, _, da, ia = A.step(acts[t], end_mask=masks[t])
        Cn.step(acts[t], end_mask=masks[t])
        B.step(acts[t])
        status = B.buf['status'].clone()
        c1 = cnt + 1
        mask = (c1 >= stagger) | (masks[t] != 0) | ((status & 3) != 0)
        cnt = torch.where(mask, torch.zeros_like(c1), c1)
        ended = [int(i) for i in mask.nonzero().flatten().cpu()]
        last = {i: B.render_layers(width=w, height=h, depth='metres', envs=(i, i + 1), cameras=cams[i:i + 1].contiguous()) for i in ended}
        if ended:
            if table:
                r, cursor = reset_rows(mask.cpu().numpy(), cursor, tab.shape[0])
                B.reset(mask=mask, o=tab[torch.from_numpy(r).to(dev).clamp(min=0).long()])
            else:
                B.reset(mask=mask)
        torch.cuda.synchronize()
        ends.append(len(ended))
        assert torch.equal(da, mask), t
        term = images(ia['terminal_observation'], ALL)
        for k in ALL:
            assert term[k] is A.image_final[k]
            for i in range(n):
                if i in last:
                    assert same_bytes(term[k][i:i + 1], last[i][k]), (t, k, i)
                else:
                    assert is_sentinel(k, term[k][i]), (t, k, i)
        got = {k: v.clone() for k, v in images(oa, ALL).items()}
        assert_equal_to_render_layers(A, got, ALL, kw, 'obs of step %d' % t)
        assert_equal_to_render_layers(B, got, ALL, kw, 'the twin after its reset, step %d' % t)
        differs += sum(not torch.equal(term['rgb'][i], got['rgb'][i]) for i in ended)
        assert torch.equal(A.get_state(), B.get_state()), t
        assert torch.equal(A.get_state(), Cn.get_state()), t
        assert torch.equal(A.episode_steps, cnt) and torch.equal(Cn.episode_steps, cnt), t
    print('%s table=%s: ends per step %s, ended envs whose terminal rgb differs from the new episode\'s first frame: %d' % (gid, table, ends, differs))
    assert ends[2] == n and ends[3] == 0 and 0 < ends[0] < n, ends
    assert differs >= 1
    for env in (A, B, Cn):
        env.close()


def test_terminal_layers_follow_the_requested_layers():
    """autoreset with ('depth',) alone: terminal_observation has img None and depth, no segmentation; without autoreset there are no terminal tensors"""
    A = make(U, 5, 2, autoreset=True, max_episode_steps=2)
    A.set_image_obs(width=33, height=50, layers='depth')
    A.reset()
    assert set(A.image_final) == {'depth'}
    fill_sentinel(A.image_final)
    ends = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    _, _, done, info = A.step(actions(A, 1, 1)[0], end_mask=ends)
    torch.cuda.synchronize()
    term = info['terminal_observation']
    assert term['img'] is None and 'segmentation' not in term and term['depth'] is A.image_final['depth']
    assert done.tolist() == [True, False, False, True, False]
    assert [is_sentinel('depth', term['depth'][i]) for i in range(5)] == [False, True, True, False, True]
    A.close()
    B = make(U, 5, 2)
    B.set_image_obs(width=33, height=50)
    assert B.image_final is None
    B.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4: masked resets

@pytest.mark.parametrize('gid', (U, P))
def test_masked_reset_redraws_only_the_masked_envs(gid):
    """reset(mask) and reset(mask, o=...): only the masked envs' image rows change - the sentinel stays on the rest - and the changed rows equal render_layers of
    those envs; no mask covers all envs"""
    n, (w, h) = 7, SIZES[0]
    env = make(gid, n, 9)
    kw = dict(width=w, height=h)
    env.set_image_obs(layers=ALL, **kw)
    obs = env.reset()
    start = obs['obs_quat'].clone()
    assert_equal_to_render_layers(env, images(obs, ALL), ALL, kw, 'reset()')
    env.step(actions(env, 1, 2)[0])
    chosen = [1, 4, 6]
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[chosen] = 1
    for what, o in (('reset(mask)', None), ('reset(mask, o)', start)):
        if o is not None and o.shape[1] < 18:
            o = torch.cat([o, torch.zeros((n, 18 - o.shape[1]), device=o.device)], 1)
        fill_sentinel(env.image_obs)
        obs = env.reset(mask=mask, o=o)
        want = env.render_layers(layers=ALL, **kw)
        torch.cuda.synchronize()
        for k, t in images(obs, ALL).items():
            for i in range(n):
                if i in chosen:
                    assert same_bytes(t[i], want[k][i]), (what, k, i)
                else:
                    assert is_sentinel(k, t[i]), (what, k, i)
        fill_sentinel(env.image_obs)
        obs = env.reset(o=o)
        assert_equal_to_render_layers(env, images(obs, ALL), ALL, kw, what + ' without a mask')
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5: visuals

def test_step_images_use_the_visuals_table():
    """after set_visuals with three different rows the step images equal render_layers, and differ from the default-visuals image"""
    n, (w, h) = 5, SIZES[1]
    env = make(U, n, 6)
    kw = dict(width=w, height=h)
    env.set_image_obs(layers=ALL, **kw)
    env.reset()
    acts = actions(env, 1, 3)
    plain = {k: v.clone() for k, v in images(env.calc_state(), ALL).items()}
    rng = np.random.default_rng(8)
    nc = len(env.visual_names)
    pick = np.arange(n) % 3
    env.set_visuals(colour=rng.random((3, nc, 3)).astype(np.float32)[pick], background=rng.random((3, 3)).astype(np.float32)[pick],
                    light=np.array([[0, 0, 1, 0.3, 0.7], [1, 1, 1, 0.6, 0.6], [-1, 2, 2, 0.2, 0.5]], dtype=np.float32)[pick])
    coloured = {k: v.clone() for k, v in images(env.calc_state(), ALL).items()}
    assert_equal_to_render_layers(env, coloured, ALL, kw, 'visuals, calc_state')
    for i in range(n):
        assert not torch.equal(coloured['rgb'][i], plain['rgb'][i]), i
    assert same_bytes(coloured['depth'], plain['depth']) and same_bytes(coloured['segmentation'], plain['segmentation'])
    obs, _, _, _ = env.step(acts[0])
    assert_equal_to_render_layers(env, images(obs, ALL), ALL, kw, 'visuals, step')
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6: off

def test_switching_off_restores_the_old_observation():
    """after set_image_obs(None) obs['img'] is None again, with record_images the 200 x 200 picture; the former output tensors are no longer written"""
    n = 5
    env = make(U, n, 1, autoreset=True, max_episode_steps=2)
    env.reset()
    acts = actions(env, 3, 1)
    obs, _, _, _ = env.step(acts[0])
    assert obs['img'] is None and 'depth' not in obs
    env.record_images = True
    env.set_image_obs(width=33, height=50, layers=ALL)
    obs, _, _, info = env.step(acts[1])
    assert tuple(obs['img'].shape) == (n, 50, 33, 3)          # while set, the 200 x 200 render is not made
    former = dict(env.image_obs), dict(env.image_final)
    env.set_image_obs(None)
    assert env.image_obs is None and env.image_final is None and env.image_cameras is None
    for t in former:
        fill_sentinel(t)
    obs, _, done, info = env.step(acts[2], end_mask=torch.ones(n, dtype=torch.uint8))          # (every env ends: a terminal pass would write every row)
    torch.cuda.synchronize()
    assert bool(done.all())
    assert tuple(obs['img'].shape) == (n, 200, 200, 3) and torch.equal(obs['img'], env.render())
    assert 'depth' not in obs and 'img' not in info['terminal_observation'] and 'depth' not in info['terminal_observation']
    for t in former:
        for k, v in t.items():
            assert is_sentinel(k, v), k
    env.record_images = False
    assert env.calc_state()['img'] is None
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7: errors

def test_bad_arguments_are_refused_and_the_handle_still_steps():
    """every RP_ERR_ARG case of the header, at the ABI (RuntimeError from _call) and, where VecPlayEnv checks first, at set_image_obs (ValueError); the configuration in
    force stays, and the handle steps afterwards with its images right"""
    n, (w, h) = 5, SIZES[0]
    env = make(U, n, 1)
    env.reset()
    kw = dict(width=w, height=h)
    env.set_image_obs(layers=ALL, **kw)
    bufs = {k: torch.zeros_like(v) for k, v in env.image_obs.items()}
    rgb, dep, seg = (C.c_void_p(bufs[k].data_ptr()) for k in ALL)
    cam = env.camera()
    rows = env.cameras()

    def call(camera=None, cam_rows=None, near=0.01, far=10.0, mode=0, width=w, height=h, out=(rgb, dep, seg)):
        env._call('rp_set_image_obs', C.byref(camera) if camera is not None else None, C.c_void_p(cam_rows.data_ptr()) if cam_rows is not None else None, near, far, mode,
                  width, height, *out, None, None, None)

    bad_fov, bad_mode, bad_aspect = env.camera(), env.camera(), env.camera()
    bad_fov.fov_deg, bad_mode.mode, bad_aspect.aspect = 180.0, 2, 0.0
    cases = {'no layer': dict(out=(None, None, None)), 'cam and cam_rows': dict(camera=cam, cam_rows=rows), 'zero width': dict(width=0), 'negative height': dict(height=-1),
             'too wide': dict(width=4097), 'too high': dict(height=4097), 'fov': dict(camera=bad_fov), 'mode': dict(camera=bad_mode), 'aspect': dict(camera=bad_aspect),
             'near': dict(near=0.0), 'far': dict(near=1.0, far=1.0), 'depth mode': dict(mode=2)}
    for name, c in cases.items():
        with pytest.raises(RuntimeError, match='rp_set_image_obs'):
            call(**c)
    for c in (dict(layers=()), dict(layers=('rgb', 'normals')), dict(camera=cam, cameras=rows), dict(near=0.0), dict(far=0.001), dict(depth='metric'), dict(width=0),
              dict(height=5000), dict(cameras=rows[:3]), dict(cameras=rows.cpu()), dict(cameras=torch.zeros((11, n), device=env.device).t())):
        with pytest.raises(ValueError, match='set_image_obs'):
            env.set_image_obs(**{**dict(width=w, height=h, layers=ALL), **c})
    obs, _, _, _ = env.step(actions(env, 1, 1)[0])          # the configuration of before the refusals is in force
    assert_equal_to_render_layers(env, images(obs, ALL), ALL, kw, 'after the refusals')
    assert all(not bool(t.any()) for t in bufs.values())          # ... and no refused call's buffers were written
    env.close()


def test_the_tile_limit_is_refused():
    """N * ceil(w / 16) * ceil(h / 16) > 2^31 - 1: 32768 envs of 4096 x 4096 are 2^31 tiles; refused before any buffer is looked at"""
    env = make('UR5Reach-v0', 32768, 1)
    one = torch.zeros(4, dtype=torch.uint8, device=env.device)
    with pytest.raises(RuntimeError, match='tiles exceed one launch'):
        env._call('rp_set_image_obs', None, None, 0.01, 10.0, 0, 4096, 4096, C.c_void_p(one.data_ptr()), None, None, None, None, None)
    env._call('rp_set_image_obs', None, None, 0.0, 0.0, 0, 0, 0, None, None, None, None, None, None)
    env.close()
