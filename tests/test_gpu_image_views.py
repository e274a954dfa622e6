"""rp_set_image_views / VecPlayEnv.set_image_views: several camera views per env written by step, reset, calc_state and the autoreset step, two or more of them by
one pose launch and one k_render_views launch.  Run with -m gpu on the MI355X box.

The yardstick is render_layers on a handle in the same state, env by env (envs=(e, e + 1)) and with the view's own arguments - the public path the project holds to a
float64 ray cast (tests/test_gpu_camera_cases.py) -, never the code under test; the terminal frames of an autoreset step are held to a twin handle's render_layers
between its plain step and its masked reset (the pattern of tests/test_gpu_image_obs.py).  Every comparison is of bytes: there is no tolerance anywhere.
Shapes: 5 and 7 envs; image sizes where the split of the block index into (view, tile, env) can go wrong - 1 x 1 (a one-tile view BETWEEN two many-tile views),
16 x 16 (exactly one full tile), 17 x 16 (one column into a second tile), 33 x 50 and 70 x 45 (ragged tiles on both axes)."""
import ctypes as C

import numpy as np
import pytest

from reset_rows import reset_rows
from test_gpu_autoreset import actions, end_masks, make
from test_gpu_image_obs import fill_sentinel, is_sentinel, per_env_cameras, same_bytes
from test_gpu_reset_table import start_table

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

U, P, W = 'UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'pandaPlay-v0'
ALL = ('rgb', 'depth', 'segmentation')
MERGE = pytest.mark.parametrize('merge', (1, 0), ids=('merged', 'per-view'))


def render_kw(spec, e=None):
    """render_layers' keyword arguments for a view's spec; e: for env e alone (its row of the view's per-env cameras)"""
    kw = {k: v for k, v in spec.items() if k not in ('layers', 'terminal', 'cameras')}
    if spec.get('cameras') is not None:
        kw['cameras'] = spec['cameras'] if e is None else spec['cameras'][e:e + 1].contiguous()
    return kw


def assert_views_equal_render_layers(env, got, specs, what, envs=None):
    """every row (of `envs`, default all) of every layer of every view = render_layers(envs=(e, e + 1), that view's arguments) on env now"""
    assert list(got) == list(specs), what
    for name, spec in specs.items():
        assert set(got[name]) == set(spec['layers']), (what, name)
        for e in (range(env.num_envs) if envs is None else envs):
            want = env.render_layers(layers=spec['layers'], envs=(e, e + 1), **render_kw(spec, e))
            for k in spec['layers']:
                assert same_bytes(got[name][k][e:e + 1], want[k]), (what, name, k, e)


def four_views(env):
    return {'img': dict(width=33, height=50, layers=('rgb', 'depth'), depth='buffer'),
            'wrist': dict(width=70, height=45, layers=ALL, depth='metres', camera=env.camera(gripper=True)),
            'dot': dict(width=1, height=1, layers=('segmentation',), cameras=per_env_cameras(env)),
            'side': dict(width=17, height=16, layers=('rgb',), camera=env.camera(yaw=40.0, distance=1.1, fov=60.0, aspect=1.4), near=0.05, far=4.0)}


def two_views(env):
    return {'tile': dict(width=16, height=16, layers=ALL, depth='metres', cameras=per_env_cameras(env), near=0.05, far=4.0),
            'wrist': dict(width=17, height=16, layers=('rgb', 'depth'), camera=env.camera(gripper=True))}


def three_views(env):
    """the middle view, of one tile, has no terminal frames: the terminal pass has the tiles of 'img' and 'wrist' alone, one behind the other"""
    return {'img': dict(width=33, height=50, layers=ALL),
            'dot': dict(width=1, height=1, layers=('segmentation',), cameras=per_env_cameras(env), terminal=False),
            'wrist': dict(width=70, height=45, layers=('rgb', 'depth'), depth='metres', camera=env.camera(gripper=True))}


def set_merge(env, on):
    env._call('rp_debug_image_views_merge', int(on))


def random_visuals(env, seed):
    rng = np.random.default_rng(seed)
    nc, pick = len(env.visual_names), np.arange(env.num_envs) % 3
    env.set_visuals(colour=rng.random((3, nc, 3)).astype(np.float32)[pick], background=rng.random((3, 3)).astype(np.float32)[pick],
                    light=np.array([[0, 0, 1, 0.3, 0.7], [1, 1, 1, 0.6, 0.6], [-1, 2, 2, 0.2, 0.5]], dtype=np.float32)[pick])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1: step, reset, calc_state (and 5: either setting of the merge switch against the same yardstick)

@MERGE
@pytest.mark.parametrize('gid,views,n,visuals', ((U, four_views, 5, False), (P, two_views, 7, True), (W, two_views, 5, False)), ids=('U-four', 'P-two-visuals', 'W-two'))
def test_step_reset_and_calc_state_draw_every_view(gid, views, n, visuals, merge):
    """after reset, after each of three steps and after calc_state every row of every layer of every view equals render_layers of that env with the view's arguments;
    obs['img'] is the view named 'img''s rgb (None without such a view), obs['depth'] / obs['segmentation'] are absent; the tensors are the same objects call to call"""
    env = make(gid, n, 3)
    specs = views(env)
    set_merge(env, merge)
    env.set_image_views(specs)
    if visuals:
        random_visuals(env, 8)
    assert set(env.image_view_cameras) == {k for k, s in specs.items() if 'cameras' in s} and env.image_views_final is None
    obs = env.reset()
    assert_views_equal_render_layers(env, obs['views'], specs, 'reset')
    assert obs['img'] is (obs['views']['img']['rgb'] if 'img' in specs else None) and 'depth' not in obs and 'segmentation' not in obs
    acts = actions(env, 3, 5)
    first = {name: {k: t.clone() for k, t in v.items()} for name, v in obs['views'].items()}
    for t in range(3):
        obs, _, _, _ = env.step(acts[t])
        assert all(obs['views'][name][k] is env.image_views[name][k] for name, s in specs.items() for k in s['layers'])
        assert_views_equal_render_layers(env, obs['views'], specs, 'step %d' % t)
    assert not same_bytes(first['wrist']['rgb'], obs['views']['wrist']['rgb'])          # (the arm moved: the gripper camera's frames are not one picture)
    for v in env.image_views.values():
        fill_sentinel(v)
    obs = env.calc_state()
    assert_views_equal_render_layers(env, obs['views'], specs, 'calc_state')
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2: masked resets

@pytest.mark.parametrize('gid', (U, P))
def test_masked_reset_redraws_only_the_masked_envs_in_every_view(gid):
    """reset(mask) and reset(mask, o=...): the masked envs' rows of every view equal render_layers, every other row keeps the sentinel in every byte"""
    n = 7
    env = make(gid, n, 9)
    specs = three_views(env)
    env.set_image_views(specs)
    obs = env.reset()
    start = obs['obs_quat'].clone()
    env.step(actions(env, 1, 2)[0])
    chosen = [1, 4, 6]
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[chosen] = 1
    for what, o in (('reset(mask)', None), ('reset(mask, o)', start)):
        if o is not None and o.shape[1] < 18:
            o = torch.cat([o, torch.zeros((n, 18 - o.shape[1]), device=o.device)], 1)
        for v in env.image_views.values():
            fill_sentinel(v)
        obs = env.reset(mask=mask, o=o)
        assert_views_equal_render_layers(env, obs['views'], specs, what, envs=chosen)
        for name, v in obs['views'].items():
            for k, t in v.items():
                for i in set(range(n)) - set(chosen):
                    assert is_sentinel(k, t[i]), (what, name, k, i)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3: terminal frames against a twin (and 5: either setting of the merge switch)

@MERGE
@pytest.mark.parametrize('table', (False, True), ids=('settle', 'table'))
def test_autoreset_terminal_frames_of_every_view_against_a_twin(table, merge):
    """Handle A: autoreset with a time limit of 3, staggered counters, a random end_mask and three views of which the middle one has NO terminal tensors; once settling,
    once from a reset table.  Twin B: same seed and actions, plain step, then the masked reset.  Before each step A's terminal tensors hold a sentinel.  After it: the
    ended envs' terminal rows of the first and the third view equal B's render_layers(envs=(e, e + 1)) taken between B's step and its reset; every other terminal row
    keeps the sentinel; A's observation layers equal A's own render_layers after the call.  Step 2 ends every env, step 3 none.  C: A without images - same state."""
    gid, n = (P, 7) if table else (U, 5)
    steps, seed, stagger = 6, 21, 3
    B = make(gid, n, seed)
    tab = start_table(B, 4, seed + 100) if table else None
    A = make(gid, n, seed, autoreset=True, max_episode_steps=stagger, reset_table=tab)
    Cn = make(gid, n, seed, autoreset=True, max_episode_steps=stagger, reset_table=tab)
    specs = three_views(A)
    set_merge(A, merge)
    A.set_image_views(specs)
    assert list(A.image_views_final) == ['img', 'wrist'] and all(set(A.image_views_final[k]) == set(specs[k]['layers']) for k in ('img', 'wrist'))
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
    cursor, ends = 0, []
    for t in range(steps):
        for v in A.image_views_final.values():
            fill_sentinel(v)
        oa, _, da, ia = A.step(acts[t], end_mask=masks[t])
        Cn.step(acts[t], end_mask=masks[t])
        B.step(acts[t])
        status = B.buf['status'].clone()
        c1 = cnt + 1
        mask = (c1 >= stagger) | (masks[t] != 0) | ((status & 3) != 0)
        cnt = torch.where(mask, torch.zeros_like(c1), c1)
        ended = [int(i) for i in mask.nonzero().flatten().cpu()]
        last = {(name, i): B.render_layers(layers=specs[name]['layers'], envs=(i, i + 1), **render_kw(specs[name], i)) for name in ('img', 'wrist') for i in ended}
        if ended:
            if table:
                r, cursor = reset_rows(mask.cpu().numpy(), cursor, tab.shape[0])
                B.reset(mask=mask, o=tab[torch.from_numpy(r).to(dev).clamp(min=0).long()])
            else:
                B.reset(mask=mask)
        torch.cuda.synchronize()
        ends.append(len(ended))
        assert torch.equal(da, mask), t
        term = ia['terminal_observation']['views']
        assert term is A.image_views_final and 'dot' not in term
        for name in ('img', 'wrist'):
            for k in specs[name]['layers']:
                for i in range(n):
                    if i in ended:
                        assert same_bytes(term[name][k][i:i + 1], last[(name, i)][k]), (t, name, k, i)
                    else:
                        assert is_sentinel(k, term[name][k][i]), (t, name, k, i)
        assert_views_equal_render_layers(A, oa['views'], specs, 'obs of step %d' % t)
        assert torch.equal(A.get_state(), B.get_state()), t
        assert torch.equal(A.get_state(), Cn.get_state()), t
        assert torch.equal(A.episode_steps, cnt), t
    assert ends[2] == n and ends[3] == 0 and 0 < ends[0] < n, ends
    for env in (A, B, Cn):
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4: cameras rewritten in place

def test_camera_rows_rewritten_in_place_move_their_view_alone():
    n = 5
    env = make(U, n, 4)
    specs = {'a': dict(width=33, height=50, layers=('rgb',), cameras=per_env_cameras(env)),
             'fixed': dict(width=17, height=16, layers=('rgb', 'segmentation')),
             'b': dict(width=70, height=45, layers=('rgb', 'depth'), cameras=per_env_cameras(env, shift=20.0))}
    env.set_image_views(specs)
    assert env.image_view_cameras['a'] is specs['a']['cameras'] and env.image_view_cameras['b'] is specs['b']['cameras'] and 'fixed' not in env.image_view_cameras
    env.reset()
    acts = actions(env, 2, 6)
    obs, _, _, _ = env.step(acts[0])
    assert_views_equal_render_layers(env, obs['views'], specs, 'before')
    old = specs['b']['cameras'].clone()
    ptr = env.image_view_cameras['b'].data_ptr()
    env.image_view_cameras['b'][:] = per_env_cameras(env, shift=70.0).flip(0)          # in place: the library reads the same memory at the next draw
    assert env.image_view_cameras['b'].data_ptr() == ptr
    obs, _, _, _ = env.step(acts[1])
    assert_views_equal_render_layers(env, obs['views'], specs, 'after')          # 'b' with the new rows, 'a' and 'fixed' with what they had
    stale = env.render_layers(width=70, height=45, layers=('rgb',), cameras=old)
    for e in range(n):
        assert not torch.equal(obs['views']['b']['rgb'][e], stale['rgb'][e]), e
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5: the merge switch, handle against handle

def test_merged_and_per_view_launches_write_the_same_bytes():
    """two handles with the same seed, one drawing its views in one k_render_views launch, one in a k_render_layers launch per view: the observation tensors of a
    reset and of three autoreset steps (time limit 2, staggered: ends in every step) and the terminal tensors are bitwise equal, layer by layer"""
    n = 7
    envs = []
    for on in (1, 0):
        env = make(U, n, 11, autoreset=True, max_episode_steps=2)
        set_merge(env, on)
        env.set_image_views(four_views(env))
        envs.append(env)
    M, S = envs
    seen = 0
    for env in envs:
        env.reset()
        env.episode_steps = torch.arange(n, device=env.device, dtype=torch.int32) % 2
        for v in env.image_views_final.values():
            fill_sentinel(v)
    acts = actions(M, 3, 2)
    for t in range(3):
        om, _, dm, im = M.step(acts[t])
        os_, _, ds, is_ = S.step(acts[t])
        assert torch.equal(dm, ds) and bool(dm.any())
        for a, b in ((om['views'], os_['views']), (im['terminal_observation']['views'], is_['terminal_observation']['views'])):
            assert list(a) == list(b) == ['img', 'wrist', 'dot', 'side']
            for name in a:
                for k in a[name]:
                    assert same_bytes(a[name][k], b[name][k]), (t, name, k)
                    seen += 1
    assert seen == 3 * 2 * 7
    assert not is_sentinel('rgb', im['terminal_observation']['views']['side']['rgb'])
    for env in envs:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6: one configuration per handle

def test_one_configuration_per_handle():
    """a single view through set_image_views gives set_image_obs' tensors; set_image_obs after set_image_views, and the reverse, leave only the later one drawing;
    set_image_views(None) restores the observation of a handle without images"""
    n = 5
    kw = dict(width=33, height=50, layers=ALL, depth='metres')
    X, Y = make(U, n, 1), make(U, n, 1)
    X.set_image_views({'img': kw})
    Y.set_image_obs(**kw)
    acts = actions(X, 4, 1)
    for env in (X, Y):
        env.reset()
    ox, _, _, _ = X.step(acts[0])
    oy, _, _, _ = Y.step(acts[0])
    assert ox['img'] is ox['views']['img']['rgb'] and 'depth' not in ox
    for k in ALL:
        assert same_bytes(ox['views']['img'][k], oy['img' if k == 'rgb' else k]), k
    Y.close()
    # set_image_views (two views) replaces the single configuration ...
    specs = two_views(X)
    single = dict(X.image_views['img'])
    X.set_image_views(specs)
    fill_sentinel(single)
    obs, _, _, _ = X.step(acts[1])
    assert all(is_sentinel(k, t) for k, t in single.items())
    assert obs['img'] is None and list(obs['views']) == ['tile', 'wrist']
    assert_views_equal_render_layers(X, obs['views'], specs, 'views over a single configuration')
    # ... set_image_obs replaces the views ...
    former = {name: dict(v) for name, v in X.image_views.items()}
    X.set_image_obs(**kw)
    assert X.image_views is None and X.image_view_cameras == {}
    for v in former.values():
        fill_sentinel(v)
    obs, _, _, _ = X.step(acts[2])
    assert all(is_sentinel(k, t) for v in former.values() for k, t in v.items())
    assert 'views' not in obs
    want = X.render_layers(**kw)
    for k in ALL:
        assert same_bytes(obs['img' if k == 'rgb' else k], want[k]), k
    # ... and the views replace it again; then off
    X.set_image_views(specs)
    assert X.image_obs is None
    obs, _, _, _ = X.step(acts[3])
    assert 'depth' not in obs
    assert_views_equal_render_layers(X, obs['views'], specs, 'views over set_image_obs')
    former = {name: dict(v) for name, v in X.image_views.items()}
    X.set_image_views(None)
    assert X.image_views is None and X.image_obs is None
    for v in former.values():
        fill_sentinel(v)
    obs = X.calc_state()
    torch.cuda.synchronize()
    assert obs['img'] is None and 'views' not in obs and 'depth' not in obs
    assert all(is_sentinel(k, t) for v in former.values() for k, t in v.items())
    X.close()


def staggered_autoreset(envs, steps, seed, limit=3):
    """reset, counters e % limit, and the (actions, end_masks) of `steps` steps for handles made with autoreset=True and max_episode_steps=limit: the time limit ends
    some envs in the first steps, end_mask all of them in step 2 and - the counters being level then - nothing ends in step 3"""
    n, dev = envs[0].num_envs, envs[0].device
    for env in envs:
        env.reset()
        env.episode_steps = torch.arange(n, device=dev, dtype=torch.int32) % limit
    masks = end_masks(n, steps, seed + 1, dev, p=0.2)
    if steps > 3:
        masks[2] = torch.ones(n, device=dev, dtype=torch.uint8)
        masks[3] = torch.zeros(n, device=dev, dtype=torch.uint8)
    return actions(envs[0], steps, seed), masks


def flat(d, prefix=''):
    """{'layer' or 'points/key': tensor} of a view's tensor dict"""
    out = {}
    for k, t in d.items():
        out.update(flat(t, k + '/') if isinstance(t, dict) else {prefix + k: t})
    return out


def fill_sentinel_deep(d):
    fill_sentinel({k: t for k, t in d.items() if not isinstance(t, dict)})
    for t in d.values():
        if isinstance(t, dict):
            fill_sentinel(t)


def test_one_view_is_a_table_of_one():
    """One view with a cloud, configured three ways: A by set_image_obs + set_image_points, B by set_image_views with the merge switch on, C the same with it off.
    Same seed, actions and end_masks over 6 autoreset steps (time limit 3, staggered; step 2 ends every env, step 3 none): every observation layer and cloud, every
    terminal layer and cloud, done and reset_row are equal across the three, byte for byte; the terminal rows of envs that did not end keep the sentinel; env 3's
    observation rows equal A's render_layers(envs=(3, 4))."""
    n, steps, seed = 5, 6, 21
    envs = [make(U, n, seed, autoreset=True, max_episode_steps=3) for _ in range(3)]
    A, B, Cc = envs
    cloud = dict(n=64, colour=True)
    spec = dict(width=33, height=50, layers=ALL, depth='metres', cameras=per_env_cameras(A))
    A.set_image_obs(**spec)
    A.set_image_points(**cloud)
    for env, on in ((B, 1), (Cc, 0)):
        set_merge(env, on)
        env.set_image_views({'img': dict(points=cloud, **{**spec, 'cameras': per_env_cameras(env)})})
    acts, masks = staggered_autoreset(envs, steps, seed)

    def tensors(env, obs, info):
        """(observation, terminal) tensors by 'layer' / 'points/key', named alike for the two ways to configure the view"""
        term = info['terminal_observation']
        if env is A:
            return tuple(flat({**{k: o['img' if k == 'rgb' else k] for k in ALL}, 'points': o['points']}) for o in (obs, term))
        return flat(obs['views']['img']), flat(term['views']['img'])

    names = set(ALL) | {'points/' + k for k in ('xyz', 'segmentation', 'count', 'rgb')}
    ends = []
    for t in range(steps):
        fill_sentinel(A.image_final)
        fill_sentinel(A.image_points_final)
        for env in (B, Cc):
            fill_sentinel_deep(env.image_views_final['img'])
        got = []
        for env in envs:
            obs, _, done, info = env.step(acts[t], end_mask=masks[t])
            got.append(tensors(env, obs, info) + (done, info['reset_row']))
        torch.cuda.synchronize()
        (oa, ta, da, ra) = got[0]
        assert set(oa) == set(ta) == names
        for which, (o, term, done, row) in zip('BC', got[1:]):
            assert set(o) == set(term) == names, which
            assert torch.equal(done, da) and torch.equal(row, ra), (t, which)
            for k in names:
                assert same_bytes(o[k], oa[k]), (t, which, 'obs', k)
                assert same_bytes(term[k], ta[k]), (t, which, 'terminal', k)
        ended = [bool(x) for x in da.cpu()]
        ends.append(sum(ended))
        for which, (_, term, _, _) in zip('ABC', got):
            for k in names:
                for i in range(n):
                    if not ended[i]:
                        assert is_sentinel(k.split('/')[-1], term[k][i]), (t, which, k, i)
        for i in range(n):
            if ended[i]:
                assert not is_sentinel('rgb', ta['rgb'][i]), (t, i)
        e = 3
        want = A.render_layers(layers=ALL, envs=(e, e + 1), **render_kw(spec, e))
        for k in ALL:
            assert same_bytes(oa[k][e:e + 1], want[k]), (t, k)
    assert ends[2] == n and ends[3] == 0 and 0 < ends[0] < n, ends
    for env in envs:
        env.close()


def test_a_two_view_configuration_with_one_terminal_view():
    """two views of which the first has no terminal frames: the terminal pass of this TWO-view configuration has one entry.  A handle with the merge switch on and one
    with it off, same seed, 4 autoreset steps (time limit 3, staggered): the observation tensors of both views and the terminal tensors of the one terminal view are
    equal byte for byte, the terminal rows of envs that did not end keep the sentinel, and image_views_final has that view alone"""
    n, steps, seed = 5, 4, 21
    envs = [make(U, n, seed, autoreset=True, max_episode_steps=3) for _ in range(2)]
    for env, on in zip(envs, (1, 0)):
        set_merge(env, on)
        specs = two_views(env)
        specs['tile']['terminal'] = False
        env.set_image_views(specs)
        assert list(env.image_views_final) == ['wrist'] and set(env.image_views_final['wrist']) == {'rgb', 'depth'}
    M, S = envs
    acts, masks = staggered_autoreset(envs, steps, seed)
    ends = []
    for t in range(steps):
        for env in envs:
            fill_sentinel(env.image_views_final['wrist'])
        om, _, dm, im = M.step(acts[t], end_mask=masks[t])
        os_, _, ds, is_ = S.step(acts[t], end_mask=masks[t])
        torch.cuda.synchronize()
        assert torch.equal(dm, ds), t
        assert list(om['views']) == list(os_['views']) == ['tile', 'wrist']
        for name in ('tile', 'wrist'):
            assert set(om['views'][name]) == set(os_['views'][name]) == set(specs[name]['layers'])
            for k in specs[name]['layers']:
                assert same_bytes(om['views'][name][k], os_['views'][name][k]), (t, name, k)
        tm, ts = im['terminal_observation']['views'], is_['terminal_observation']['views']
        assert list(tm) == list(ts) == ['wrist']
        ended = [bool(x) for x in dm.cpu()]
        ends.append(sum(ended))
        for k in ('rgb', 'depth'):
            assert same_bytes(tm['wrist'][k], ts['wrist'][k]), (t, k)
            for i in range(n):
                assert is_sentinel(k, tm['wrist'][k][i]) == (not ended[i]), (t, k, i)
    assert ends[2] == n and ends[3] == 0 and 0 < ends[0] < n, ends
    for env in envs:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7: refusals

def test_refusals_leave_the_configuration_in_force_drawing():
    """five views, a view with no layer, with both cam and cam_rows, with far <= near, with an unknown depth mode, a 0 x 5 view: RP_ERR_ARG at the ABI (RuntimeError
    from _call, the message naming the view), ValueError from set_image_views; the two views set before still draw, and no refused call's buffer is written"""
    from roboticsplayroompybullet_amd._lib import RpImageView
    n = 5
    env = make(U, n, 1)
    env.reset()
    specs = two_views(env)
    env.set_image_views(specs)
    buf = torch.zeros((n, 16, 16, 3), dtype=torch.uint8, device=env.device)
    cam, rows = env.camera(), env.cameras()

    def view(**kw):
        v = RpImageView()
        v.near_plane, v.far_plane, v.depth_mode, v.width, v.height, v.rgb = 0.01, 10.0, 0, 16, 16, buf.data_ptr()
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def call(*vs):
        env._call('rp_set_image_views', (RpImageView * len(vs))(*vs), len(vs))

    with pytest.raises(RuntimeError, match='rp_set_image_views: n_views'):
        call(*[view() for _ in range(5)])
    with pytest.raises(RuntimeError, match='rp_set_image_views: n_views'):
        env._call('rp_set_image_views', None, -1)
    with pytest.raises(RuntimeError, match='rp_set_image_views: views is NULL'):
        env._call('rp_set_image_views', None, 2)
    bad = {'no layer': view(rgb=None), 'cam and cam_rows': view(cam=C.pointer(cam), cam_rows=rows.data_ptr()), 'far <= near': view(near_plane=1.0, far_plane=1.0),
           'depth mode': view(depth_mode=2), '0 x 5': view(width=0, height=5)}
    for name, v in bad.items():
        with pytest.raises(RuntimeError, match='rp_set_image_views: view 1: '):
            call(view(), v)
        with pytest.raises(RuntimeError, match='rp_set_image_views: view 0: '):          # (a single bad view: refused before it is handed to rp_set_image_obs' path)
            call(v)
    ok = dict(width=16, height=16)
    with pytest.raises(ValueError, match='set_image_views'):
        env.set_image_views({str(i): ok for i in range(5)})
    for kw in (dict(layers=()), dict(camera=cam, cameras=rows), dict(near=1.0, far=1.0), dict(depth='metric'), dict(width=0, height=5)):
        with pytest.raises(ValueError, match="set_image_views: view 'second'"):
            env.set_image_views({'first': ok, 'second': {**ok, **kw}})
    obs, _, _, _ = env.step(actions(env, 1, 1)[0])          # the configuration of before the refusals is in force
    assert list(obs['views']) == ['tile', 'wrist']
    assert_views_equal_render_layers(env, obs['views'], specs, 'after the refusals')
    assert not bool(buf.any())
    env.close()


def test_the_tile_limit_counts_the_sum_of_the_views():
    """32768 envs, two views of 4096 x 2048: 2^30 tiles each - either would pass alone -, 2^31 together; refused before any buffer is looked at"""
    from roboticsplayroompybullet_amd._lib import RpImageView
    env = make('UR5Reach-v0', 32768, 1)
    one = torch.zeros(4, dtype=torch.uint8, device=env.device)
    vs = (RpImageView * 2)()
    for v in vs:
        v.near_plane, v.far_plane, v.width, v.height, v.rgb = 0.01, 10.0, 4096, 2048, one.data_ptr()
    with pytest.raises(RuntimeError, match='tiles of 2 views exceed one launch'):
        env._call('rp_set_image_views', vs, 2)
    env._call('rp_set_image_views', None, 0)
    env.close()
