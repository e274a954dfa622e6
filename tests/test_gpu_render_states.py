"""rp_render_states / VecPlayEnv.render_states and goal_images: camera images of state rows the handle is not in.  Run with -m gpu on the MI355X box.

The yardstick is never the new code: it is render_layers on a handle (or a twin handle put into the state in question with set_state, set_visuals and
set_kinematics) - the path tests/test_gpu_camera_cases.py holds to a float64 ray cast - and the comparison is same_bytes on every layer.  Unwritten images are
checked with the sentinels of tests/test_gpu_image_obs.py.  Shapes: 4 envs; images of 33 x 20 and 17 x 16 (more than one 16 x 16 tile, no axis a multiple of 16);
seven images over chunks of three where a chunk boundary is to be crossed (rp_debug_render_states_chunk)."""
import ctypes as C
import re

import numpy as np
import pytest

from test_gpu_autoreset import actions, make
from test_gpu_image_obs import fill_sentinel, is_sentinel, same_bytes

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

U, P, W, R = 'UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'pandaPlay-v0', 'UR5Reach-v0'
ALL = ('rgb', 'depth', 'segmentation')
SIZES = ((33, 20), (17, 16))
N = 4


def stepped(gid, seed, steps=30, act_seed=5, **kw):
    """a handle of N envs after `steps` fixed random actions"""
    env = make(gid, N, seed, **kw)
    env.reset()
    for a in actions(env, steps, act_seed):
        env.step(a)
    return env


def cams(env, m, shift=0.0):
    """m different cameras [m, 11]"""
    i = np.arange(m)
    return env.cameras(yaw=-60.0 + 25.0 * i + shift, distance=0.9 + 0.15 * i, fov=35.0 + 6.0 * i, aspect=0.7 + 0.12 * i, pitch=-25.0 - 3.0 * i)


def i32(env, v):
    return torch.tensor(v, dtype=torch.int32, device=env.device)


def assert_same(got, want, what, rows=None):
    for k in ALL:
        a, b = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        assert same_bytes(a, b), (what, k)


def camera_choices(env, m):
    return {'fixed': {}, 'gripper': dict(camera=env.camera(gripper=True)), 'rows': dict(cameras=cams(env, m))}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 1: identity

@pytest.mark.parametrize('gid', (U, P, W))
def test_the_handle_s_own_rows_give_render_layers_bytes(gid):
    """render_states of get_state() after 30 random steps is render_layers, byte for byte: fixed, gripper and per-image cameras, both depth modes, both sizes; with
    the rows as get_state returns them, None (the live rows), the [:, :128] slice as a view and as a copy (stride 512 bytes), and embedded in a wider buffer
    (stride state_bytes + 64)"""
    env = stepped(gid, 3)
    states = env.get_state()
    nf = states.shape[1]
    assert nf >= 128
    wider = torch.zeros((N, nf + 16), dtype=torch.float32, device=env.device)
    wider[:, :nf] = states
    forms = {'get_state': states, 'live': None, 'slice': states[:, :128], 'records': states[:, :128].contiguous(), 'embedded': wider[:, :nf]}
    assert forms['records'].stride(0) == 128 and forms['embedded'].stride(0) == nf + 16
    for w, h in SIZES:
        for cname, cam in camera_choices(env, N).items():
            for depth in ('buffer', 'metres'):
                kw = dict(width=w, height=h, depth=depth, near=0.05, far=4.0, **cam)
                want = env.render_layers(**kw)
                for fname, s in forms.items():
                    got = env.render_states(s, **kw)
                    torch.cuda.synchronize()
                    assert_same(got, want, (gid, w, h, cname, depth, fname))
        assert bool((want['segmentation'] != -1).any())          # (the pictures show something)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 2: another handle's rows, gathered over several chunks

def test_rows_of_another_handle_gathered_over_chunks_leave_the_drawing_handle_alone():
    """handle A's rows drawn by handle B (same id, other states): 7 images of 4 rows with repeats, in chunks of 3, 3, 1; image i is A's render_layers image of env
    index[i] with camera row i.  B's state rows and episode counters are the same bytes afterwards, and its next step is a twin's that never drew.  Then M = 1 and
    M = 2 < N, with the chunk cap and without it"""
    A, B, T = stepped(U, 3), stepped(U, 9, act_seed=7), stepped(U, 9, act_seed=7)
    rows = A.get_state()
    assert not same_bytes(rows, B.get_state()) and same_bytes(B.get_state(), T.get_state())
    B.lib.rp_debug_render_states_chunk(B.h, 3)
    for index in ([2, 0, 2, 3, 1, 1, 0], [3], [1, 2]):
        m = len(index)
        crows = cams(A, m)
        for w, h in SIZES:
            for cname, cam in (('fixed', {}), ('gripper', dict(camera=A.camera(gripper=True))), ('rows', None)):
                if cam is None:          # camera row i belongs to image i: A draws env index[i] alone with that row
                    parts = [A.render_layers(width=w, height=h, depth='metres', envs=(e, e + 1), cameras=crows[i:i + 1]) for i, e in enumerate(index)]
                    want = {k: torch.cat([p[k] for p in parts]) for k in ALL}
                    cam = dict(cameras=crows)
                else:
                    full = A.render_layers(width=w, height=h, depth='metres', **cam)
                    want = {k: full[k][index] for k in ALL}
                before, steps = B.get_state().clone(), B.episode_steps.clone()
                got = B.render_states(rows, w, h, index=i32(B, index), depth='metres', **cam)
                torch.cuda.synchronize()
                assert tuple(got['rgb'].shape) == (m, h, w, 3)
                assert_same(got, want, (index, w, h, cname))
                assert same_bytes(B.get_state(), before) and torch.equal(B.episode_steps, steps)
    # the chunk size changes no byte
    index = i32(B, [2, 0, 2, 3, 1, 1, 0])
    three = B.render_states(rows, 33, 20, index=index, cameras=cams(A, 7))
    B.lib.rp_debug_render_states_chunk(B.h, 0)
    assert_same(B.render_states(rows, 33, 20, index=index, cameras=cams(A, 7)), three, 'one chunk')
    a = actions(B, 1, 11)[0]
    ob, rb, _, _ = B.step(a)
    ot, rt, _, _ = T.step(a)
    torch.cuda.synchronize()
    assert same_bytes(B.get_state(), T.get_state()) and same_bytes(rb, rt)
    for k in ('observation', 'achieved_goal', 'desired_goal'):
        assert same_bytes(ob[k], ot[k]), k
    for e in (A, B, T):
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 3: visuals

def visuals_values(env, seed):
    rng = np.random.default_rng(seed)
    nc = len(env.visual_names)
    return dict(colour=rng.random((N, nc, 3)).astype(np.float32), background=rng.random((N, 3)).astype(np.float32),
                light=np.array([[0, 0, 1, 0.3, 0.7], [1, 1, 1, 0.6, 0.6], [-1, 2, 2, 0.2, 0.5], [2, -1, 1, 0.5, 0.4]], dtype=np.float32))


def test_images_are_drawn_with_the_named_visuals_row():
    """a handle with four different visuals rows: visuals = identity gives render_layers' bytes; crossed permutations of index and visuals equal a twin given
    set_state(rows[index]) and set_visuals(values[visuals]); None, -1 and N give the default look of a twin that never called set_visuals; a handle without a
    table draws the default look and get_visuals afterwards returns the defaults"""
    V, T, D = stepped(U, 3), make(U, N, 3), make(U, N, 3)
    T.reset()
    D.reset()
    vals = visuals_values(V, 8)
    V.set_visuals(**vals)
    rows = V.get_state()
    D.set_state(rows)
    ident = i32(V, [0, 1, 2, 3])
    for w, h in SIZES:
        for cname, cam in (('fixed', {}), ('gripper', dict(camera=V.camera(gripper=True)))):
            kw = dict(width=w, height=h, **cam)
            own = V.render_layers(**kw)
            assert_same(V.render_states(None, visuals=ident, **kw), own, ('identity, live', w, h, cname))
            assert_same(V.render_states(rows, visuals=ident, **kw), own, ('identity, rows', w, h, cname))
            for index, vis in (([3, 1, 0, 2], [1, 3, 2, 0]), ([0, 0, 2, 1], [2, 2, 3, 3])):
                T.set_state(rows[index])
                T.set_visuals(**{k: v[vis] for k, v in vals.items()})
                want = T.render_layers(**kw)
                assert_same(V.render_states(rows, index=i32(V, index), visuals=i32(V, vis), **kw), want, ('crossed', index, vis, w, h, cname))
            plain = D.render_layers(**kw)
            assert not same_bytes(plain['rgb'], own['rgb'])
            assert_same(V.render_states(rows, **kw), plain, ('visuals=None', w, h, cname))
            assert_same(V.render_states(rows, visuals=i32(V, [-1, N, -1, N + 7]), **kw), plain, ('outside [0, N)', w, h, cname))
            mixed = V.render_states(rows, visuals=i32(V, [0, -1, N, 3]), **kw)
            assert_same(mixed, own, ('mixed, own rows', w, h, cname), rows=[0, 3])
            assert_same(mixed, plain, ('mixed, default rows', w, h, cname), rows=[1, 2])
            # D never made a table: the call draws the default look whatever visuals names, and makes none
            assert_same(D.render_states(rows, visuals=ident, **kw), plain, ('no table', w, h, cname))
    torch.cuda.synchronize()
    got = D.get_visuals()
    fresh = make(U, 1, 0)
    want = fresh.get_visuals()
    assert same_bytes(got['colour'], want['colour'].expand(N, -1, -1).contiguous())
    assert same_bytes(got['light'], torch.tensor([[0.2672612, -0.5345225, 0.8017837, 0.45, 0.55]] * N, dtype=torch.float32, device=D.device))
    assert same_bytes(got['background'], torch.tensor([[0.82, 0.88, 0.96]] * N, dtype=torch.float32, device=D.device))
    for e in (V, T, D, fresh):
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 4: unwritten images

def test_an_index_outside_the_rows_leaves_its_image_unwritten():
    """index entries of -1 and n_rows: those images keep the sentinel in all three layers, the others are right; a buffer's rows and the live rows, one chunk and
    chunks of two"""
    A, B = stepped(U, 3), stepped(U, 9, act_seed=7)
    rows = A.get_state()
    index = [0, -1, 2, N, 1]
    good, bad = [0, 2, 4], [1, 3]
    for chunk in (0, 2):
        for drawer, src, owner in ((B, rows, A), (A, None, A)):
            drawer.lib.rp_debug_render_states_chunk(drawer.h, chunk)
            for w, h in SIZES:
                out = {'rgb': torch.empty((5, h, w, 3), dtype=torch.uint8, device=A.device), 'depth': torch.empty((5, h, w), dtype=torch.float32, device=A.device),
                       'segmentation': torch.empty((5, h, w), dtype=torch.int32, device=A.device)}
                fill_sentinel(out)
                got = drawer.render_states(src, w, h, index=i32(drawer, index), out=out)
                want = owner.render_layers(width=w, height=h)
                torch.cuda.synchronize()
                for k in ALL:
                    assert got[k] is out[k]
                    assert is_sentinel(k, out[k][bad]), (chunk, w, h, k)
                    assert same_bytes(out[k][good], want[k][[index[i] for i in good]]), (chunk, w, h, k)
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5: goals

def goal_of(env, pos):
    """the achieved-goal vector whose words are those of kinematics rows `pos`: per object its position (and quaternion where the id's goal holds it), then on play
    ids the drawer's y, door, button, dial - the words a sub-goal overwrites"""
    names = list(env.kinematics_names['pos'])
    n_ag = env.dims['achieved_goal']
    objects = [nm[:-2] for nm in names if nm.endswith('.x') and nm != 'drawer.x']
    play = 'drawer.x' in names
    per = (n_ag - (4 if play else 0)) // max(len(objects), 1)
    assert per in (3, 7)
    cols = []
    for b in objects:
        cols += [names.index('%s.%s' % (b, c)) for c in ('x', 'y', 'z', 'qx', 'qy', 'qz', 'qw')[:per]]
    if play:
        cols += [names.index(c) for c in ('drawer.y', 'door', 'button', 'dial')]
    assert len(cols) == n_ag
    return pos[:, cols].contiguous()


def moved(env, pos, changes):
    """kinematics rows with some columns replaced: {name: value or [N] values}"""
    names = list(env.kinematics_names['pos'])
    p = pos.clone()
    for nm, v in changes.items():
        p[:, names.index(nm)] = torch.as_tensor(v, dtype=torch.float32, device=pos.device)
    return p


def source_and_twin(gid):
    """A in a state after 30 steps with the button released (0.04: the globe is white), a twin T of the same id, and a third handle B that draws"""
    A, T, B = stepped(gid, 3), make(gid, N, 3), make(gid, N, 21)
    T.reset()
    B.reset()
    if 'button' in A.kinematics_names['pos']:
        A.set_kinematics(pos=moved(A, A.get_kinematics()['pos'], {'button': 0.04}))
    return A, T, B


PLAY_MOVES = {'block': {'block.x': [-0.1, 0.0, 0.1, 0.15], 'block.y': 0.2, 'block.z': 0.12}, 'drawer': {'drawer.y': [-0.1, -0.05, 0.05, 0.1]},
              'door': {'door': [0.02, 0.06, 0.1, 0.14]}, 'button': {'button': [0.0, 0.01, 0.02, 0.0]}, 'dial': {'dial': [0.5, 1.5, 2.5, 3.0]}}


def zoom_camera(env):
    """a camera close over the table: some 2 cm per pixel at 33 x 20 and 4 cm at 17 x 16, so that a 5 cm block cannot fall between the pixel centres"""
    return env.camera(target=(0.0, 0.15, 0.07), distance=0.7)


def solid_cases(env, gid, moves):
    """every move of `moves` alone: the solid image of A's rows with the moved words as the goal equals the plain image of the twin row that holds those words (made
    on T with set_kinematics), drawn by B, in all three layers, both sizes, fixed and gripper camera"""
    A, T, B = env
    rows = A.get_state()
    pos = A.get_kinematics()['pos']
    for what, changes in moves.items():
        p = moved(A, pos, changes)
        T.set_state(rows)
        T.set_kinematics(pos=p)
        twin_rows = T.get_state()
        assert not same_bytes(twin_rows, rows)
        for sz in SIZES:
            for cname, cam in (('fixed', {}), ('gripper', dict(camera=A.camera(gripper=True)))):
                want = B.render_states(twin_rows, *sz, **cam)
                got = B.render_states(rows, *sz, goal=goal_of(A, p), goal_mode='solid', **cam)
                torch.cuda.synchronize()
                assert_same(got, want, (gid, what, sz, cname))


def assert_the_block_moves(env, changes, name='block'):
    """not a no-op: seen from close by, the solid image's depth and segmentation differ from the plain one's, and the moved block's collider is in the segmentation"""
    A, T, B = env
    rows, pos = A.get_state(), A.get_kinematics()['pos']
    cam = zoom_camera(A)
    block = A.visual_names.index(name)
    for w, h in SIZES:
        plain = B.render_states(rows, w, h, camera=cam)
        solid = B.render_states(rows, w, h, camera=cam, goal=goal_of(A, moved(A, pos, changes)), goal_mode='solid')
        torch.cuda.synchronize()
        assert not same_bytes(solid['segmentation'], plain['segmentation']) and not same_bytes(solid['depth'], plain['depth']), (w, h)
        assert bool(((solid['segmentation'] != -1) & ((solid['segmentation'] & 0xFF) == block)).any()), (w, h)


def test_a_ghost_goal_is_render_layers_sub_goal():
    A, T, B = source_and_twin(U)
    rows = A.get_state()
    goal = goal_of(A, moved(A, A.get_kinematics()['pos'], {**PLAY_MOVES['block'], **PLAY_MOVES['drawer'], **PLAY_MOVES['door']}))
    for w, h in SIZES:
        for cname, cam in (('fixed', {}), ('gripper', dict(camera=A.camera(gripper=True)))):
            want = A.render_layers(width=w, height=h, sub_goal=goal, **cam)
            for mode in ({}, dict(goal_mode='ghost')):
                assert_same(B.render_states(rows, w, h, goal=goal, **mode, **cam), want, ('ghost', w, h, cname))
            nogoal = A.render_layers(width=w, height=h, **cam)
            assert same_bytes(want['depth'], nogoal['depth']) and same_bytes(want['segmentation'], nogoal['segmentation'])
    zoom = dict(width=33, height=20, camera=zoom_camera(A))
    assert not same_bytes(A.render_layers(sub_goal=goal, **zoom)['rgb'], A.render_layers(**zoom)['rgb'])          # (the ghosts show)
    for e in (A, T, B):
        e.close()


def test_a_solid_goal_is_the_image_of_the_row_with_the_goal_s_words():
    """each goal entry moved alone - block, drawer, door, button, dial: the solid image equals, in all three layers, the plain image of a twin row made by writing
    the same words with set_kinematics; the block's move shows in the segmentation; a button pressed in the goal draws the globe in its "on" colour"""
    env = source_and_twin(U)
    A, T, B = env
    solid_cases(env, U, PLAY_MOVES)
    assert_the_block_moves(env, PLAY_MOVES['block'])
    # the globe: a camera that looks at it from outside the workspace (the static sphere of radius 0.03 at (-0.25, 0.45, 0.24)); released = white, pressed in
    # the goal = red
    cam = A.camera(target=(-0.25, 0.45, 0.24), distance=0.45, yaw=-90.0, pitch=-40.0)
    globe = A.visual_names.index('globe')
    rows, pos = A.get_state(), A.get_kinematics()['pos']
    for w, h in SIZES:
        off = B.render_states(rows, w, h, camera=cam)
        on = B.render_states(rows, w, h, camera=cam, goal=goal_of(A, moved(A, pos, PLAY_MOVES['button'])), goal_mode='solid')
        torch.cuda.synchronize()
        for e in range(N):
            px = (on['segmentation'][e] & 0xFF) == globe
            px &= on['segmentation'][e] != -1
            assert bool(px.any()), (w, h, e)
            c_on, c_off = on['rgb'][e][px].int(), off['rgb'][e][px].int()
            assert bool(((c_on[:, 0] > 0) & (c_on[:, 1] == 0) & (c_on[:, 2] == 0)).all()), (w, h, e)          # red: (1, 0, 0) shaded
            assert bool(((c_off[:, 0] == c_off[:, 1]) & (c_off[:, 1] == c_off[:, 2]) & (c_off[:, 0] > 0)).all()), (w, h, e)          # white: (1, 1, 1) shaded
    for e in env:
        e.close()


def test_a_solid_goal_on_the_other_ids():
    """pandaPick-v0 (a goal of the block's position alone), the wide build with its second object, and UR5Reach-v0, which has no object: the solid image is the
    plain one"""
    env = source_and_twin(P)
    solid_cases(env, P, {'block': {'block.x': [-0.1, 0.0, 0.1, 0.15], 'block.z': 0.15}})
    assert_the_block_moves(env, {'block.x': [-0.1, 0.0, 0.1, 0.15], 'block.y': 0.15, 'block.z': 0.15})
    for e in env:
        e.close()
    env = source_and_twin(W)
    solid_cases(env, W, {'block2': {'block2.x': [-0.1, 0.0, 0.1, 0.15], 'block2.y': 0.2, 'block2.z': 0.15}, 'both': {'block.x': 0.1, 'block2.x': -0.1, 'dial': 2.0}})
    assert_the_block_moves(env, {'block2.x': [-0.1, 0.0, 0.1, 0.15], 'block2.y': 0.2, 'block2.z': 0.15}, 'block2')
    for e in env:
        e.close()
    A, B = stepped(R, 3), make(R, N, 21)
    B.reset()
    rows = A.get_state()
    goal = torch.tensor([[0.1, 0.1, 0.1]] * N, dtype=torch.float32, device=A.device)
    assert A.dims['achieved_goal'] == 3
    for w, h in SIZES:
        want = A.render_layers(width=w, height=h)
        for mode in ('solid', 'ghost'):
            assert_same(B.render_states(rows, w, h, goal=goal, goal_mode=mode), want, (R, mode, w, h))
    A.close()
    B.close()


def test_goal_images_draw_every_live_env_at_its_goal_with_its_own_visuals():
    env = stepped(U, 3)
    env.set_visuals(**visuals_values(env, 4))
    obs = env.calc_state()
    goal = obs['desired_goal']
    assert tuple(goal.shape) == (N, env.dims['achieved_goal'])
    before = env.get_state().clone()
    ident = i32(env, [0, 1, 2, 3])
    for w, h in SIZES:
        for cam in ({}, dict(cameras=cams(env, N)), dict(camera=env.camera(gripper=True), depth='metres', layers=('depth', 'rgb'))):
            got = env.goal_images(goal, w, h, **cam)
            want = env.render_states(None, w, h, goal=goal, goal_mode='solid', visuals=ident, **cam)
            torch.cuda.synchronize()
            assert set(got) == set(want) == set(cam.get('layers', ALL))
            for k in got:
                assert same_bytes(got[k], want[k]), (w, h, k)
        zoom = zoom_camera(env)
        assert not same_bytes(env.goal_images(goal, w, h, camera=zoom)['segmentation'], env.render_layers(width=w, height=h, camera=zoom)['segmentation'])      # (the goal is not where the scene is)
    assert same_bytes(env.get_state(), before)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 6: with images in the step

def test_a_draw_that_grows_the_pose_table_between_two_image_steps():
    """while set_image_obs is in force (the pose table holds N envs), a render_states of 7 > N images in one chunk grows the table between two steps: the next
    step's images still equal a twin's that never drew stored rows"""
    A, T = make(U, N, 3), make(U, N, 3)
    acts = actions(A, 4, 5)
    for e in (A, T):
        e.set_image_obs(width=33, height=20, layers=ALL)
        e.reset()
        e.step(acts[0])
    rows = A.get_state().clone()
    A.lib.rp_debug_render_states_chunk(A.h, 0)
    drawn = A.render_states(rows, 17, 16, index=i32(A, [2, 0, 2, 3, 1, 1, 0]))
    want = A.render_layers(width=17, height=16)
    assert_same(drawn, {k: want[k][[2, 0, 2, 3, 1, 1, 0]] for k in ALL}, 'seven images')
    for t in (1, 2):
        oa, _, _, _ = A.step(acts[t])
        ot, _, _, _ = T.step(acts[t])
        torch.cuda.synchronize()
        for k in ('img', 'depth', 'segmentation'):
            assert same_bytes(oa[k], ot[k]), (t, k)
        A.render_states(rows, 17, 16, index=i32(A, [1, 1, 0, 3, 2]))
    assert same_bytes(A.get_state(), T.get_state())
    A.close()
    T.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# 7: refusals

def test_bad_arguments_are_refused_with_their_cause_and_nothing_is_written():
    """every RP_ERR_ARG case of the header at the ABI, with its message; after each one the outputs still hold the sentinel"""
    env = stepped(U, 3, steps=2)
    w, h = SIZES[0]
    m = 3
    out = {'rgb': torch.empty((m, h, w, 3), dtype=torch.uint8, device=env.device), 'depth': torch.empty((m, h, w), dtype=torch.float32, device=env.device),
           'segmentation': torch.empty((m, h, w), dtype=torch.int32, device=env.device)}
    fill_sentinel(out)
    rgb, dep, seg = (C.c_void_p(out[k].data_ptr()) for k in ALL)
    rows = env.get_state()
    stride = 4 * rows.stride(0)
    index = i32(env, [0, 1, 2])
    cam, crows = env.camera(), cams(env, m)
    from roboticsplayroompybullet_amd import _lib

    def call(src='rows', row_stride=stride, n_rows=N, idx=None, m=m, camera=None, cam_rows=None, near=0.01, far=10.0, mode=0, width=w, height=h, outs=(rgb, dep, seg),
             goal_mode=0):
        s = None
        if src is not None:
            s = C.byref(_lib.RpStateRows(C.c_void_p(rows.data_ptr()) if src == 'rows' else None, row_stride, n_rows, C.c_void_p(idx.data_ptr()) if idx is not None else None,
                                         None))
        env._call('rp_render_states', s, m, C.byref(camera) if camera is not None else None, C.c_void_p(cam_rows.data_ptr()) if cam_rows is not None else None, near, far,
                  mode, width, height, *outs, None, goal_mode, None)

    bad_fov, bad_mode, bad_aspect = env.camera(), env.camera(), env.camera()
    bad_fov.fov_deg, bad_mode.mode, bad_aspect.aspect = 180.0, 2, 0.0
    cases = {'src is NULL': dict(src=None), 'm < 1': dict(m=0), 'm < 1 ': dict(m=-3), 'row_stride < 512': dict(row_stride=508),
             'row_stride is not a multiple of 4': dict(row_stride=stride + 2), 'n_rows < 1': dict(n_rows=0), 'm exceeds n_rows': dict(m=N + 1),
             'm exceeds n_rows ': dict(n_rows=2), 'm exceeds the handle\'s envs': dict(src='live', m=N + 1), 'no output layer': dict(outs=(None, None, None)),
             'both cam and cam_rows': dict(camera=cam, cam_rows=crows), 'unknown goal_mode': dict(goal_mode=2), 'unknown goal_mode ': dict(goal_mode=-1),
             'bad image size': dict(width=0), 'bad image size ': dict(height=4097), 'bad camera': dict(camera=bad_fov), 'bad camera ': dict(camera=bad_mode),
             'bad camera  ': dict(camera=bad_aspect), 'near_plane <= 0': dict(near=0.0), 'far_plane <= near_plane': dict(near=1.0, far=1.0), 'unknown depth mode': dict(mode=2)}
    for cause, c in cases.items():
        with pytest.raises(RuntimeError, match=r'rp_render_states failed \(-1\): rp_render_states: ' + re.escape(cause.strip())):
            call(**c)
    torch.cuda.synchronize()
    for k in ALL:
        assert is_sentinel(k, out[k]), k
    # the wrapper's own refusals name the call and come before the library: a goal of the wrong shape, out tensors of the wrong shape, an index beside its visuals
    for kw in (dict(goal=torch.zeros((m, 3), device=env.device)), dict(out={'rgb': out['rgb'][:2]}), dict(visuals=i32(env, [0, 1])), dict(index=i32(env, []))):
        with pytest.raises(ValueError, match='render_states'):
            env.render_states(rows, w, h, **{'index': index, **kw})
    for k in ALL:
        assert is_sentinel(k, out[k]), k
    # ... and the right call still draws, live rows beyond N included through an index
    call(idx=index)
    call(src='live', idx=index, m=m)
    torch.cuda.synchronize()
    want = env.render_layers(width=w, height=h)
    for k in ALL:
        assert same_bytes(out[k], want[k][:m]), k
    assert env.lib.rp_debug_render_states_chunk(env.h, -1) == -1
    env.close()
