"""Per-env colours, light and background of the camera images (rp_get_visuals_dims / rp_set_visuals / rp_get_visuals) on a GPU-less host: declared in
include/rp_playroom.h, exported by both libraries together with their kernels, mirrored in _lib and VecPlayEnv; the collider names against the bake and against
dynamics_names; the host-side value checks; and the float64 reference of tests/visual_cases.py against camera_cases' own at the default values, with what one colour and
the background may change."""
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest

from abi_decl import REPO, TABLE_KERNELS, assert_exported_by_both_libraries, decl as _decl, header as _header

NEW = ('rp_get_visuals_dims', 'rp_set_visuals', 'rp_get_visuals')
KINDS = ('U', 'R', 'P', 'Q', 'V', 'W')


def test_entry_points_are_declared():
    src = _header()
    assert _decl(src, 'rp_get_visuals_dims') == 'rp_handle h , int32_t* n_col'
    assert _decl(src, 'rp_set_visuals') == ('rp_handle h , const float* colour , const float* light , const float* background , int32_t rows , '
                                            'const uint8_t* mask , void* stream')
    assert _decl(src, 'rp_get_visuals') == 'rp_handle h , float* colour , float* light , float* background , void* stream'


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(NEW, (b'k_collider_poses', b'k_render_layers') + TABLE_KERNELS)
    vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)
    n_args = {name: len(_decl(_header(), name).split(' , ')) for name in NEW}
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_get_visuals_dims.argtypes == [vp, ip]
        assert lib.rp_set_visuals.argtypes == [vp, vp, vp, vp, ctypes.c_int32, vp, vp]
        assert lib.rp_get_visuals.argtypes == [vp, vp, vp, vp, vp]
        for name in NEW:          # the binding's arity is the declaration's
            assert len(getattr(lib, name).argtypes) == n_args[name], name
        assert lib.rp_set_visuals(None, None, None, None, 1, None, None) == -1          # RP_ERR_ARG for a NULL handle, before anything is touched
        assert lib.rp_get_visuals(None, None, None, None, None) == -1
        assert lib.rp_get_visuals_dims(None, None) == -1


def test_vec_env_has_the_visuals_methods():
    from roboticsplayroompybullet_amd import VecPlayEnv
    assert isinstance(inspect.getattr_static(VecPlayEnv, 'visual_names'), property)
    assert list(inspect.signature(VecPlayEnv.get_visuals).parameters) == ['self']
    p = inspect.signature(VecPlayEnv.set_visuals).parameters
    assert list(p) == ['self', 'colour', 'light', 'background', 'mask']
    assert all(p[k].default is None for k in ('colour', 'light', 'background', 'mask'))
    p = inspect.signature(VecPlayEnv.set_colour).parameters
    assert list(p) == ['self', 'name', 'rgb', 'mask'] and p['mask'].default is None
    assert 'record_images' in VecPlayEnv.set_visuals.__doc__


@pytest.mark.parametrize('kind', KINDS)
def test_visual_names_follow_the_bake(kind):
    """one name per collider, in collider order: the name dynamics_names gives the collider's collision object (the bake's collider -> object map); an object with
    several colliders repeats its name"""
    from roboticsplayroompybullet_amd.vec_env import dynamics_names, visual_names
    mdl = next(m for m in json.load(open(os.path.join(REPO, 'roboticsplayroompybullet_amd', 'assets', 'models.json')))['models'] if m['kind'] == kind)
    names = visual_names(kind)
    assert isinstance(names, tuple) and len(names) == len(mdl['col'])
    objects = dynamics_names(kind)['friction']
    for c, col in enumerate(mdl['col']):
        assert names[c] == objects[col['obj']], (c, names[c])
    assert set(names) == set(objects)
    per_object = np.bincount([col['obj'] for col in mdl['col']])
    assert all(names.count(objects[k]) == per_object[k] for k in range(len(objects)))
    if kind in ('U', 'V', 'W'):
        assert names.count('drawer') > 1 and names.count('block') >= 1


def test_host_values_are_checked():
    import torch
    from roboticsplayroompybullet_amd.vec_env import check_visual_values
    assert check_visual_values('colour', [0.0, 0.5, 1.0]).tolist() == [0.0, 0.5, 1.0]
    assert check_visual_values('colour', np.zeros((4, 7, 3))).dtype == torch.float32
    assert check_visual_values('background', [1.0, 0.0, 0.25]).tolist() == [1.0, 0.0, 0.25]
    assert check_visual_values('light', [0.0, 0.0, 2.0, 0.0, 3.0]).tolist() == [0.0, 0.0, 1.0, 0.0, 3.0]          # ambient and diffuse have no upper bound
    bad = {'colour': ([0.0, math.nan, 0.0], [0.0, 1.5, 0.0], [-0.1, 0.0, 0.0], [0.5, 0.5], np.zeros((3, 4)), 0.5),
           'background': ([math.inf, 0.0, 0.0], [0.0, 0.0, 1.5], [0.0] * 5),
           'light': ([1.0, -2.0, 3.0, -0.1, 0.55], [1.0, -2.0, 3.0, 0.45, -0.1], [0.0, 0.0, 0.0, 0.45, 0.55], [1.0, -2.0, 3.0], [math.nan, 0.0, 1.0, 0.45, 0.55],
                     torch.tensor([[1.0, 0.0, 0.0, 0.4, 0.5], [0.0, 0.0, 0.0, 0.4, 0.5]]))}
    for what, values in bad.items():
        for v in values:
            with pytest.raises(ValueError):
                check_visual_values(what, v)


def test_a_direction_is_normalised_in_float64():
    """a host direction comes out as a unit vector: every component within 8e-8 of the float64 unit vector - 5e-8 from the seven decimals it is kept to, 3e-8 from
    the float32 cast of a number below 1 - whatever its length, a batch row by row; an axis stays an axis exactly"""
    from roboticsplayroompybullet_amd.vec_env import LIGHT_DECIMALS, check_visual_values
    assert LIGHT_DECIMALS == 7
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.normal(size=(500, 3)) * rng.uniform(1e-3, 1e3, (500, 1)), rng.uniform(0, 2, (500, 2))], axis=1)
    got = check_visual_values('light', v).numpy()
    unit = v[:, :3] / np.linalg.norm(v[:, :3], axis=1, keepdims=True)
    assert np.abs(got[:, :3].astype(np.float64) - unit).max() <= 8e-8
    assert np.abs(np.linalg.norm(got[:, :3].astype(np.float64), axis=1) - 1.0).max() <= 1.4e-7          # (sqrt(3) * 8e-8)
    assert got[:, 3:].tobytes() == v[:, 3:].astype(np.float32).tobytes()
    rows = check_visual_values('light', [[10.0, -20.0, 30.0, 0.45, 0.55], [0.0, 0.0, -5.0, 0.1, 0.2]]).numpy()
    assert rows[0].tobytes() == check_visual_values('light', [1.0, -2.0, 3.0, 0.45, 0.55]).numpy().tobytes()
    assert rows[1].tolist() == [0.0, 0.0, -1.0, np.float32(0.1), np.float32(0.2)]


def test_the_default_direction_is_what_normalising_1_m2_3_gives():
    """check_visual_values normalises (1, -2, 3) to the default direction's float32 values exactly: the library's default row is rp_render.cuh's literals
    (0.2672612f, -0.5345225f, 0.8017837f), which the images of every earlier version were drawn with and which stay.  Those are (1, -2, 3) / sqrt(14) at seven decimals,
    and two of them are one ulp below the float32 nearest to the true value (0x3e88d676 against 0x3e88d677, 0x3f4d41b2 against 0x3f4d41b3), so the float64 unit vector
    cast to float32 alone does not give them; kept to the same seven decimals before the cast (vec_env.LIGHT_DECIMALS) it does."""
    from roboticsplayroompybullet_amd.vec_env import check_visual_values
    import visual_cases as vc
    got = check_visual_values('light', [1.0, -2.0, 3.0, 0.45, 0.55]).numpy()
    print('normalised', got.view(np.uint32), 'default', vc.DEVICE_LIGHT.view(np.uint32))
    assert got.tobytes() == vc.DEVICE_LIGHT.tobytes(), (got.view(np.uint32), vc.DEVICE_LIGHT.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference

def _scene():
    pytest.importorskip('scipy')
    import camera_cases as cc
    o = cc.oracle_of(cc.U, 'scene')
    return cc, o, cc.host_camera('default', o)


def test_reference_at_the_defaults_is_camera_cases_own():
    """reference_rgb with the table's colours, camera_cases' LIGHT with 0.45 / 0.55 and its BACKGROUND equals reference_layers' rgb in every bit (== in float64), and so
    do who, seg and tint: on (U, 'scene', default camera, 33 x 50) and on U's combined sub-goal with its ghosts"""
    import visual_cases as vc
    cc, o, cam = _scene()
    w, h = 33, 50
    for state, ghosted in (('scene', False), ('reset', True)):
        o = cc.oracle_of(cc.U, state)
        cam = cc.host_camera('default', o)
        ghosts = [cc.ghost_records(cc.sub_goal_oracle(cc.U, o, cc.sub_goal_vector(cc.U, o, cc.GHOST_COMBINED[cc.U])))] if ghosted else None
        want = cc.reference_layers(o, cam, w, h, ghosts=ghosts)
        got = vc.reference_rgb(o, cam, w, h, vc.table_colours(o), vc.DEFAULT_LIGHT, vc.DEFAULT_BACKGROUND, ghosts=ghosts)
        assert (got['rgb'] == want['rgb']).all()
        for k in ('who', 'seg', 'tint'):
            assert np.array_equal(got[k], want[k]), k
        assert (want['who'] >= 0).mean() > 0.05 and (not ghosted or want['tint'].sum() > 0)
        assert np.array_equal(got['ghost'] >= 0, want['tint'])


def test_one_colour_changes_only_its_own_pixels():
    """another colour for one collider changes only pixels whose solid hit or whose ghost is that collider - and a toggle collider's colour changes nothing"""
    import visual_cases as vc
    cc, o, cam = _scene()
    w, h = 33, 50
    o = cc.oracle_of(cc.U, 'reset')
    cam = cc.host_camera('default', o)
    ghosts = [cc.ghost_records(cc.sub_goal_oracle(cc.U, o, cc.sub_goal_vector(cc.U, o, cc.GHOST_COMBINED[cc.U])))]
    base = vc.table_colours(o)
    bare = vc.reference_rgb(o, cam, w, h, base, vc.DEFAULT_LIGHT, vc.DEFAULT_BACKGROUND, ghosts=ghosts)
    seen = [c for c in np.unique(bare['who']) if c >= 0]
    block = int(ghosts[0][6][0])
    assert block in np.unique(bare['ghost'])
    toggles = [c for c in seen if c in vc.toggle_colliders(o)]
    assert toggles
    for c in seen[:2] + seen[-2:] + toggles + [block]:          # (a few: arm links, fixtures, the globe or the grill, the block with its ghost)
        colour = base.copy()
        colour[c] = 1.0 - colour[c] * 0.5
        got = vc.reference_rgb(o, cam, w, h, colour, vc.DEFAULT_LIGHT, vc.DEFAULT_BACKGROUND, ghosts=ghosts)
        changed = (got['rgb'] != bare['rgb']).any(axis=2)
        own = (bare['who'] == c) | (bare['ghost'] == c)
        assert not (changed & ~own).any(), c
        if c in vc.toggle_colliders(o):
            assert not changed.any(), c
        else:
            assert changed.any(), c
        for k in ('who', 'seg', 'tint', 'ghost'):
            assert np.array_equal(got[k], bare[k])


def test_the_background_changes_only_misses():
    import visual_cases as vc
    cc, o, cam = _scene()
    w, h = 33, 50
    bare = vc.reference_rgb(o, cam, w, h, vc.table_colours(o), vc.DEFAULT_LIGHT, vc.DEFAULT_BACKGROUND)
    got = vc.reference_rgb(o, cam, w, h, vc.table_colours(o), vc.DEFAULT_LIGHT, [0.1, 0.7, 0.2])
    changed = (got['rgb'] != bare['rgb']).any(axis=2)
    assert np.array_equal(changed, bare['who'] < 0) and changed.any() and not changed.all()
    assert (got['rgb'][changed] == [0.1, 0.7, 0.2]).all()


def test_random_visuals_are_the_rows_the_gpu_test_needs():
    import visual_cases as vc
    v = vc.random_visuals(3, 52, 7)
    assert v['colour'].shape == (3, 52, 3) and v['light'].shape == (3, 5) and v['background'].shape == (3, 3)
    assert all(a.dtype == np.float32 for a in v.values())
    assert v['light'][0].tolist() == [0.0, 0.0, -1.0, np.float32(0.3), np.float32(0.7)]
    assert abs(np.linalg.norm(v['light'][1, :3].astype(np.float64)) - 1.0) > 0.5          # used as it stands: a length the library must not normalise away
    assert v['light'][2, 3] + v['light'][2, 4] > 1.0                                      # saturates: exercises the clamp
    assert len({tuple(r) for r in v['background']}) == 3 and len({tuple(r) for r in v['light']}) == 3
    assert ((v['colour'] >= 0) & (v['colour'] < 1)).all() and not np.array_equal(v['colour'][0], v['colour'][1])
