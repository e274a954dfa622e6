"""Per-env point clouds (rp_render_points, rp_set_image_points) on a GPU-less host: the struct, the enum and the two entry points declared in include/rp_playroom.h,
exported by both libraries together with k_point_cloud, mirrored in _lib (EXPORTS, RpPointsSpec with the header's field order, the frame constants), the argument
checks that need no device, and VecPlayEnv's host-side checks."""
import ctypes
import inspect
import re

import pytest

from abi_decl import assert_exported_by_both_libraries, decl as _decl, header as _header

FIELDS = ('max_points', 'frame', 'max_depth', 'drop')


def struct_fields(src):
    body = re.search(r'typedef struct rp_points_spec \{(.*?)\} rp_points_spec;', src, flags=re.S).group(1)
    return tuple(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', s.strip()).group(1) for s in body.split(';') if s.strip())


def test_the_header_declares_the_struct_the_enum_and_the_entry_points():
    src = _header()
    assert struct_fields(src) == FIELDS
    assert re.search(r'enum rp_points_frame \{ RP_POINTS_WORLD = 0, RP_POINTS_CAMERA = 1 \};', src)
    assert _decl(src, 'rp_render_points') == ('rp_handle h , const rp_camera* cam , const float* cam_rows , int32_t width , int32_t height , int32_t first_env , '
                                              'int32_t num_envs , const rp_points_spec* spec , uint8_t* rgb , float* depth , int32_t* segmentation , float* xyz , '
                                              'int32_t* point_seg , uint8_t* point_rgb , int32_t* count , void* stream')
    assert _decl(src, 'rp_set_image_points') == ('rp_handle h , int32_t view , const rp_points_spec* spec , float* xyz , int32_t* point_seg , uint8_t* point_rgb , '
                                                 'int32_t* count , float* final_xyz , int32_t* final_point_seg , uint8_t* final_point_rgb , int32_t* final_count')


def test_the_header_states_the_rule_the_costs_and_the_errors():
    import os
    from abi_decl import REPO
    src = open(os.path.join(REPO, 'include', 'rp_playroom.h')).read()
    text = ' '.join(src[src.index('per-env point clouds from the camera views'):src.index('int rp_ray_test')].split())
    for words in ('row-major', 'i = y * width + x', 'segmentation[i] != -1', '& 0xFF', 'max_depth <= 0', 'floor(j * n / P)', '64-bit', 'PADDING', 'NOT capped',
                  'no atomics', 'bit for bit', 'RP_POINTS_CAMERA', 'RP_POINTS_WORLD', 'k_point_cloud', 'Three launches', 'no host wait', 'IN FORCE', 'ONE more',
                  'done != 0', 'drops ALL attachments', 'rp_copy_envs', 'launches exactly what it launched before', 'RP_ERR_ARG', 'RP_DEPTH_METRES'):
        assert words in text, words


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(('rp_render_points', 'rp_set_image_points'), (b'k_point_cloud',))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        spec = ctypes.POINTER(_lib.RpPointsSpec)
        assert lib.rp_render_points.argtypes == [vp, ctypes.POINTER(_lib.RpCamera), vp, i32, i32, i32, i32, spec] + [vp] * 8
        assert lib.rp_set_image_points.argtypes == [vp, i32, spec] + [vp] * 8
        # RP_ERR_ARG for a NULL handle, before anything is touched
        s = _lib.RpPointsSpec(16, 0, 0.0, 0)
        assert lib.rp_render_points(None, None, None, 8, 8, 0, 1, ctypes.byref(s), None, None, None, None, None, None, None, None) == -1
        assert lib.rp_set_image_points(None, 0, ctypes.byref(s), None, None, None, None, None, None, None, None) == -1
        assert lib.rp_version().decode().startswith('rp_playroom 0.5.2 ')


def test_the_ctypes_struct_and_the_constants_are_the_header_s():
    """field order as in the header; the C layout on an LP64 host: two ints, a float, four bytes of padding, the 64-bit mask"""
    from roboticsplayroompybullet_amd import _lib
    assert tuple(n for n, _ in _lib.RpPointsSpec._fields_) == FIELDS == struct_fields(_header())
    types = dict(_lib.RpPointsSpec._fields_)
    assert types == {'max_points': ctypes.c_int32, 'frame': ctypes.c_int32, 'max_depth': ctypes.c_float, 'drop': ctypes.c_uint64}
    assert ctypes.sizeof(_lib.RpPointsSpec) == 24
    assert {n: getattr(_lib.RpPointsSpec, n).offset for n in FIELDS} == {'max_points': 0, 'frame': 4, 'max_depth': 8, 'drop': 16}
    src = _header()
    values = {k: int(v) for k, v in re.findall(r'(RP_POINTS_[A-Z]+) = (\d+)', re.search(r'enum rp_points_frame \{(.*?)\}', src).group(1))}
    assert values == {'RP_POINTS_WORLD': _lib.POINTS_WORLD, 'RP_POINTS_CAMERA': _lib.POINTS_CAMERA} == {'RP_POINTS_WORLD': 0, 'RP_POINTS_CAMERA': 1}
    assert _lib.MAX_POINTS == 65536


def test_vec_env_checks_host_values_and_names_the_view():
    """the host-side checks of render_points and of the `points` key read nothing of the handle: every complaint is a ValueError naming the call and, for a view, the view"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = object.__new__(VecPlayEnv)
    env.h = None
    env.num_envs, env.device, env.autoreset, env.env_id = 5, 'cpu', False, 'UR5PlayAbsRPY1Obj-v0'
    names = env.visual_names
    assert len(names) > 3
    for kw in (dict(n_points=0), dict(n_points=65537), dict(frame='eye'), dict(drop=('no such collider',)), dict(max_depth=float('nan')), dict(drop='table')):
        with pytest.raises(ValueError, match='render_points'):
            env.render_points(8, 8, **{'n_points': 16, **kw})
    # a view's points=... in set_image_views: checked with the view's other values, before anything changes
    ok = dict(width=8, height=8, layers=('depth', 'segmentation'), depth='metres')
    for bad in (dict(layers=('depth',)), dict(layers=('rgb', 'segmentation')), dict(depth='buffer'), dict(points=dict(n=16, colour=True)),
                dict(points=dict(n=0)), dict(points=dict(n=16, frame='eye')), dict(points=dict(n=16, drop=('nothing',))), dict(points=dict(n=16, size=3)),
                dict(points=dict(frame='world')), dict(points=16)):
        with pytest.raises(ValueError, match="set_image_views: view 'wrist': points"):
            env.set_image_views({'img': dict(width=8, height=8), 'wrist': {'points': dict(n=16), **ok, **bad}})
    # set_image_points: no configuration, then set_image_obs' view, then a named view (the tensors are never looked at)
    env.image_views = env.image_obs = env.image_final = env.image_views_final = None
    with pytest.raises(ValueError, match='set_image_points: no image configuration is in force'):
        env.set_image_points(16)
    env.image_obs, env._image_depth = {'depth': None, 'segmentation': None}, 'metres'
    with pytest.raises(ValueError, match='set_image_points: view'):
        env.set_image_points(16, view='wrist')
    for kw in (dict(n=0), dict(n=65537), dict(n=16.0), dict(n=16, frame='eye'), dict(n=16, max_depth=-1.0), dict(n=16, drop=('nothing',)), dict(n=16, colour=True)):
        with pytest.raises(ValueError, match='set_image_points: points'):
            env.set_image_points(**kw)
    for layers, depth in (({'depth': None}, 'metres'), ({'rgb': None, 'segmentation': None}, 'metres'), ({'depth': None, 'segmentation': None}, 'buffer')):
        env.image_obs, env._image_depth = layers, depth
        with pytest.raises(ValueError, match="set_image_points: points need the layers .* with depth='metres'"):
            env.set_image_points(16)
    env.image_obs = None
    env.image_views, env._image_depth = {'img': {'rgb': None}, 'wrist': {'depth': None, 'segmentation': None}}, {'img': 'buffer', 'wrist': 'metres'}
    for view in (None, 'side'):
        with pytest.raises(ValueError, match="set_image_points: view is one of 'img', 'wrist'"):
            env.set_image_points(16, view=view)
    with pytest.raises(ValueError, match="set_image_points: view 'img': points need"):
        env.set_image_points(16, view='img')
    with pytest.raises(ValueError, match="set_image_points: view 'wrist': points need"):
        env.set_image_points(16, view='wrist', colour=True)
    p = inspect.signature(VecPlayEnv.set_image_points).parameters
    assert {k: v.default for k, v in p.items() if k not in ('self', 'n')} == {'frame': 'world', 'max_depth': None, 'drop': (), 'colour': False, 'view': None}
    p = inspect.signature(VecPlayEnv.render_points).parameters
    assert list(p) == ['self', 'width', 'height', 'n_points', 'envs', 'camera', 'cameras', 'frame', 'max_depth', 'drop', 'colour']
    for doc in (VecPlayEnv.render_points.__doc__, VecPlayEnv.set_image_points.__doc__):
        for words in ('count', 'floor(j n / P)', 'padding', 'visual_names'):
            assert words in doc, words
    assert 'set_image_points' in VecPlayEnv.set_image_obs.__doc__ and 'points=dict(' in VecPlayEnv.set_image_views.__doc__
