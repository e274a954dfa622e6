"""Several camera views per env written by the batched step (rp_set_image_views) on a GPU-less host: the struct and the entry point declared in
include/rp_playroom.h as the issue spells them, the merge switch in the debug header, both exported by both libraries together with k_render_views, the ctypes
struct with the header's field order and size, the argument checks that need no device, and VecPlayEnv.set_image_views' host-side checks."""
import ctypes
import os
import re

import pytest

from abi_decl import REPO, assert_exported_by_both_libraries, decl as _decl, header as _header

FIELDS = ('cam', 'cam_rows', 'near_plane', 'far_plane', 'depth_mode', 'width', 'height', 'rgb', 'depth', 'segmentation', 'final_rgb', 'final_depth',
          'final_segmentation')


def struct_fields(src):
    """the member names of rp_image_view, in the header's order"""
    body = re.search(r'typedef struct rp_image_view \{(.*?)\} rp_image_view;', src, flags=re.S).group(1)
    names = []
    for statement in body.split(';'):
        for part in statement.split(','):
            m = re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', part.strip())
            if m:
                names.append(m.group(1))
    return tuple(names)


def test_the_header_declares_the_struct_and_the_entry_point():
    src = _header()
    assert re.search(r'#define\s+RP_MAX_IMAGE_VIEWS\s+4\b', src)
    assert struct_fields(src) == FIELDS
    assert _decl(src, 'rp_set_image_views') == 'rp_handle h , const rp_image_view* views , int32_t n_views'
    dbg = open(os.path.join(REPO, 'include', 'rp_playroom_debug.h')).read()
    assert _decl(re.sub(r'/\*.*?\*/', '', dbg, flags=re.S), 'rp_debug_image_views_merge') == 'rp_handle h , int32_t on'


def test_the_header_states_the_rules():
    src = open(os.path.join(REPO, 'include', 'rp_playroom.h')).read()
    comment = re.findall(r'/\*.*?\*/', src[:src.index('#define RP_MAX_IMAGE_VIEWS')], flags=re.S)[-1]
    text = ' '.join(comment.split())
    for words in ('rp_step and rp_calc_state', 'rp_reset and rp_reset_to', 'RP_ERR_INCOMPLETE', 'k_autoreset_mark', 'done != 0', 'byte for byte', 'rp_render_layers(',
                  'ONE image configuration', 'n_views == 0', 'copied at the call', 'synchronises the device', 'rp_copy_envs', 'rp_destroy', 'k_render_views',
                  'RP_ERR_ARG', 'names the view', 'SUM', '2^31 - 1'):
        assert words in text, words


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(('rp_set_image_views',), (b'k_render_views', b'k_render_layers', b'k_collider_poses'))
    assert 'rp_debug_image_views_merge' in _lib.DEBUG_EXPORTS
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_set_image_views.argtypes == [vp, ctypes.POINTER(_lib.RpImageView), i32]
        assert lib.rp_debug_image_views_merge.argtypes == [vp, i32]
        # RP_ERR_ARG for a NULL handle, before anything is touched
        one = (_lib.RpImageView * 1)()
        assert lib.rp_set_image_views(None, one, 1) == -1
        assert lib.rp_set_image_views(None, None, 0) == -1
        assert lib.rp_debug_image_views_merge(None, 1) == -1


def test_the_ctypes_struct_is_the_header_s():
    """field order as in the header; the size and the offsets of the C layout on an LP64 host: two pointers, two floats, three ints, four bytes of padding, six
    pointers"""
    from roboticsplayroompybullet_amd import _lib
    assert tuple(n for n, _ in _lib.RpImageView._fields_) == FIELDS == struct_fields(_header())
    assert _lib.MAX_IMAGE_VIEWS == 4
    p = ctypes.sizeof(ctypes.c_void_p)
    assert p == 8
    assert ctypes.sizeof(_lib.RpImageView) == 2 * p + 2 * 4 + 3 * 4 + 4 + 6 * p == 88
    offsets = {n: getattr(_lib.RpImageView, n).offset for n in FIELDS}
    assert offsets == {'cam': 0, 'cam_rows': 8, 'near_plane': 16, 'far_plane': 20, 'depth_mode': 24, 'width': 28, 'height': 32, 'rgb': 40, 'depth': 48,
                       'segmentation': 56, 'final_rgb': 64, 'final_depth': 72, 'final_segmentation': 80}
    types = dict(_lib.RpImageView._fields_)
    assert types['cam'] == ctypes.POINTER(_lib.RpCamera)
    assert all(types[n] == ctypes.c_float for n in ('near_plane', 'far_plane')) and all(types[n] == ctypes.c_int32 for n in ('depth_mode', 'width', 'height'))


def test_vec_env_checks_host_values_per_view_and_names_the_view():
    """set_image_views' host-side checks read nothing of the handle: every complaint is a ValueError that names set_image_views and, for a view's values, the view"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = object.__new__(VecPlayEnv)
    env.h = None
    env.num_envs, env.device, env.autoreset = 5, 'cpu', False
    five = {str(i): dict(width=8, height=8) for i in range(5)}
    for bad in ({}, five, [dict(width=8)], 'img'):
        with pytest.raises(ValueError, match='set_image_views'):
            env.set_image_views(bad)
    ok = dict(width=33, height=50)
    for kw in (dict(layers=()), dict(layers=('rgb', 'normals')), dict(depth='metric'), dict(camera=object(), cameras=object()), dict(near=0.0),
               dict(near=1.0, far=1.0), dict(width=0, height=5), dict(height=5000), dict(size=3)):
        with pytest.raises(ValueError, match="set_image_views: view 'wrist'"):
            env.set_image_views({'img': ok, 'wrist': {**ok, **kw}})
    doc = VecPlayEnv.set_image_views.__doc__
    for words in ("obs['views']", "obs['img']", 'terminal_observation', 'image_view_cameras', 'record_images', 'set_image_views(None)', 'render_layers'):
        assert words in doc, words
