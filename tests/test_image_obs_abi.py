"""Camera images written by the batched step (rp_set_image_obs) on a GPU-less host: declared in include/rp_playroom.h as the issue spells it, exported by both
libraries together with the two render kernels, mirrored in _lib with the declaration's arity, refusing a NULL handle before anything is touched, and
VecPlayEnv.set_image_obs with its signature, defaults and the host-side checks it shares with render_layers."""
import ctypes
import inspect

import pytest

from abi_decl import assert_exported_by_both_libraries, decl as _decl, header as _header

DECL = ('rp_handle h , const rp_camera* cam , const float* cam_rows , float near_plane , float far_plane , int32_t depth_mode , int32_t width , int32_t height , '
        'uint8_t* rgb , float* depth , int32_t* segmentation , uint8_t* final_rgb , float* final_depth , int32_t* final_segmentation')


def test_entry_point_is_declared():
    assert _decl(_header(), 'rp_set_image_obs') == DECL


def test_the_header_states_the_rules():
    """the rules a C caller relies on stand in the comment above the declaration: the calls that draw, the order inside rp_step_autoreset, equality with
    rp_render_layers, who owns cam_rows, the cost, switching off, the errors, what is not state and the shared pose table"""
    import os
    import re
    from abi_decl import REPO
    src = open(os.path.join(REPO, 'include', 'rp_playroom.h')).read()
    comment = re.findall(r'/\*.*?\*/', src[:src.index('int rp_set_image_obs(')], flags=re.S)[-1]
    text = ' '.join(comment.split())
    for words in ('rp_step, rp_calc_state', 'rp_reset, rp_reset_to', 'RP_ERR_INCOMPLETE', 'k_autoreset_mark', 'done != 0', 'byte for byte', 'rp_render_layers(',
                  'rp_default_camera', 'caller-owned', 'no host wait', 'no allocation', 'width == 0 && height == 0', 'RP_ERR_ARG', '2^31 - 1', 'rp_copy_envs',
                  'collider-pose table', 'another stream'):
        assert words in text, words


def test_entry_point_is_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(('rp_set_image_obs',), (b'k_collider_poses', b'k_render_layers'))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    n_args = len(DECL.split(' , '))
    assert n_args == 14
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_set_image_obs.argtypes == [vp, ctypes.POINTER(_lib.RpCamera), vp, f32, f32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        assert len(lib.rp_set_image_obs.argtypes) == n_args
        # RP_ERR_ARG for a NULL handle, before anything is touched: switching on and switching off
        assert lib.rp_set_image_obs(None, None, None, 0.01, 10.0, 0, 64, 64, None, None, None, None, None, None) == -1
        assert lib.rp_set_image_obs(None, None, None, 0.0, 0.0, 0, 0, 0, None, None, None, None, None, None) == -1


def test_vec_env_has_set_image_obs():
    from roboticsplayroompybullet_amd import VecPlayEnv
    p = inspect.signature(VecPlayEnv.set_image_obs).parameters
    assert list(p) == ['self', 'width', 'height', 'layers', 'camera', 'cameras', 'depth', 'near', 'far']
    assert {k: v.default for k, v in p.items() if k != 'self'} == {'width': 84, 'height': 84, 'layers': ('rgb',), 'camera': None, 'cameras': None,
                                                                  'depth': 'buffer', 'near': 0.01, 'far': 10.0}
    doc = VecPlayEnv.set_image_obs.__doc__
    for words in ('terminal_observation', 'image_cameras', 'record_images', 'set_image_obs(None)', 'render_layers'):
        assert words in doc, words
    assert 'set_image_obs' in VecPlayEnv.step.__doc__


def test_the_image_keys_of_an_observation():
    """'img' is the rgb tensor or None; depth and segmentation exist only where asked for"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    assert VecPlayEnv._image_keys({'rgb': 1}) == {'img': 1}
    assert VecPlayEnv._image_keys({'depth': 2}) == {'img': None, 'depth': 2}
    assert VecPlayEnv._image_keys({'rgb': 1, 'depth': 2, 'segmentation': 3}) == {'img': 1, 'depth': 2, 'segmentation': 3}


def test_host_values_are_checked_before_the_library_is_called():
    """set_image_obs shares render_layers' host-side checks, which need no handle: each complaint names set_image_obs"""
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = object.__new__(VecPlayEnv)          # (the checks read nothing of the handle)
    env.h = None
    bad = (dict(layers=()), dict(layers=('rgb', 'normals')), dict(depth='metric'), dict(camera=object(), cameras=object()), dict(near=0.0), dict(near=1.0, far=1.0))
    for kw in bad:
        args = dict(layers=('rgb',), depth='buffer', camera=None, cameras=None, near=0.01, far=10.0)
        args.update(kw)
        with pytest.raises(ValueError, match='set_image_obs'):
            env._layer_args('set_image_obs', 5, 33, 50, **args)
    layers, shapes, cams = env._layer_args('set_image_obs', 5, 33, 50, 'depth', 'metres', None, None, 0.01, 10.0)
    assert layers == ('depth',) and cams is None and shapes['depth'][0] == (5, 50, 33) and shapes['rgb'][0] == (5, 50, 33, 3)
