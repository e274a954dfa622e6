"""Camera depth and segmentation layers and per-env cameras (rp_render_layers, rp_debug_render_cull) on a GPU-less host: declared in the headers, exported by
both libraries together with the kernel, mirrored in _lib and VecPlayEnv; the host arithmetic and value checks of cameras(); the segmentation helper."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from abi_decl import REPO, assert_exported_by_both_libraries, decl as _decl, header as _header


def test_entry_point_is_declared():
    src = _header()
    assert _decl(src, 'rp_render_layers') == ('rp_handle h , const rp_camera* cam , const float* cam_rows , float near_plane , float far_plane , int32_t depth_mode , '
                                              'int32_t width , int32_t height , int32_t first_env , int32_t num_envs , uint8_t* rgb , float* depth , '
                                              'int32_t* segmentation , const float* sub_goal , const float* ghost_arm , void* stream')
    assert re.search(r'enum rp_depth_mode \{ RP_DEPTH_BUFFER = 0, RP_DEPTH_METRES = 1 \};', src)
    # the older entry points keep their signatures
    assert _decl(src, 'rp_render_ex') == ('rp_handle h , const rp_camera* cam , int32_t width , int32_t height , int32_t first_env , int32_t num_envs , uint8_t* rgb , '
                                          'const float* sub_goal , const float* ghost_arm , void* stream')
    assert _decl(src, 'rp_render') == ('rp_handle h , const rp_camera* cam , int32_t width , int32_t height , int32_t first_env , int32_t num_envs , uint8_t* rgb , '
                                       'const float* sub_goal , void* stream')
    assert _decl(src, 'rp_ray_test') == ('rp_handle h , const float* from , const float* to , int32_t k , float* hit_fraction , int32_t* collider , int32_t* link , '
                                         'float* hit_position , float* hit_normal , void* stream')
    dbg = open(os.path.join(REPO, 'include', 'rp_playroom_debug.h')).read()
    dbg = re.sub(r'/\*.*?\*/', '', dbg, flags=re.S)
    assert re.search(r'int rp_debug_render_cull\(rp_handle h, int32_t on\);', dbg)


def test_entry_point_is_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(('rp_render_layers',), (b'k_render_layers', b'k_collider_poses'))
    assert 'rp_debug_render_cull' in _lib.DEBUG_EXPORTS and 'rp_debug_render_cull' not in _lib.EXPORTS
    assert (_lib.DEPTH_BUFFER, _lib.DEPTH_METRES) == (0, 1)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_render_layers.argtypes == [vp, ctypes.POINTER(_lib.RpCamera), vp, f32, f32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        assert len(lib.rp_render_layers.argtypes) == 16 == len(_decl(_header(), 'rp_render_layers').split(' , '))
        assert lib.rp_debug_render_cull.argtypes == [vp, i32]
        assert hasattr(lib, 'rp_debug_render_cull')
        assert lib.rp_debug_render_cull(None, 1) == -1          # RP_ERR_ARG without a handle; needs no GPU
        lib.rp_version.restype = ctypes.c_char_p
        assert lib.rp_version().startswith(b'rp_playroom 0.5.2 ')


def test_vec_env_has_the_layer_methods():
    from roboticsplayroompybullet_amd import VecPlayEnv, vec_env
    p = inspect.signature(VecPlayEnv.render_layers).parameters
    assert list(p) == ['self', 'width', 'height', 'envs', 'camera', 'cameras', 'layers', 'depth', 'near', 'far', 'sub_goal', 'ghost_arm', 'out']
    assert (p['width'].default, p['height'].default, p['layers'].default, p['depth'].default, p['near'].default, p['far'].default) == \
        (200, 200, ('rgb', 'depth', 'segmentation'), 'buffer', 0.01, 10.0)
    assert all(p[k].default is None for k in ('envs', 'camera', 'cameras', 'sub_goal', 'ghost_arm', 'out'))
    p = inspect.signature(VecPlayEnv.cameras).parameters
    assert list(p) == ['self', 'target', 'distance', 'yaw', 'pitch', 'roll', 'fov', 'aspect']
    q = inspect.signature(VecPlayEnv.camera).parameters          # the same defaults as the one-camera constructor: the reference's fixed camera
    assert all(p[k].default == q[k].default for k in list(p)[1:])
    assert isinstance(inspect.getattr_static(VecPlayEnv, 'unpack_segmentation'), staticmethod)
    assert VecPlayEnv.unpack_segmentation is vec_env.unpack_segmentation
    # render is as it was
    assert list(inspect.signature(VecPlayEnv.render).parameters) == ['self', 'mode', 'width', 'height', 'envs', 'camera', 'sub_goal', 'out', 'ghost_arm']


def test_camera_rows_are_the_references_camera():
    """cameras()' host arithmetic against the numpy restatement of computeViewMatrixFromYawPitchRoll in tests/test_gpu_render.py, and against
    rp_camera_from_yaw_pitch_roll itself (host code of the library, no GPU), bit for bit"""
    import torch
    from test_gpu_render import default_camera
    from roboticsplayroompybullet_amd import _lib
    from roboticsplayroompybullet_amd.vec_env import camera_rows
    row = camera_rows()
    assert row.shape == (1, 11) and row.dtype == torch.float32 and not row.is_cuda
    eye, target, up = default_camera()
    np.testing.assert_allclose(row[0, 0:3].numpy(), eye, atol=1e-6)
    np.testing.assert_allclose(row[0, 3:6].numpy(), target, atol=1e-7)
    np.testing.assert_allclose(row[0, 6:9].numpy(), up, atol=1e-6)
    assert row[0, 9:].tolist() == [50.0, 1.0]
    # three different cameras, each argument a scalar or a length-3 array, against the C function
    yaw, dist, fov = np.array([-30.0, 20.0, 75.0]), torch.tensor([1.3, 2.0, 0.8]), [50.0, 60.0, 35.0]
    tg = np.array([[0.0, 0.25, 0.0], [0.1, 0.2, 0.05], [-0.2, 0.3, 0.1]])
    rows = camera_rows(target=tg, distance=dist, yaw=yaw, pitch=-40.0, roll=[0.0, 5.0, -10.0], fov=fov, aspect=320 / 240)
    assert rows.shape == (3, 11)
    lib = _lib.load()
    for e in range(3):
        cam = _lib.RpCamera()
        assert lib.rp_camera_from_yaw_pitch_roll((ctypes.c_float * 3)(*tg[e]), float(dist[e]), float(yaw[e]), -40.0, [0.0, 5.0, -10.0][e], ctypes.byref(cam)) == 0
        want = list(cam.eye) + list(cam.target) + list(cam.up) + [np.float32(fov[e]), np.float32(320 / 240)]
        assert rows[e].tolist() == [float(v) for v in want], e
    assert camera_rows(n=4).shape == (4, 11) and bool((camera_rows(n=4) == row).all())
    assert camera_rows(target=[0.0, 0.0, 0.1], yaw=[1.0, 2.0]).shape == (2, 11)


def test_camera_host_values_are_checked():
    from roboticsplayroompybullet_amd.vec_env import camera_rows
    for kw in (dict(fov=0.0), dict(fov=180.0), dict(fov=[50.0, -1.0]), dict(aspect=0.0), dict(aspect=[1.0, -2.0]), dict(distance=0.0), dict(distance=-1.3),
               dict(yaw=float('nan')), dict(pitch=float('inf')), dict(target=[0.0, float('nan'), 0.0]), dict(target=[0.0, 0.0]),
               dict(yaw=[1.0, 2.0], fov=[50.0, 50.0, 50.0]), dict(yaw=[1.0, 2.0], n=3)):
        with pytest.raises(ValueError):
            camera_rows(**kw)
    assert camera_rows(fov=179.0, aspect=0.1, distance=1e-3).shape == (1, 11)


def test_segmentation_unpacks_to_collider_and_link():
    import torch
    from roboticsplayroompybullet_amd import VecPlayEnv
    seg = np.array([-1, 51, 7 | (3 << 24), 0 | (1 << 24), 63 | (12 << 24)], dtype=np.int32)
    for s in (seg, torch.tensor(seg)):
        collider, link = VecPlayEnv.unpack_segmentation(s)
        assert collider.tolist() == [-1, 51, 7, 0, 63] and link.tolist() == [-1, -1, 2, 0, 11]
