"""Camera images of stored state rows (rp_render_states) on a GPU-less host: the struct, the enum and the entry point declared in include/rp_playroom.h, the debug
hook in rp_playroom_debug.h, both exported by both libraries together with the two kernels, mirrored in _lib (EXPORTS, DEBUG_EXPORTS, RpStateRows with the header's
field order and offsets, the goal modes), the argument check that needs no device, and VecPlayEnv's host-side checks."""
import ctypes
import inspect
import re

import pytest

from abi_decl import assert_exported_by_both_libraries, decl as _decl, header as _header

FIELDS = ('rows', 'row_stride', 'n_rows', 'row_index', 'vis_env')


def struct_fields(src):
    body = re.search(r'typedef struct rp_state_rows \{(.*?)\} rp_state_rows;', src, flags=re.S).group(1)
    return tuple(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', s.strip()).group(1) for s in body.split(';') if s.strip())


def test_the_header_declares_the_struct_the_enum_and_the_entry_point():
    src = _header()
    assert struct_fields(src) == FIELDS
    assert re.search(r'enum rp_goal_mode \{ RP_GOAL_GHOST = 0, RP_GOAL_SOLID = 1 \};', src)
    assert _decl(src, 'rp_render_states') == ('rp_handle h , const rp_state_rows* src , int32_t m , const rp_camera* cam , const float* cam_rows , float near_plane , '
                                              'float far_plane , int32_t depth_mode , int32_t width , int32_t height , uint8_t* rgb , float* depth , '
                                              'int32_t* segmentation , const float* goal , int32_t goal_mode , void* stream')
    import os
    from abi_decl import REPO
    dbg = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'rp_playroom_debug.h')).read(), flags=re.S)
    assert _decl(dbg, 'rp_debug_render_states_chunk') == 'rp_handle h , int32_t slots'


def test_the_header_states_the_semantics_the_costs_and_the_errors():
    import os
    from abi_decl import REPO
    src = open(os.path.join(REPO, 'include', 'rp_playroom.h')).read()
    text = ' '.join(src[src.index('camera images of stored state rows'):src.index('int rp_render_states')].replace('\n * ', ' ').split())      # (the comment's line starts)
    for words in ('byte for byte', 'rp_render_layers', 'OF THE ROW\'S STATE', 'never writes', 'NOT DRAWN', 'keep what they held', 'rp_copy_envs', 'ahead of their first barrier',
                  'DEFAULT row', 'does not make the table', 'RP_GOAL_GHOST', 'RP_GOAL_SOLID', 'ONE and only pass', 'opaque', 'GOAL\'s joint values', 'UR5Reach-v0',
                  '2^31 - 1', 'min(m, max(N, 4096))', 'two launches', 'tile-major', 'No host wait', 'growth of the pose table', 'another stream', 'RP_ERR_ARG',
                  'row_stride < 512', 'multiple of 4', 'n_rows < 1', 'unknown goal_mode', 'k_collider_poses_rows', 'k_render_states'):
        assert words in text, words


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(('rp_render_states',), (b'k_collider_poses_rows', b'k_render_states'))
    assert 'rp_debug_render_states_chunk' in _lib.DEBUG_EXPORTS and 'rp_debug_render_states_chunk' not in _lib.EXPORTS
    import subprocess
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], check=True, capture_output=True, text=True).stdout
        assert re.search(r' T rp_debug_render_states_chunk$', out, flags=re.M), path
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_render_states.argtypes == [vp, ctypes.POINTER(_lib.RpStateRows), i32, ctypes.POINTER(_lib.RpCamera), vp, f32, f32, i32, i32, i32, vp, vp, vp, vp, i32, vp]
        assert lib.rp_debug_render_states_chunk.argtypes == [vp, i32]
        # RP_ERR_ARG for a NULL handle, before anything is touched
        src = _lib.RpStateRows(None, 512, 1, None, None)
        assert lib.rp_render_states(None, ctypes.byref(src), 1, None, None, 0.01, 10.0, 0, 8, 8, None, None, None, None, 0, None) == -1
        assert lib.rp_debug_render_states_chunk(None, 3) == -1
        assert lib.rp_version().decode().startswith('rp_playroom 0.5.2 ')


def test_the_ctypes_struct_and_the_constants_are_the_header_s():
    """field order as in the header; the C layout on an LP64 host: a pointer, a size_t, an int and four bytes of padding, two pointers"""
    from roboticsplayroompybullet_amd import _lib
    assert tuple(n for n, _ in _lib.RpStateRows._fields_) == FIELDS == struct_fields(_header())
    assert dict(_lib.RpStateRows._fields_) == {'rows': ctypes.c_void_p, 'row_stride': ctypes.c_size_t, 'n_rows': ctypes.c_int32, 'row_index': ctypes.c_void_p,
                                               'vis_env': ctypes.c_void_p}
    assert ctypes.sizeof(_lib.RpStateRows) == 40
    assert {n: getattr(_lib.RpStateRows, n).offset for n in FIELDS} == {'rows': 0, 'row_stride': 8, 'n_rows': 16, 'row_index': 24, 'vis_env': 32}
    src = _header()
    values = {k: int(v) for k, v in re.findall(r'(RP_GOAL_[A-Z]+) = (\d+)', re.search(r'enum rp_goal_mode \{(.*?)\}', src).group(1))}
    assert values == {'RP_GOAL_GHOST': _lib.GOAL_GHOST, 'RP_GOAL_SOLID': _lib.GOAL_SOLID} == {'RP_GOAL_GHOST': 0, 'RP_GOAL_SOLID': 1}
    assert _lib.STATE_RECORD_BYTES == 512


def test_vec_env_checks_host_values_before_the_library_is_touched():
    """render_states' host-side checks read nothing of the handle (h is None here: a call that reached the library would fail otherwise): every complaint is a
    ValueError naming the call"""
    import torch
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = object.__new__(VecPlayEnv)
    env.h = None
    env.num_envs, env.device, env.autoreset, env.env_id = 5, 'cpu', False, 'UR5PlayAbsRPY1Obj-v0'
    ok = torch.zeros((6, 160), dtype=torch.float32)
    idx = torch.zeros(3, dtype=torch.int32)
    bad_states = (torch.zeros((6, 160), dtype=torch.float64),          # dtype
                  torch.zeros((6, 160), dtype=torch.float16),
                  torch.zeros(160, dtype=torch.float32),                # shape: one dimension
                  torch.zeros((2, 3, 160), dtype=torch.float32),        # three
                  torch.zeros((6, 127), dtype=torch.float32),           # a row shorter than the state record
                  torch.zeros((0, 160), dtype=torch.float32),           # no row
                  torch.zeros((6, 320), dtype=torch.float32)[:, ::2],   # the last dimension is not contiguous
                  torch.zeros((160, 6), dtype=torch.float32).t(),
                  torch.zeros((1, 160), dtype=torch.float32).expand(6, 160),      # rows that overlap (stride 0)
                  [[0.0] * 160],                                        # not a tensor
                  ok)                                                   # right in every respect but on the host
    for s in bad_states:
        with pytest.raises(ValueError, match='render_states: .*states'):
            env.render_states(s, 8, 8)
    for kw in (dict(index=torch.zeros(3, dtype=torch.int64)), dict(index=torch.zeros(3, dtype=torch.float32)), dict(index=torch.zeros((3, 1), dtype=torch.int32)),
               dict(index=[0, 1, 2]), dict(index=idx)):
        with pytest.raises(ValueError, match='render_states: index'):
            env.render_states(None, 8, 8, **kw)
    for kw in (dict(visuals=torch.zeros(5, dtype=torch.int64)), dict(visuals=torch.zeros(5, dtype=torch.uint8)), dict(visuals=(0, 1, 2, 3, 4)),
               dict(visuals=torch.zeros(5, dtype=torch.int32))):
        with pytest.raises(ValueError, match='render_states: visuals'):
            env.render_states(None, 8, 8, **kw)
    for kw in (dict(goal_mode='opaque'), dict(goal_mode=1), dict(goal_mode=None)):
        with pytest.raises(ValueError, match="render_states: goal_mode is 'ghost' or 'solid'"):
            env.render_states(None, 8, 8, **kw)
    with pytest.raises(ValueError, match='render_states: camera or cameras, not both'):
        env.render_states(None, 8, 8, camera=object(), cameras=torch.zeros((5, 11)))
    for kw in (dict(layers=()), dict(layers=('rgb', 'normals')), dict(depth='metric'), dict(near=0.0), dict(far=0.001), dict(cameras=torch.zeros((5, 11)))):
        with pytest.raises(ValueError, match='render_states'):
            env.render_states(None, 8, 8, **kw)
    p = inspect.signature(VecPlayEnv.render_states).parameters
    assert list(p) == ['self', 'states', 'width', 'height', 'index', 'visuals', 'camera', 'cameras', 'layers', 'depth', 'near', 'far', 'goal', 'goal_mode', 'out']
    assert {k: v.default for k, v in p.items() if k not in ('self', 'states', 'width', 'height')} == {
        'index': None, 'visuals': None, 'camera': None, 'cameras': None, 'layers': ('rgb', 'depth', 'segmentation'), 'depth': 'buffer', 'near': 0.01, 'far': 10.0,
        'goal': None, 'goal_mode': 'ghost', 'out': None}
    p = inspect.signature(VecPlayEnv.goal_images).parameters
    assert list(p)[:4] == ['self', 'goal', 'width', 'height'] and 'goal_mode' not in p and 'visuals' not in p
    for words in ('get_state()', '[:, :128]', 'replay buffer', 'unwritten', 'solid', 'ghost', 'ValueError'):
        assert words in VecPlayEnv.render_states.__doc__, words
    assert "goal_mode='solid'" in VecPlayEnv.goal_images.__doc__ and 'desired_goal' in VecPlayEnv.goal_images.__doc__
