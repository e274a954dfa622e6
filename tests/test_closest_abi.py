"""Closest points between colliders (rp_closest_points) on a GPU-less host: the enum and the entry points declared in include/rp_playroom.h with the rule, the
statuses, the costs and the errors stated, exported by both libraries together with k_closest_points, mirrored in _lib (EXPORTS, argtypes, the status constants), the
argument checks that need no device, and VecPlayEnv's host-side checks and name expansion on an object without a handle."""
import ctypes
import inspect
import os
import re

import pytest

from abi_decl import REPO, assert_exported_by_both_libraries, decl as _decl, header as _header


def test_the_header_declares_the_enum_and_the_entry_points():
    src = _header()
    assert re.search(r'enum rp_cp_status \{ RP_CP_SEPARATED = 0, RP_CP_OVERLAP = 1, RP_CP_FAR = 2, RP_CP_SKIPPED = 3, RP_CP_CAPPED = 4\s*\};', src)
    assert _decl(src, 'rp_get_collider_dims') == 'rp_handle h , int32_t* n_col'
    assert _decl(src, 'rp_closest_points') == ('rp_handle h , const rp_state_rows* src , int32_t m , const int32_t* pairs , int32_t k , int32_t n_groups , '
                                               'float max_distance , float* distance , float* point_a , float* point_b , float* normal , int32_t* status , '
                                               'float* group_min , int32_t* group_pair , void* stream')


def test_the_header_states_the_rule_the_statuses_the_costs_and_the_errors():
    src = open(os.path.join(REPO, 'include', 'rp_playroom.h')).read()
    text = src[src.index('closest points between colliders, live or from stored state rows'):src.index('enum rp_cp_status')]
    text = ' '.join(re.sub(r'\n \* ?', '\n', text).split())      # (the comment's line starts are no words of it)
    for words in ('getClosestPoints', 'WITHOUT MARGINS', 'exact box', 'convex hull of its baked vertices', 'link against link', 'DEVICE int32 [k, 3]', 'never on the host',
                  "GJK's distance phase", 'lowest vertex number among equals', 'in double', 'bounded', 'upper bound', 'RP_CP_CAPPED', 'FROM B TOWARD A',
                  'point_a - point_b = normal * distance', 'RP_CP_OVERLAP', 'exactly 0', 'common point', 'PENETRATION DEPTH IS NOT REPORTED', 'RP_CP_FAR', 'world AABBs',
                  'lower bound', 'max_distance <= 0', 'RP_CP_SKIPPED', 'a == b', 'KEEP WHAT THEY HELD', 'rp_copy_envs', 'group_min', 'group_pair',
                  'lowest index among equals', '+inf and -1', 'no atomics', 'same bits on every run', 'two launches', 'k_collider_poses_rows', 'k_closest_points',
                  'no host wait', 'no host read', 'only allocation', 'never writes state rows', 'ONE collider-pose table', 'another stream', 'vis_env is ignored',
                  'RP_ERR_ARG', 'm < 1', '1 .. 4096', '0 .. 64', 'n_groups == 0', 'pairs NULL', 'every output NULL', 'not a number', 'row_stride < 512'):
        assert words in text, words


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(('rp_closest_points', 'rp_get_collider_dims'), (b'k_closest_points',))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_closest_points.argtypes == [vp, ctypes.POINTER(_lib.RpStateRows), i32, vp, i32, i32, ctypes.c_float] + [vp] * 8
        assert lib.rp_get_collider_dims.argtypes == [vp, ctypes.POINTER(i32)]
        # RP_ERR_ARG for a NULL handle, before anything is touched
        assert lib.rp_closest_points(None, None, 1, None, 1, 0, 0.0, None, None, None, None, None, None, None, None) == -1
        n = i32(0)
        assert lib.rp_get_collider_dims(None, ctypes.byref(n)) == -1
        assert lib.rp_version().decode().startswith('rp_playroom 0.5.2 ')


def test_the_constants_are_the_header_s():
    from roboticsplayroompybullet_amd import _lib
    values = {k: int(v) for k, v in re.findall(r'(RP_CP_[A-Z]+) = (\d+)', re.search(r'enum rp_cp_status \{(.*?)\}', _header()).group(1))}
    assert values == {'RP_CP_SEPARATED': _lib.CP_SEPARATED, 'RP_CP_OVERLAP': _lib.CP_OVERLAP, 'RP_CP_FAR': _lib.CP_FAR, 'RP_CP_SKIPPED': _lib.CP_SKIPPED,
                      'RP_CP_CAPPED': _lib.CP_CAPPED} == {'RP_CP_SEPARATED': 0, 'RP_CP_OVERLAP': 1, 'RP_CP_FAR': 2, 'RP_CP_SKIPPED': 3, 'RP_CP_CAPPED': 4}
    assert (_lib.CP_MAX_PAIRS, _lib.CP_MAX_GROUPS) == (4096, 64)
    src = open(os.path.join(REPO, 'roboticsplayroompybullet_amd', 'csrc', 'rp_closest.cuh')).read()
    assert re.search(r'#define RP_CP_MAX_PAIRS 4096\b', src) and re.search(r'#define RP_CP_MAX_GROUPS 64\b', src)


def _env(env_id='pandaPlayAbsRPY1Obj-v0'):
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = object.__new__(VecPlayEnv)
    env.h = None
    env.num_envs, env.device, env.autoreset, env.env_id = 5, 'cpu', False, env_id
    return env


@pytest.mark.parametrize('env_id', ['UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'pandaPlayAbsRPY1Obj-v0', 'pandaPlay-v0', 'UR5Reach-v0'])
def test_collider_names_are_unique_and_follow_visual_names(env_id):
    env = _env(env_id)
    names, objects = env.collider_names, env.visual_names
    assert len(names) == len(objects) == len(set(names))
    for c, (nm, ob) in enumerate(zip(names, objects)):
        if objects.count(ob) == 1:
            assert nm == ob
        else:
            assert nm == '%s.%d' % (ob, objects[:c].count(ob))
    assert any(n.startswith('link') for n in names)      # arm colliders carry their link's name


def test_collider_pairs_expands_names_objects_and_indices():
    import torch
    env = _env()
    names, objects = env.collider_names, env.visual_names
    drawer = [c for c, o in enumerate(objects) if o == 'drawer']
    assert len(drawer) > 1 and 'drawer' not in names and 'drawer.0' in names
    p = env.collider_pairs('block', 'drawer', group=3)
    assert p.dtype == torch.int32 and tuple(p.shape) == (len(drawer), 3)
    assert p.tolist() == [[names.index('block'), c, 3] for c in drawer]
    # the full product, a-major, without a == b
    p = env.collider_pairs(['link8', 'link9', 'table'], ['table', 'drawer.1', names.index('link9')])
    a, b = [names.index(n) for n in ('link8', 'link9', 'table')], [names.index('table'), names.index('drawer.1'), names.index('link9')]
    assert p.tolist() == [[x, y, 0] for x in a for y in b if x != y] and len(p) == 7
    assert env.collider_pairs(2, 5).tolist() == [[2, 5, 0]]
    for args, kw in ((('no such thing', 'table'), {}), (('table', len(names)), {}), (('table', -1), {}), (('table', 'table'), {}), (('table', 1.5), {}),
                     (('table', 'block'), dict(group=64)), (('table', 'block'), dict(group=-1)), (('table', 'block'), dict(group=1.0))):
        with pytest.raises(ValueError, match='collider_pairs'):
            env.collider_pairs(*args, **kw)


def test_vec_env_checks_host_values_before_the_library_is_touched():
    """every complaint is a ValueError naming closest_points; the object has no handle, so a check that came too late would fail another way"""
    import torch
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = _env()
    n = len(env.collider_names)
    ok = [(0, 1), (2, 3, 0)]
    for pairs, kw in ((ok + [(0, n)], {}), (ok + [(0, 0)], {}), (ok + [(-1, 2)], {}), ([(0, 1, 1)], {}), ([(0, 1, 2)], dict(n_groups=2)), ([(0, 1, -1)], dict(n_groups=2)),
                      ([], {}), ([(0, 1)] * 4097, {}), ([(0, 1, 2, 3)], {}), (5, {}), ('pairs', {}), (torch.zeros((3, 2), dtype=torch.int32), {}),
                      (ok, dict(n_groups=65)), (ok, dict(n_groups=-1)), (ok, dict(n_groups=1.0)), (ok, dict(max_distance=float('nan'))), (ok, dict(max_distance='far')),
                      (ok, dict(states=torch.zeros((4, 127)))), (ok, dict(states=torch.zeros((4, 128), dtype=torch.float64))), (ok, dict(states=torch.zeros(128))),
                      (ok, dict(states=torch.zeros((4, 128)))), (ok, dict(states=torch.zeros((4, 256))[:, ::2])), (ok, dict(index=torch.zeros(3, dtype=torch.int32))),
                      (ok, dict(index=[0, 1])), (ok, dict(out=[1])), (ok, dict(out={'depth': None})),
                      (ok, dict(out={'distance': torch.zeros((5, 2))})), (ok, dict(n_groups=2, out={'group_pair': torch.zeros((5, 2), dtype=torch.int32)}))):
        with pytest.raises(ValueError, match='closest_points'):
            env.closest_points(pairs, **kw)
    p = inspect.signature(VecPlayEnv.closest_points).parameters
    assert list(p) == ['self', 'pairs', 'states', 'index', 'max_distance', 'n_groups', 'out']
    assert {k: v.default for k, v in p.items() if k not in ('self', 'pairs')} == {'states': None, 'index': None, 'max_distance': None, 'n_groups': 0, 'out': None}
    assert list(inspect.signature(VecPlayEnv.collider_pairs).parameters) == ['self', 'a', 'b', 'group']
    for words in ('getClosestPoints', 'from b toward a', 'penetration depth is not reported', 'max_distance', 'skipped', 'upper bound', 'lowest among equals', '+inf / -1',
                  'passed through unread', 'range-checked', 'render_states'):
        assert words in VecPlayEnv.closest_points.__doc__, words
