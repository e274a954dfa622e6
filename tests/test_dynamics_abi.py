"""Per-env dynamics (rp_get_dynamics_dims / rp_set_dynamics / rp_get_dynamics) on a GPU-less host: declared in include/rp_playroom.h, exported by both
libraries, mirrored in _lib and VecPlayEnv; the column names against the oracle's baked colliders; the host-side value checks."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from abi_decl import REPO, TABLE_KERNELS, assert_exported_by_both_libraries, decl as _decl, header as _header

NEW = ('rp_get_dynamics_dims', 'rp_set_dynamics', 'rp_get_dynamics')
KIND_OF = {'U': 'UR5PlayAbsRPY1Obj-v0', 'R': 'UR5Reach-v0', 'P': 'pandaPick-v0', 'Q': 'pandaReach-v0', 'V': 'pandaPlayAbsRPY1Obj-v0', 'W': 'pandaPlay-v0'}


def test_entry_points_are_declared():
    src = _header()
    assert _decl(src, 'rp_get_dynamics_dims') == 'rp_handle h , int32_t* n_obj , int32_t* n_free'
    assert _decl(src, 'rp_set_dynamics') == 'rp_handle h , const float* friction , const float* mass , int32_t rows , const uint8_t* mask , void* stream'
    assert _decl(src, 'rp_get_dynamics') == 'rp_handle h , float* friction , float* mass , void* stream'


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(NEW, TABLE_KERNELS)
    vp = ctypes.c_void_p
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_get_dynamics_dims.argtypes == [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        assert lib.rp_set_dynamics.argtypes == [vp, vp, vp, ctypes.c_int32, vp, vp]
        assert lib.rp_get_dynamics.argtypes == [vp, vp, vp, vp]


def test_vec_env_has_the_dynamics_methods():
    from roboticsplayroompybullet_amd import VecPlayEnv
    assert isinstance(inspect.getattr_static(VecPlayEnv, 'dynamics_names'), property)
    assert list(inspect.signature(VecPlayEnv.get_dynamics).parameters) == ['self']
    p = inspect.signature(VecPlayEnv.set_dynamics).parameters
    assert list(p) == ['self', 'friction', 'mass', 'mask']
    assert all(p[k].default is None for k in ('friction', 'mass', 'mask'))


@pytest.mark.parametrize('kind', tuple(KIND_OF))
def test_dynamics_names_follow_the_bake(kind):
    """per id: one friction column per collision object, named uniquely, each holding the friction the oracle gives every collider of that object;
    one mass column per free body with the oracle's mass; the blocks, the drawer and the table top by name"""
    import json
    from oracle import OracleEnv
    from roboticsplayroompybullet_amd.vec_env import MODEL_OF, dynamics_names
    assert MODEL_OF[KIND_OF[kind]] == kind
    names = dynamics_names(kind)
    mdl = next(m for m in json.load(open(os.path.join(REPO, 'roboticsplayroompybullet_amd', 'assets', 'models.json')))['models'] if m['kind'] == kind)
    cols = OracleEnv(kind).collider_list()
    assert len(cols) == len(mdl['col'])
    n_obj = max(c['obj'] for c in mdl['col']) + 1
    assert len(names['friction']) == n_obj == len({c['obj'] for c in mdl['col']})
    assert len(set(names['friction'])) == n_obj and len(set(names['mass'])) == len(names['mass'])
    for o in range(n_obj):
        fr = {cols[c]['friction'] for c in range(len(cols)) if mdl['col'][c]['obj'] == o}
        assert len(fr) == 1, (kind, o, names['friction'][o], fr)
    n_arm = mdl['n_arm']
    assert len(names['mass']) == len(mdl['free'])
    for f in range(len(mdl['free'])):
        masses = {c['mass'] for c in cols if c['body'] == n_arm + 1 + f}
        assert masses == {mdl['free'][f]['mass']}, (kind, f, masses)
    fr_of = {names['friction'][mdl['col'][c]['obj']]: cols[c]['friction'] for c in range(len(cols))}
    ms_of = dict(zip(names['mass'], (mdl['free'][f]['mass'] for f in range(len(mdl['free'])))))
    if kind in ('U', 'V', 'W'):
        assert fr_of['table'] == 0.5 and fr_of['block'] == 1.5 and ms_of['block'] == pytest.approx(0.3) and 'drawer' in ms_of and 'drawer' in fr_of
    if kind == 'W':
        assert fr_of['block2'] == 1.5 and ms_of['block2'] == pytest.approx(0.3)
    if kind == 'P':
        assert 'block' in ms_of and 'tray' in fr_of
    assert all(re.fullmatch(r'link\d+', n) for n, c in zip(names['friction'], range(n_obj))
               if next(cc for cc in mdl['col'] if cc['obj'] == c)['tag'] == 'arm')


def test_host_values_are_checked():
    from roboticsplayroompybullet_amd.vec_env import check_dynamics_values
    assert check_dynamics_values('friction', [0.0, 1.5]).tolist() == [0.0, 1.5]
    assert check_dynamics_values('mass', np.array([[0.3, 1.2]])).shape == (1, 2)
    for bad in ([-0.1, 1.0], [math.nan, 1.0], [math.inf]):
        with pytest.raises(ValueError):
            check_dynamics_values('friction', bad)
    for bad in ([0.0], [-1.0], [math.nan], np.array([0.3, math.inf])):
        with pytest.raises(ValueError):
            check_dynamics_values('mass', bad)
    import torch
    with pytest.raises(ValueError):
        check_dynamics_values('mass', torch.tensor([0.3, 0.0]))
