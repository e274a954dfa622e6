"""Per-env gravity and arm-motor gain / strength (rp_get_actuation_dims / rp_set_actuation / rp_get_actuation) on a GPU-less host: declared in
include/rp_playroom.h, exported by both libraries together with their kernels, mirrored in _lib and VecPlayEnv; the column names against the bake and
against wrench_names; the host-side value checks."""
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest

from abi_decl import REPO, TABLE_KERNELS, assert_exported_by_both_libraries, decl as _decl, header as _header

NEW = ('rp_get_actuation_dims', 'rp_set_actuation', 'rp_get_actuation')
KINDS = ('U', 'R', 'P', 'Q', 'V', 'W')


def test_entry_points_are_declared():
    src = _header()
    assert _decl(src, 'rp_get_actuation_dims') == 'rp_handle h , int32_t* n_arm'
    assert _decl(src, 'rp_set_actuation') == ('rp_handle h , const float* gravity , const float* motor_gain , const float* motor_strength , int32_t rows , '
                                              'const uint8_t* mask , void* stream')
    assert _decl(src, 'rp_get_actuation') == 'rp_handle h , float* gravity , float* motor_gain , float* motor_strength , void* stream'


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(NEW, TABLE_KERNELS)
    vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)
    n_args = {name: len(_decl(_header(), name).split(' , ')) for name in NEW}
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_get_actuation_dims.argtypes == [vp, ip]
        assert lib.rp_set_actuation.argtypes == [vp, vp, vp, vp, ctypes.c_int32, vp, vp]
        assert lib.rp_get_actuation.argtypes == [vp, vp, vp, vp, vp]
        for name in NEW:          # the binding's arity is the declaration's
            assert len(getattr(lib, name).argtypes) == n_args[name], name


def test_version_keeps_its_prefix():
    from roboticsplayroompybullet_amd import _lib
    _lib.build()
    for wide in (False, True):
        v = _lib.load(wide=wide).rp_version().decode()
        assert v.startswith('rp_playroom 0.5'), v
        assert v.startswith('rp_playroom 0.5.2 '), v


def test_vec_env_has_the_actuation_methods():
    from roboticsplayroompybullet_amd import VecPlayEnv
    assert isinstance(inspect.getattr_static(VecPlayEnv, 'actuation_names'), property)
    assert list(inspect.signature(VecPlayEnv.get_actuation).parameters) == ['self']
    p = inspect.signature(VecPlayEnv.set_actuation).parameters
    assert list(p) == ['self', 'gravity', 'motor_gain', 'motor_strength', 'mask']
    assert all(p[k].default is None for k in ('gravity', 'motor_gain', 'motor_strength', 'mask'))


@pytest.mark.parametrize('kind', KINDS)
def test_actuation_names_follow_the_bake(kind):
    """gravity's columns are x, y, z; the motor columns are the arm's dofs in dof order, named as wrench_names names their links"""
    from roboticsplayroompybullet_amd.vec_env import actuation_names, wrench_names
    mdl = next(m for m in json.load(open(os.path.join(REPO, 'roboticsplayroompybullet_amd', 'assets', 'models.json')))['models'] if m['kind'] == kind)
    names = actuation_names(kind)
    assert set(names) == {'gravity', 'motor'}
    assert list(names['gravity']) == ['x', 'y', 'z']
    assert len(names['motor']) == mdl['n_arm'] and len(set(names['motor'])) == mdl['n_arm']
    assert tuple(names['motor']) == wrench_names(kind)[:mdl['n_arm']]


def test_host_values_are_checked():
    import torch
    from roboticsplayroompybullet_amd.vec_env import check_actuation_values
    assert check_actuation_values('gravity', [0.0, -50.0, 50.0]).tolist() == [0.0, -50.0, 50.0]
    assert check_actuation_values('gravity', np.zeros((4, 3))).dtype == torch.float32
    assert check_actuation_values('motor_gain', [0.0, 1.0, 10.0]).tolist() == [0.0, 1.0, 10.0]
    assert check_actuation_values('motor_strength', [0.0, 0.5, 10.0]).tolist() == [0.0, 0.5, 10.0]
    bad = {'gravity': ([0.0, 0.0, -50.5], [51.0, 0.0, 0.0], [math.nan, 0.0, 0.0], [0.0, math.inf, 0.0]),
           'motor_gain': ([-0.1], [10.5], [math.nan], torch.tensor([1.0, math.inf])),
           'motor_strength': ([-1e-3], [11.0], [math.nan], np.array([[-math.inf]]))}
    for what, values in bad.items():
        for v in values:
            with pytest.raises(ValueError):
                check_actuation_values(what, v)
