"""The names functions of the per-env tables on a GPU-less host: the bake is read once and the names are cached per model, so repeated calls must return equal
values, and what a caller does to a returned dict or list must not show in the next call."""
import pytest

KINDS = ('U', 'R', 'P', 'Q', 'V', 'W')
NAMES = ('dynamics_names', 'wrench_names', 'kinematics_names', 'actuation_names')


@pytest.mark.parametrize('fn', NAMES)
def test_names_are_equal_on_repeated_calls(fn):
    from roboticsplayroompybullet_amd import vec_env
    for kind in KINDS:
        a, b = getattr(vec_env, fn)(kind), getattr(vec_env, fn)(kind)
        assert a == b and type(a) is type(b), (fn, kind)
        assert len(a) > 0


@pytest.mark.parametrize('fn', NAMES)
def test_a_callers_mutation_does_not_reach_the_next_call(fn):
    from roboticsplayroompybullet_amd import vec_env
    for kind in KINDS:
        first = getattr(vec_env, fn)(kind)
        if isinstance(first, dict):
            keep = {k: tuple(v) for k, v in first.items()}
            for k in list(first):
                first[k] = list(first[k]) + ['mutated']      # the values are tuples: a caller can only replace them ...
            first['extra'] = ()                              # ... or add and drop keys
            del first[next(iter(keep))]
            again = getattr(vec_env, fn)(kind)
            assert {k: tuple(v) for k, v in again.items()} == keep, (fn, kind)
        else:
            keep = tuple(first)
            if isinstance(first, list):                      # (a tuple cannot be changed at all)
                first.append('mutated')
            assert tuple(getattr(vec_env, fn)(kind)) == keep, (fn, kind)


def test_the_env_properties_hand_out_the_module_functions_values():
    """VecPlayEnv's *_names properties are the module functions of the id's model (no GPU: read off the class without a handle)"""
    from roboticsplayroompybullet_amd import VecPlayEnv, vec_env

    class Stub:
        env_id = 'UR5PlayAbsRPY1Obj-v0'
    for fn in NAMES:
        got = getattr(VecPlayEnv, fn).fget(Stub())
        assert got == getattr(vec_env, fn)('U'), fn
        if isinstance(got, dict):
            got.clear()
            assert getattr(VecPlayEnv, fn).fget(Stub()) == getattr(vec_env, fn)('U') != {}, fn
