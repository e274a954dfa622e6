"""rp_step_autoreset's C ABI (0.5) on a GPU-less host: declared in include/rp_playroom.h, exported by both libraries, mirrored in _lib and in VecPlayEnv."""
import ctypes
import inspect
import re

from abi_decl import assert_exported_by_both_libraries, header as _header

NEW = ('rp_set_autoreset', 'rp_get_episode_steps', 'rp_set_episode_steps', 'rp_step_autoreset')


def test_new_entry_points_are_declared():
    src = _header()
    for name in NEW:
        assert re.search(r'\bint %s\s*\(' % name, src), name
    decl = ' '.join(re.search(r'int rp_step_autoreset\((.*?)\);', src, flags=re.S).group(1).replace(',', ' , ').split())
    assert decl == ('rp_handle h , const float* action , const uint8_t* end_mask , const rp_out* out , const rp_out* final_out , int32_t* done , '
                    'void* stream'), decl


def test_new_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(NEW)
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH):
        lib = ctypes.CDLL(path)
        lib.rp_version.restype = ctypes.c_char_p
        assert b'rp_playroom 0.5' in lib.rp_version()
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert len(lib.rp_step_autoreset.argtypes) == 7
        assert lib.rp_set_autoreset.argtypes[1:] == [ctypes.c_int32, ctypes.c_uint32]


def test_autoreset_enum_matches_the_header():
    from roboticsplayroompybullet_amd import _lib
    enums = {k: int(v) for k, v in re.findall(r'\b(RP_AR_[A-Z_]+)\s*=\s*(\d+)', _header())}
    assert enums == {'RP_AR_TIME_LIMIT': 1, 'RP_AR_FAULT': 2, 'RP_AR_SUCCESS': 4}
    assert (_lib.AR_TIME_LIMIT, _lib.AR_FAULT, _lib.AR_SUCCESS) == (1, 2, 4)
    assert (_lib.DONE_TIME_LIMIT, _lib.DONE_END_MASK, _lib.DONE_FAULT, _lib.DONE_SUCCESS) == (1, 2, 4, 8)


def test_vec_env_takes_the_autoreset_kwargs():
    from roboticsplayroompybullet_amd import VecPlayEnv
    params = inspect.signature(VecPlayEnv.__init__).parameters
    assert params['autoreset'].default is False
    assert params['max_episode_steps'].default is None
    assert params['end_on_fault'].default is True
    assert params['end_on_success'].default is False
    assert 'end_mask' in inspect.signature(VecPlayEnv.step).parameters
    assert isinstance(inspect.getattr_static(VecPlayEnv, 'episode_steps'), property)
    assert VecPlayEnv.episode_steps.fset is not None


def test_autoreset_kernels_are_in_the_library():
    """the device path is HIP: k_autoreset_mark and k_autoreset are compiled into both code objects"""
    from roboticsplayroompybullet_amd import _lib
    _lib.build()
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH):
        blob = open(path, 'rb').read()
        assert b'k_autoreset_mark' in blob and b'k_autoreset' in blob, path
