"""rp_set_reset_table / rp_get_reset_rows on a GPU-less host: declared in include/rp_playroom.h, exported by both libraries, mirrored in _lib and in
VecPlayEnv, their kernels compiled into both code objects; and the row rule (tests/reset_rows.py) on hand-worked cases."""
import ctypes
import inspect

from abi_decl import assert_exported_by_both_libraries, decl as _decl, header as _header
from reset_rows import reset_rows

NEW = ('rp_set_reset_table', 'rp_get_reset_rows')


def test_entry_points_are_declared():
    src = _header()
    assert _decl(src, 'rp_set_reset_table') == 'rp_handle h , const float* o , int32_t rows , int32_t n_o , void* stream'
    assert _decl(src, 'rp_get_reset_rows') == 'rp_handle h , int32_t* dst , void* stream'


def test_entry_points_are_exported_by_both_libraries_and_mirrored():
    from roboticsplayroompybullet_amd import _lib
    assert_exported_by_both_libraries(NEW)
    vp = ctypes.c_void_p
    for wide in (False, True):
        lib = _lib.load(wide=wide)
        assert lib.rp_set_reset_table.argtypes == [vp, vp, ctypes.c_int32, ctypes.c_int32, vp]
        assert lib.rp_get_reset_rows.argtypes == [vp, vp, vp]


def test_vec_env_takes_a_reset_table():
    from roboticsplayroompybullet_amd import VecPlayEnv
    assert inspect.signature(VecPlayEnv.__init__).parameters['reset_table'].default is None
    assert list(inspect.signature(VecPlayEnv.set_reset_table).parameters) == ['self', 'o']
    assert list(inspect.signature(VecPlayEnv.random_start_table).parameters) == ['self', 'm', 'seed']


def test_reset_table_kernels_are_in_the_library():
    """the row pass and the reset from a table are HIP kernels in both code objects"""
    from roboticsplayroompybullet_amd import _lib
    _lib.build()
    for path in (_lib.LIB_PATH, _lib.WIDE_LIB_PATH):
        blob = open(path, 'rb').read()
        assert b'k_autoreset_rows' in blob and b'k_autoreset_to' in blob, path


def test_row_rule_by_hand():
    # one end: the cursor's row, the cursor moves by one
    rows, cur = reset_rows([0, 0, 1, 0], 2, 5)
    assert list(rows) == [-1, -1, 2, -1] and cur == 3
    # several ends in one call: ranked by env index
    rows, cur = reset_rows([1, 0, 1, 1, 0, 1], 1, 10)
    assert list(rows) == [1, -1, 2, 3, -1, 4] and cur == 5
    # more ends than rows: the rows wrap inside the call
    rows, cur = reset_rows([1, 1, 1, 1, 1, 0, 1], 1, 3)
    assert list(rows) == [1, 2, 0, 1, 2, -1, 0] and cur == 1
    # rows > N: no wrap, the cursor keeps going past N
    rows, cur = reset_rows([1, 0, 1], 6, 100)
    assert list(rows) == [6, -1, 7] and cur == 8
    # ... and wraps at rows
    rows, cur = reset_rows([1, 1, 0], 99, 100)
    assert list(rows) == [99, 0, -1] and cur == 1
    # no ends: nothing moves
    rows, cur = reset_rows([0, 0, 0], 4, 7)
    assert list(rows) == [-1, -1, -1] and cur == 4


def test_row_rule_across_waves_is_the_env_order():
    """ends in several 64-env waves (0, 63, 64, 1000, N - 1): ranks follow env indices, not waves"""
    n = 1101
    done = [0] * n
    for e in (0, 63, 64, 1000, n - 1):
        done[e] = 1
    rows, cur = reset_rows(done, 5, 7)
    assert [int(rows[e]) for e in (0, 63, 64, 1000, n - 1)] == [5, 6, 0, 1, 2] and cur == 3
    assert sum(r >= 0 for r in rows) == 5
