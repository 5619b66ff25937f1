"""CPU: the ABI surface of sec_decode_correct_batch (result struct layout, exported symbol, NULL
context, timing kind) and Engine.decode_correct_host's precondition check, which raises before any
device work."""

import ctypes

import numpy as np
import pytest

from storb_amd import _lib
from storb_amd.engine import Error, check_decode_correct_item


def test_result_struct_layout():
    assert ctypes.sizeof(_lib.sec_cor_result) == 24
    assert _lib.COR_RESULT_DTYPE.itemsize == 24
    assert _lib.COR_RESULT_DTYPE.names == tuple(f for f, _ in _lib.sec_cor_result._fields_)
    assert _lib.COR_RESULT_DTYPE.names == ("first", "first_open", "corrected", "open")
    assert [_lib.COR_RESULT_DTYPE.fields[f][1] for f in _lib.COR_RESULT_DTYPE.names] == [0, 8, 16, 20]
    for name, _ in _lib.sec_cor_result._fields_:
        assert _lib.COR_RESULT_DTYPE.fields[name][1] == getattr(_lib.sec_cor_result, name).offset, name


def test_symbol_is_declared_and_exported():
    assert "sec_decode_correct_batch" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "sec_decode_correct_batch")
    assert lib.sec_abi_version() == 1  # an addition: the ABI version stays


def test_null_context_is_einval():
    lib = _lib.load()
    d = np.zeros(1, dtype=_lib.DCHK_DTYPE)
    d[0] = (0, 64, 0, 0, 6, 4, 6, 0)
    sn = np.arange(6, dtype=np.int32)
    bo = np.zeros(6, np.uint64)
    res = np.zeros(1, dtype=_lib.COR_RESULT_DTYPE)
    hits = np.zeros(6, np.uint32)
    out = np.zeros(256, np.uint8)
    assert lib.sec_decode_correct_batch(None, d.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                        out.ctypes.data, res.ctypes.data, hits.ctypes.data, 0) == _lib.SEC_EINVAL
    assert lib.sec_decode_correct_batch(None, None, 0, None, None, None, None, None, None, None,
                                        _lib.SEC_F_HOST) == _lib.SEC_EINVAL


def test_timing_kind_has_a_name():
    from storb_amd import engine
    assert engine._TIMING_KINDS["decode_correct"] == 8
    assert sorted(engine._TIMING_KINDS.values()) == list(range(9))
    lib = _lib.load()
    ms, n = ctypes.c_double(), ctypes.c_int64()
    assert lib.sec_timing_collect(None, 8, ctypes.byref(ms), ctypes.byref(n)) == _lib.SEC_EINVAL


B2 = [b"ab"] * 6


@pytest.mark.parametrize("item,code", [
    ((4, 6, B2, [0, 1, 2, 3, 4], 0), _lib.SEC_ENBLOCKS),            # blocks and sharenums differ in number
    ((4, 6, [b"ab"] * 5 + [b"abc"], [0, 1, 2, 3, 4, 5], 0), _lib.SEC_EBLOCKLEN),
    ((0, 6, B2, [0, 1, 2, 3, 4, 5], 0), _lib.SEC_EKM),
    ((7, 6, B2, [0, 1, 2, 3, 4, 5], 0), _lib.SEC_EKM),
    ((4, 257, B2, [0, 1, 2, 3, 4, 5], 0), _lib.SEC_EKM),
    ((4, 6, B2[:3], [0, 1, 2], 0), _lib.SEC_ENBLOCKS),              # n < k
    ((4, 5, B2, [0, 1, 2, 3, 4, 5], 0), _lib.SEC_ENBLOCKS),         # n > m
    ((4, 6, B2, [0, 1, 2, 3, 4, 6], 0), _lib.SEC_ESHARENUM),
    ((4, 6, B2, [0, 1, 2, 3, 4, -1], 0), _lib.SEC_ESHARENUM),
    ((4, 6, B2, [0, 1, 2, 3, 4, 4], 0), _lib.SEC_EDUPSHARE),
    ((4, 6, B2, [0, 1, 2, 2, 4, 5], 0), _lib.SEC_EDUPSHARE),
    ((4, 6, B2, [0, 1, 2, 3, 4, 5], -1), _lib.SEC_EPADLEN),
    ((4, 6, B2, [0, 1, 2, 3, 4, 5], 9), _lib.SEC_EPADLEN),          # padlen > k*B
])
def test_item_preconditions_raise_without_a_device(item, code):
    with pytest.raises(Error) as e:
        check_decode_correct_item(*item)
    assert str(e.value) == _lib.strerror(code)


def test_valid_items_pass():
    check_decode_correct_item(4, 6, B2, [5, 0, 3, 2, 4, 1], 8)
    check_decode_correct_item(4, 6, B2[:4], [5, 0, 3, 2], 0)  # n == k: a plain decode
