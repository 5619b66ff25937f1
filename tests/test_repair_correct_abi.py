"""CPU: the ABI surface of sec_repair_correct_batch (exported symbol, NULL context, no new timing
kind) and Engine.repair_correct_host's precondition check, which raises before any device work and
differs from repair + check's in one point: a target may be a block that is held."""

import ctypes

import numpy as np
import pytest

from storb_amd import _lib
from storb_amd.engine import Error, check_repair_check_item, check_repair_correct_item


def test_symbol_is_declared_and_exported():
    assert "sec_repair_correct_batch" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "sec_repair_correct_batch")
    assert lib.sec_abi_version() == 1  # an addition: the ABI version stays


def test_null_context_is_einval():
    lib = _lib.load()
    d = np.zeros(1, dtype=_lib.RCHK_DTYPE)
    d[0] = (64, 0, 0, 2, 6, 4, 6)
    sn = np.arange(6, dtype=np.int32)
    bo = np.zeros(6, np.uint64)
    tn = np.array([1, 4], np.int32)
    to = np.zeros(2, np.uint64)
    res = np.zeros(1, dtype=_lib.COR_RESULT_DTYPE)
    hits = np.zeros(6, np.uint32)
    out = np.zeros(256, np.uint8)
    assert lib.sec_repair_correct_batch(None, d.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                        tn.ctypes.data, to.ctypes.data, out.ctypes.data, None, res.ctypes.data,
                                        hits.ctypes.data, 0) == _lib.SEC_EINVAL
    assert lib.sec_repair_correct_batch(None, None, 0, None, None, None, None, None, None, None, None, None, None,
                                        _lib.SEC_F_HOST) == _lib.SEC_EINVAL


def test_it_shares_the_correcting_timing_kind():
    from storb_amd import engine
    assert "repair_correct" not in engine._TIMING_KINDS
    assert engine._TIMING_KINDS["decode_correct"] == 8
    lib = _lib.load()
    ms, n = ctypes.c_double(), ctypes.c_int64()
    assert lib.sec_timing_collect(None, 9, ctypes.byref(ms), ctypes.byref(n)) == _lib.SEC_EINVAL


B2 = [b"ab"] * 6
ALL = [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("item,code", [
    ((4, 6, B2, [0, 1, 2, 3, 4], []), _lib.SEC_ENBLOCKS),            # blocks and sharenums differ in number
    ((4, 6, [b"ab"] * 5 + [b"abc"], ALL, []), _lib.SEC_EBLOCKLEN),
    ((0, 6, B2, ALL, []), _lib.SEC_EKM),
    ((7, 6, B2, ALL, []), _lib.SEC_EKM),
    ((4, 257, B2, ALL, []), _lib.SEC_EKM),
    ((4, 6, B2[:3], [0, 1, 2], [3]), _lib.SEC_ENBLOCKS),             # n < k
    ((4, 5, B2, ALL, []), _lib.SEC_ENBLOCKS),                        # n > m
    ((4, 7, B2, [0, 1, 2, 3, 4, 7], [6]), _lib.SEC_ESHARENUM),
    ((4, 7, B2, ALL, [7]), _lib.SEC_ESHARENUM),                      # a target >= m
    ((4, 7, B2, ALL, [-1]), _lib.SEC_ESHARENUM),
    ((4, 7, B2, [0, 1, 2, 3, 4, 4], [6]), _lib.SEC_EDUPSHARE),       # a repeat among the entries
    ((4, 7, B2, ALL, [6, 6]), _lib.SEC_EDUPSHARE),                   # a repeated lost target
    ((4, 7, B2, ALL, [1, 6, 1]), _lib.SEC_EDUPSHARE),                # a repeated heal target
    ((4, 7, B2, [0, 1, 2, 3, 4, 9], [6, 6]), _lib.SEC_ESHARENUM),    # range errors before any repeat
])
def test_item_preconditions_raise_without_a_device(item, code):
    with pytest.raises(Error) as e:
        check_repair_correct_item(*item)
    assert str(e.value) == _lib.strerror(code)


def test_a_held_target_is_accepted_here_and_only_here():
    item = (4, 7, B2, [5, 0, 3, 2, 4, 1], [6, 1, 5, 0])
    check_repair_correct_item(*item)
    with pytest.raises(Error) as e:
        check_repair_check_item(*item)
    assert str(e.value) == _lib.strerror(_lib.SEC_EDUPSHARE)
    check_repair_check_item(4, 7, B2, [5, 0, 3, 2, 4, 1], [6])


def test_valid_items_pass():
    check_repair_correct_item(4, 7, B2, [5, 0, 3, 2, 4, 1], [])          # no target: judge and count
    check_repair_correct_item(4, 6, B2[:4], [5, 0, 3, 2], [5, 1])        # n == k: a heal target is a copy
    check_repair_correct_item(4, 6, B2, ALL, ALL)                        # every held piece healed
