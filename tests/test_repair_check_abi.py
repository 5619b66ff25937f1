"""CPU: the ABI surface of sec_repair_check_batch (struct layout, declared and exported symbol,
NULL context) and Engine.repair_check_host's precondition check, which raises before any device
work."""

import ctypes
import os
import re

import numpy as np
import pytest

from storb_amd import _lib
from storb_amd.engine import Error, check_repair_check_item

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "storb_ec.h")


def test_struct_layout():
    assert ctypes.sizeof(_lib.sec_rchk_chunk) == 40
    assert _lib.RCHK_DTYPE.itemsize == 40
    assert _lib.RCHK_DTYPE.names == tuple(f for f, _ in _lib.sec_rchk_chunk._fields_)
    assert _lib.RCHK_DTYPE.names == ("B", "slot0", "tgt0", "ntargets", "n", "k", "m")
    for name, _ in _lib.sec_rchk_chunk._fields_:
        assert _lib.RCHK_DTYPE.fields[name][1] == getattr(_lib.sec_rchk_chunk, name).offset, name


def test_symbol_is_declared_bound_and_exported():
    with open(HEADER) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+sec_repair_check_batch\s*\(", txt)
    assert re.search(r"\}\s*sec_rchk_chunk\s*;", txt)
    assert re.search(r"#define\s+SEC_ABI_VERSION\s+1\b", txt)
    assert "sec_repair_check_batch" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "sec_repair_check_batch")
    assert lib.sec_abi_version() == 1  # an addition: the ABI version stays


def test_null_context_is_einval():
    lib = _lib.load()
    d = np.zeros(1, dtype=_lib.RCHK_DTYPE)
    d[0] = (64, 0, 0, 1, 5, 4, 6)
    sn = np.array([0, 2, 3, 4, 5], dtype=np.int32)
    bo = np.zeros(5, np.uint64)
    tn = np.array([1], dtype=np.int32)
    to = np.zeros(1, np.uint64)
    res = np.zeros(1, dtype=_lib.CHK_RESULT_DTYPE)
    out = np.zeros(64, np.uint8)
    assert lib.sec_repair_check_batch(None, d.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                      tn.ctypes.data, to.ctypes.data, out.ctypes.data, None, res.ctypes.data, None,
                                      None, 0) == _lib.SEC_EINVAL
    assert lib.sec_repair_check_batch(None, None, 0, None, None, None, None, None, None, None, None, None, None, None,
                                      _lib.SEC_F_HOST) == _lib.SEC_EINVAL


def test_timing_kind_has_a_name():
    from storb_amd import engine
    assert engine._TIMING_KINDS["repair_check"] == 7
    lib = _lib.load()
    ms, n = ctypes.c_double(), ctypes.c_int64()
    assert lib.sec_timing_collect(None, 7, ctypes.byref(ms), ctypes.byref(n)) == _lib.SEC_EINVAL


B2 = [b"ab"] * 5
OK = [0, 2, 3, 4, 5]


@pytest.mark.parametrize("item,code", [
    ((4, 6, B2, [0, 2, 3, 4], [1]), _lib.SEC_ENBLOCKS),                 # blocks and sharenums differ in number
    ((4, 6, [b"ab"] * 4 + [b"abc"], OK, [1]), _lib.SEC_EBLOCKLEN),
    ((0, 6, B2, OK, [1]), _lib.SEC_EKM),
    ((7, 6, B2, OK, [1]), _lib.SEC_EKM),
    ((4, 257, B2, OK, [1]), _lib.SEC_EKM),
    ((7, 6, B2[:3], OK[:3], [9]), _lib.SEC_EKM),                        # before SEC_ENBLOCKS and SEC_ESHARENUM
    ((4, 6, B2[:3], OK[:3], [1]), _lib.SEC_ENBLOCKS),                   # n < k
    ((4, 4, B2, OK, []), _lib.SEC_ENBLOCKS),                            # n > m, before SEC_ESHARENUM
    ((4, 6, B2, [0, 2, 3, 4, 6], [1]), _lib.SEC_ESHARENUM),
    ((4, 6, B2, [0, 2, 3, 4, -1], [1]), _lib.SEC_ESHARENUM),
    ((4, 6, B2, OK, [6]), _lib.SEC_ESHARENUM),                          # a target outside [0, m)
    ((4, 6, B2, OK, [-1]), _lib.SEC_ESHARENUM),
    ((4, 6, B2, [0, 2, 2, 4, 5], [7]), _lib.SEC_ESHARENUM),             # before SEC_EDUPSHARE
    ((4, 6, B2, [0, 2, 2, 4, 5], [1]), _lib.SEC_EDUPSHARE),             # a repeat within the basis
    ((4, 6, B2, [0, 2, 3, 4, 4], [1]), _lib.SEC_EDUPSHARE),             # a check row that is a basis block
    ((4, 8, B2, OK, [1, 6, 1]), _lib.SEC_EDUPSHARE),                    # a repeated target
    ((4, 6, B2, OK, [5]), _lib.SEC_EDUPSHARE),                          # a target that is held as a check row
    ((4, 6, B2, OK, [2]), _lib.SEC_EDUPSHARE),                          # a target that is held in the basis
])
def test_item_preconditions_raise_without_a_device(item, code):
    with pytest.raises(Error) as e:
        check_repair_check_item(*item)
    assert str(e.value) == _lib.strerror(code)


def test_valid_items_pass():
    check_repair_check_item(4, 6, B2, [5, 0, 3, 2, 4], [1])
    check_repair_check_item(4, 6, B2[:4], [5, 0, 3, 2], [1, 4])  # n == k: a plain repair
    check_repair_check_item(4, 6, B2, [5, 0, 3, 2, 4], [])        # no target: a plain check
    check_repair_check_item(4, 6, B2[:4], [5, 0, 3, 2], [])       # neither: nothing to do
