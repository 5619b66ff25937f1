"""CPU: the ABI additions of the bit-sliced check: sec_check_method (host logic: which chunks of a
check or a decode + check are eligible for sec_check_bs_kernel), sec_ctx_check_methods and the
context option SEC_CHECK_BS.  No device is needed."""

import ctypes
import random

import numpy as np
import pytest

from storb_amd import _lib, engine

SHAPES = [(10, 14), (8, 12), (16, 24), (32, 48), (64, 96), (8, 11)]


def method(k, m, sharenums, B, avail=None, padlen=0, n=None):
    lib = _lib.load()
    sn = np.asarray(sharenums, np.int32)
    av = None if avail is None else np.asarray(avail, np.uint64)
    out = ctypes.c_int(-7)
    rc = lib.sec_check_method(k, m, sn.ctypes.data if sn.size else None, len(sn) if n is None else n, B,
                              None if av is None else av.ctypes.data, padlen, ctypes.byref(out))
    return rc, out.value


def test_symbols_resolve_and_abi_version_is_one():
    lib = _lib.load()
    for name in ("sec_check_method", "sec_ctx_check_methods"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.sec_abi_version() == 1
    assert "SEC_CHECK_BS" in engine.option_names()
    assert lib.sec_ctx_check_methods(None, None, None) == _lib.SEC_EINVAL


def test_option_listed_with_default_minus_one():
    assert engine.option_default("SEC_CHECK_BS") == -1
    assert len(engine.option_names()) <= 12


@pytest.mark.parametrize("k,m", SHAPES)
def test_eligible_with_shuffled_data_basis_and_any_parity_subset(k, m):
    rng = random.Random(k * 1000 + m)
    for trial in range(12):
        basis = list(range(k))
        rng.shuffle(basis)
        p = m - k
        rows = rng.sample(range(k, m), 1 if trial == 0 else p if trial == 1 else rng.randint(1, p))
        for B in (16, 17, 4096 + 21, (1 << 31) - 1):
            assert method(k, m, basis + rows, B) == (_lib.SEC_OK, 1), (basis, rows, B)
    # block k-1 (zfec's padded last block read in place) may be short; any other entry may not
    sn = list(range(k)) + [k, m - 1]
    full = [4096] * len(sn)
    short_last = list(full)
    short_last[k - 1] = 4096 - 7
    assert method(k, m, sn, 4096, short_last, 7) == (_lib.SEC_OK, 1)
    assert method(k, m, sn, 4096, full) == (_lib.SEC_OK, 1)
    over = [5000] * len(sn)  # avail counts to B at most
    assert method(k, m, sn, 4096, over) == (_lib.SEC_OK, 1)
    for e in (0, k, k + 1):
        short = list(full)
        short[e] = 4095
        assert method(k, m, sn, 4096, short) == (_lib.SEC_OK, 0), e
    # only output row k-1 may be short
    assert method(k, m, sn, 4096, None, 4095) == (_lib.SEC_OK, 1)
    assert method(k, m, sn, 4096, None, 4096) == (_lib.SEC_OK, 0)


def test_not_eligible():
    # a basis holding a parity row (a decode + check with a missing primary, too)
    assert method(16, 24, [0, 1, 2, 16] + list(range(4, 16)) + [3, 20], 4096) == (_lib.SEC_OK, 0)
    assert method(10, 14, list(range(1, 11)) + [0, 12], 4096) == (_lib.SEC_OK, 0)
    # a shape without the bit-sliced kernels
    assert method(4, 6, [0, 1, 2, 3, 4, 5], 4096) == (_lib.SEC_OK, 0)
    assert method(10, 15, list(range(15)), 4096) == (_lib.SEC_OK, 0)
    # n == k: nothing to check
    assert method(16, 24, list(range(16)), 4096) == (_lib.SEC_OK, 0)
    # B < 16: the tail kernel
    assert method(16, 24, list(range(24)), 15) == (_lib.SEC_OK, 0)
    assert method(16, 24, list(range(24)), 16) == (_lib.SEC_OK, 1)


def test_errors_are_sec_check_batch_s_in_its_order():
    E = _lib
    ok = list(range(10)) + [11, 13]
    assert method(10, 14, ok, 4096) == (E.SEC_OK, 1)
    lib = _lib.load()
    sn = np.asarray(ok, np.int32)
    assert lib.sec_check_method(10, 14, sn.ctypes.data, 12, 4096, None, 0, None) == E.SEC_EINVAL
    out = ctypes.c_int(0)
    assert lib.sec_check_method(10, 14, None, 12, 4096, None, 0, ctypes.byref(out)) == E.SEC_EINVAL
    assert lib.sec_check_method(10, 14, sn.ctypes.data, 12, 4096, None, -1, ctypes.byref(out)) == E.SEC_EINVAL
    # SEC_EINVAL (n < 0) before SEC_EKM before SEC_ENBLOCKS before SEC_ESHARENUM before SEC_EDUPSHARE
    # before SEC_ESIZE: each case carries every later fault as well
    bad = [0, 0, 99] + list(range(3, 10)) + [11, 13]  # a repeat and an out-of-range number
    big = 1 << 31
    assert method(0, 14, bad, big, n=-1)[0] == E.SEC_EINVAL
    assert method(0, 14, bad, big, n=3)[0] == E.SEC_EKM
    assert method(15, 14, bad, big)[0] == E.SEC_EKM
    assert method(10, 257, bad, big)[0] == E.SEC_EKM
    assert method(10, 14, bad, big, n=9)[0] == E.SEC_ENBLOCKS
    assert method(10, 11, bad, big)[0] == E.SEC_ENBLOCKS  # n > m
    assert method(10, 14, bad, big)[0] == E.SEC_ESHARENUM  # the range error, though the repeat comes first
    dup = [0, 0] + list(range(2, 10)) + [11, 13]
    assert method(10, 14, dup, big)[0] == E.SEC_EDUPSHARE
    assert method(10, 14, ok[:11] + [11], big)[0] == E.SEC_EDUPSHARE  # a check row held twice
    assert method(10, 14, ok, big)[0] == E.SEC_ESIZE
    assert method(10, 14, ok, big - 1) == (E.SEC_OK, 1)
    # an error leaves *method alone
    assert method(10, 14, dup, 4096) == (E.SEC_EDUPSHARE, -7)
