"""CPU: sec_check_locate / engine.check_locate, the host arithmetic that names the one entry whose
change explains an inconsistent column of a check.  Columns come from the oracle's code words
(cfec.easy_encode); errors are put in here, so every expectation is where the test put them."""

import ctypes
import random

import numpy as np
import pytest

from oracle import cfec
from storb_amd import _lib
from storb_amd.engine import Error, check_locate


def _column(k, m, sharenums, seed, t=1, B=3):
    """Byte t of blocks `sharenums` of a seeded random code word."""
    data = bytes(random.Random(seed).randrange(256) for _ in range(k * B))
    blocks = cfec.easy_encode(data, k, m)
    return bytearray(blocks[s][t] for s in sharenums)


def _exhaustive(k, m, sharenums, seed):
    col = _column(k, m, sharenums, seed)
    assert check_locate(k, m, sharenums, col) == -1
    for i in range(len(sharenums)):
        for e in range(1, 256):
            bad = bytearray(col)
            bad[i] ^= e
            assert check_locate(k, m, sharenums, bad) == i, (i, e)


def test_rs46_every_entry_every_error():
    _exhaustive(4, 6, [0, 1, 2, 3, 4, 5], seed=46)


def test_rs46_shuffled_basis():
    _exhaustive(4, 6, [5, 0, 3, 2, 4, 1], seed=47)
    _exhaustive(4, 6, [4, 5, 1, 0, 2, 3], seed=48)  # both parity rows in the basis, data rows checked


@pytest.mark.parametrize("k,m", [(10, 14), (3, 12), (16, 24), (64, 96)])
def test_spot_checks(k, m):
    rng = random.Random(1000 * k + m)
    for trial in range(4):
        sharenums = rng.sample(range(m), m)  # every block held, any k of them the basis
        col = _column(k, m, sharenums, seed=rng.randrange(1 << 30))
        assert check_locate(k, m, sharenums, col) == -1
        for _ in range(12):
            i, e = rng.randrange(m), rng.randrange(1, 256)
            bad = bytearray(col)
            bad[i] ^= e
            assert check_locate(k, m, sharenums, bad) == i
    # fewer held: n = k + 2, the least that can locate
    sharenums = rng.sample(range(m), k + 2)
    col = _column(k, m, sharenums, seed=7)
    for i in range(k + 2):
        bad = bytearray(col)
        bad[i] ^= rng.randrange(1, 256)
        assert check_locate(k, m, sharenums, bad) == i


@pytest.mark.parametrize("k,m,sharenums", [(4, 6, [5, 0, 3, 2, 1]), (10, 14, list(range(11))), (1, 3, [2, 0])])
def test_one_check_row_cannot_locate(k, m, sharenums):
    col = _column(k, m, sharenums, seed=5)
    assert check_locate(k, m, sharenums, col) == -1
    for i in range(len(sharenums)):
        bad = bytearray(col)
        bad[i] ^= 0x5A
        assert check_locate(k, m, sharenums, bad) == -2
    assert check_locate(k, m, sharenums[:k], col[:k]) == -1  # nothing to check: any column is a code word


@pytest.mark.parametrize("k,m", [(4, 6), (4, 8), (10, 14), (3, 12)])
def test_two_errors_are_never_a_code_word(k, m):
    """Two errors leave the column inconsistent (n - k >= 2).  With exactly two check rows they may
    mimic a single other error, so no more is asserted there; with three or more no three columns
    of [R | I] are dependent (MDS), so no single entry explains them."""
    rng = random.Random(k * m)
    sharenums = rng.sample(range(m), m)
    col = _column(k, m, sharenums, seed=11)
    for _ in range(300):
        i, j = rng.sample(range(m), 2)
        bad = bytearray(col)
        bad[i] ^= rng.randrange(1, 256)
        bad[j] ^= rng.randrange(1, 256)
        who = check_locate(k, m, sharenums, bad)
        assert who != -1
        if m - k >= 3:
            assert who == -2


def _rc(k, m, sharenums, n=None, column=True, culprit=True):
    lib = _lib.load()
    sn = None if sharenums is None else np.array(sharenums, np.int32)
    n = (0 if sn is None else sn.size) if n is None else n
    col = np.zeros(max(n, 1), np.uint8)
    who = ctypes.c_int32(7)
    return lib.sec_check_locate(k, m, None if sn is None else sn.ctypes.data, n, col.ctypes.data if column else None,
                                ctypes.byref(who) if culprit else None)


def _repair_matrix_rc(k, m, sharenums, n=None):
    lib = _lib.load()
    sn = None if sharenums is None else np.array(sharenums, np.int32)
    n = (0 if sn is None else sn.size) if n is None else n
    out = np.zeros(256 * 256, np.uint8)
    return lib.sec_repair_matrix(k, m, None if sn is None else sn.ctypes.data,
                                 None if sn is None else sn.ctypes.data + 4 * k, n - k, out.ctypes.data)


@pytest.mark.parametrize("k,m,sharenums,n,want", [
    (4, 6, [0, 1, 2, 3, 4, 5], None, _lib.SEC_OK),
    (4, 6, [0, 1, 2], None, _lib.SEC_EINVAL),           # n < k
    (4, 6, None, 6, _lib.SEC_EINVAL),                   # no sharenums
    (0, 6, [0, 1, 2, 3], None, _lib.SEC_EKM),
    (5, 4, [0, 1, 2, 3, 4], None, _lib.SEC_EKM),
    (4, 257, [0, 1, 2, 3, 4], None, _lib.SEC_EKM),
    (4, 6, [0, 1, 2, 6, 4, 5], None, _lib.SEC_ESHARENUM),
    (4, 6, [0, 1, 2, 3, 4, -1], None, _lib.SEC_ESHARENUM),
    (4, 6, [0, 1, 1, 3, 4, 5], None, _lib.SEC_EDUPSHARE),
    (4, 6, [0, 1, 2, 3, 4, 4], None, _lib.SEC_EDUPSHARE),
    (4, 6, [0, 1, 2, 3, 4, 2], None, _lib.SEC_EDUPSHARE),
    (4, 6, [0, 1, 6, 1, 4, 5], None, _lib.SEC_ESHARENUM),  # the first bad basis entry decides
])
def test_validation_is_repair_matrix_s(k, m, sharenums, n, want):
    assert _rc(k, m, sharenums, n) == want
    assert _repair_matrix_rc(k, m, sharenums, n) == want


def test_null_outputs_and_wrapper_errors():
    assert _rc(4, 6, [0, 1, 2, 3, 4, 5], column=False) == _lib.SEC_EINVAL
    assert _rc(4, 6, [0, 1, 2, 3, 4, 5], culprit=False) == _lib.SEC_EINVAL
    with pytest.raises(Error):
        check_locate(4, 6, [0, 1, 2, 3, 4, 4], bytes(6))
    with pytest.raises(ValueError):
        check_locate(4, 6, [0, 1, 2, 3, 4, 5], bytes(5))
