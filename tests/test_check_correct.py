"""CPU: sec_check_correct / engine.check_correct, the one-column model of the correcting calls with
several errors per position, against a brute force written here on oracle.zfec_ref: for a column and
a bound t, every subset of at most t entries in ascending size is erased, the rest checked for
consistency, and the first subset whose rest is consistent gives the code word.  Columns come from
the oracle's code words (cfec.easy_encode); errors are put in here."""

import ctypes
import itertools
import random

import numpy as np
import pytest

from oracle import cfec, zfec_ref
from storb_amd import _lib
from storb_amd.engine import Error, check_correct, check_locate


def _bound(r, max_errors):
    t = min(r // 2, 16)
    return t if max_errors == 0 else min(t, max_errors)


def _brute(k, m, sharenums, cols, t):
    """cols: n x N columns.  Per column (fixed n bytes, nchanged): the code word within t entries
    found by erasing subsets in ascending size, or (the column, -2)."""
    n, N = cols.shape
    G = zfec_ref.encode_matrix(k, m)[list(sharenums)]
    fixed = cols.copy()
    changed = np.full(N, -2, dtype=np.int64)
    for size in range(t + 1):
        for E in itertools.combinations(range(n), size):
            todo = np.nonzero(changed == -2)[0]
            if todo.size == 0:
                return fixed, changed
            rest = [j for j in range(n) if j not in E]
            P = zfec_ref.gf_matmul(G, zfec_ref.gf_invert(G[rest[:k]]))  # the code word from k of the rest
            word = zfec_ref.gf_matmul(P, cols[rest[:k]][:, todo])
            ok = (word[rest] == cols[rest][:, todo]).all(axis=0)
            hit = todo[ok]
            fixed[:, hit] = word[:, ok]
            changed[hit] = (word[:, ok] != cols[:, hit]).sum(axis=0)
    return fixed, changed


def _code_columns(k, m, sharenums, seed, N):
    data = bytes(random.Random(seed).randrange(256) for _ in range(k * N))
    blocks = cfec.easy_encode(data, k, m)
    return np.array([list(blocks[s][:N]) for s in sharenums], dtype=np.uint8)


def _held_sets(k, m, rng):
    """Held lists with and without piece 0, piece 0 in the basis and among the check rows."""
    every = list(range(m))
    rng.shuffle(every)
    zero_last = [s for s in every if s != 0] + [0]            # piece 0 a check row
    zero_first = [0] + [s for s in every if s != 0]           # piece 0 in the basis
    without = [s for s in every if s != 0]                    # n = m - 1
    fewer = [0] + rng.sample(range(1, m), max(k + 2, m - 2) - 1)
    rng.shuffle(fewer)
    return [every, zero_last, zero_first, without, fewer]


CASES = [(4, 6, 0), (8, 11, 0), (8, 12, 0), (10, 14, 0), (16, 24, 2)]  # (k, m, cap on t: 0 = none)


@pytest.mark.parametrize("k,m,cap", CASES)
@pytest.mark.parametrize("max_errors", [0, 1, 2])
def test_against_brute_force(k, m, cap, max_errors):
    if cap and (max_errors == 0 or max_errors > cap):
        max_errors = cap  # (16,24): t capped at 2 so the subset count stays small
    rng = random.Random(97 * k + m + 1000 * max_errors)
    for sharenums in _held_sets(k, m, rng):
        n, r = len(sharenums), len(sharenums) - k
        t = _bound(r, max_errors)
        clean = _code_columns(k, m, sharenums, rng.randrange(1 << 30), 24)
        cols, want_fixed, want_changed = [], [], []
        counts = list(range(0, t + 1)) + list(range(t + 1, r - t + 1))
        zero = sharenums.index(0) if 0 in sharenums else None
        for c, ne in enumerate(counts * 3):
            col = clean[:, c % clean.shape[1]].copy()
            where = rng.sample(range(n), ne)
            if zero is not None and ne and c % 2 == 0 and zero not in where:
                where[0] = zero  # piece 0 among the errors
            for j in where:
                col[j] ^= rng.randrange(1, 256)
            cols.append(col)
            want_fixed.append(clean[:, c % clean.shape[1]] if ne <= t else col)
            want_changed.append(ne if ne <= t else -2)
        cols = np.array(cols, dtype=np.uint8).T
        bf_fixed, bf_changed = _brute(k, m, sharenums, cols, t)
        for c in range(cols.shape[1]):
            fixed, changed = check_correct(k, m, sharenums, cols[:, c].tobytes(), max_errors)
            assert changed == want_changed[c], (sharenums, c)
            assert fixed == want_fixed[c].tobytes(), (sharenums, c)
            assert changed == bf_changed[c] and fixed == bf_fixed[:, c].tobytes(), (sharenums, c)
            if max_errors == 1:
                who = check_locate(k, m, sharenums, cols[:, c].tobytes())
                if who == -1:
                    assert changed == 0
                elif who == -2:
                    assert changed == -2
                else:
                    assert changed == 1
                    assert [j for j in range(n) if fixed[j] != cols[j, c]] == [who]


@pytest.mark.parametrize("k,m", [(4, 6), (8, 12), (10, 14)])
def test_any_column_agrees_with_brute_force(k, m):
    """Columns with more errors than r - t, and plain noise: the verdict is whatever code word lies
    within t, if any, which the brute force finds independently."""
    rng = random.Random(k * 31 + m)
    sharenums = rng.sample(range(m), m)
    n, r = m, m - k
    t = r // 2
    clean = _code_columns(k, m, sharenums, 5, 40)
    cols = []
    for c in range(40):
        col = clean[:, c].copy()
        for j in rng.sample(range(n), rng.randrange(r - t + 1, n + 1)):
            col[j] ^= rng.randrange(1, 256)
        cols.append(col)
    cols = np.array(cols, dtype=np.uint8).T
    bf_fixed, bf_changed = _brute(k, m, sharenums, cols, t)
    for c in range(cols.shape[1]):
        fixed, changed = check_correct(k, m, sharenums, cols[:, c].tobytes(), 0)
        assert changed == bf_changed[c] and fixed == bf_fixed[:, c].tobytes(), c
    for s in (sharenums, sharenums[:k + 1], sharenums[:k]):  # max_errors = 1 is check_locate on any column
        for c in range(cols.shape[1]):
            col = cols[:len(s), c].tobytes()
            who = check_locate(k, m, s, col)
            fixed, changed = check_correct(k, m, s, col, 1)
            assert changed == {-1: 0, -2: -2}.get(who, 1)
            assert [j for j in range(len(s)) if fixed[j] != col[j]] == ([who] if who >= 0 else [])


def test_zfec_64_96_sixteen_errors():
    k, m = 64, 96
    rng = random.Random(6496)
    sharenums = rng.sample(range(m), m)
    clean = _code_columns(k, m, sharenums, 3, 8)
    for c in range(8):
        for ne in (1, 15, 16):
            col = clean[:, c].copy()
            for j in rng.sample(range(m), ne):
                col[j] ^= rng.randrange(1, 256)
            assert check_correct(k, m, sharenums, col.tobytes(), 0) == (clean[:, c].tobytes(), ne)
        col = clean[:, c].copy()
        for j in rng.sample(range(m), 17):  # t + 1 = r - t + 1 here: always open
            col[j] ^= rng.randrange(1, 256)
        assert check_correct(k, m, sharenums, col.tobytes(), 0) == (col.tobytes(), -2)
        assert check_correct(k, m, sharenums, col.tobytes(), 40) == (col.tobytes(), -2)  # T past 16 is 16


def _rc(k, m, sharenums, max_errors=0, column=True, fixed=True, nchanged=True):
    lib = _lib.load()
    sn = np.array(sharenums, np.int32)
    col = np.zeros(max(sn.size, 1), np.uint8)
    out = np.zeros(max(sn.size, 1), np.uint8)
    ch = ctypes.c_int32(7)
    return lib.sec_check_correct(k, m, sn.ctypes.data, sn.size, col.ctypes.data if column else None, max_errors,
                                 out.ctypes.data if fixed else None, ctypes.byref(ch) if nchanged else None)


def test_errors():
    ok = [0, 1, 2, 3, 4, 5]
    assert _rc(4, 6, ok) == _lib.SEC_OK
    assert _rc(4, 6, ok, max_errors=-1) == _lib.SEC_EINVAL
    assert _rc(4, 6, ok, column=False) == _lib.SEC_EINVAL
    assert _rc(4, 6, ok, fixed=False) == _lib.SEC_EINVAL
    assert _rc(4, 6, ok, nchanged=False) == _lib.SEC_EINVAL
    assert _rc(0, 6, ok) == _lib.SEC_EKM
    assert _rc(4, 6, [0, 1, 2, 3, 4, 6]) == _lib.SEC_ESHARENUM
    assert _rc(4, 6, [0, 1, 2, 3, 4, 4]) == _lib.SEC_EDUPSHARE
    assert _rc(4, 6, [0, 1, 2]) == _lib.SEC_EINVAL  # n < k, as sec_check_locate
    with pytest.raises(Error):
        check_correct(4, 6, [0, 1, 2, 3, 4, 4], bytes(6))
    with pytest.raises(ValueError):
        check_correct(4, 6, ok, bytes(6), -1)
    with pytest.raises(ValueError):
        check_correct(4, 6, ok, bytes(5))
