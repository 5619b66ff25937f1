"""CPU: the ABI additions of the bit-sliced repair: sec_repair_method (host logic: which chunks of a
repair or a repair + check are eligible for sec_repair_bs_kernel) and sec_ctx_repair_methods.  The
kernel's choice rides on the existing context option SEC_CHECK_BS: no option is added.  No device is
needed."""

import ctypes
import random

import numpy as np
import pytest

from storb_amd import _lib, engine

SHAPES = [(10, 14), (8, 12), (16, 24), (32, 48), (64, 96), (8, 11)]
# the option list as it stood before this call was added: it is full, and stays as it is
OPTIONS_BEFORE = 12


def method(k, m, sharenums, targets, B, avail=None, n=None, nt=None):
    lib = _lib.load()
    sn = np.asarray(sharenums, np.int32)
    tg = np.asarray(targets, np.int32)
    av = None if avail is None else np.asarray(avail, np.uint64)
    out = ctypes.c_int(-7)
    rc = lib.sec_repair_method(k, m, sn.ctypes.data if sn.size else None, len(sn) if n is None else n,
                               tg.ctypes.data if tg.size else None, len(tg) if nt is None else nt, B,
                               None if av is None else av.ctypes.data, ctypes.byref(out))
    return rc, out.value


def test_symbols_resolve_and_abi_version_is_one():
    lib = _lib.load()
    for name in ("sec_repair_method", "sec_ctx_repair_methods"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.sec_abi_version() == 1
    assert lib.sec_ctx_repair_methods(None, None, None) == _lib.SEC_EINVAL
    b, d = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.sec_ctx_repair_methods(None, ctypes.byref(b), ctypes.byref(d)) == _lib.SEC_EINVAL


def test_no_new_option():
    names = engine.option_names()
    assert len(names) <= OPTIONS_BEFORE
    assert "SEC_CHECK_BS" in names and engine.option_default("SEC_CHECK_BS") == -1
    assert not [n for n in names if "REPAIR" in n or "RBS" in n]


@pytest.mark.parametrize("k,m", SHAPES)
def test_eligible_with_shuffled_data_basis_and_any_target_subset(k, m):
    rng = random.Random(k * 1000 + m)
    p = m - k
    for trial in range(12):
        basis = list(range(k))
        rng.shuffle(basis)
        parity = rng.sample(range(k, m), p)
        nt = 1 if trial == 0 else p if trial == 1 else rng.randint(1, p)
        targets, rest = parity[:nt], parity[nt:]
        held = rest[:rng.randint(0, len(rest))]  # a repair + check holds some of the others, or none
        for B in (16, 17, 4096 + 21, (1 << 31) - 1):
            assert method(k, m, basis, targets, B) == (_lib.SEC_OK, 1), (basis, targets, B)  # plain repair: n == k
            assert method(k, m, basis + held, targets, B) == (_lib.SEC_OK, 1), (basis, held, targets, B)
    # the module function says the same
    assert engine.repair_method(k, m, list(range(k)), [k], 4096) is True
    assert engine.repair_method(k, m, list(range(k)) + [m - 1], [k], 4096, avail=[4096] * (k + 1)) is True
    # block k-1 (zfec's padded last block read in place) may be short; any other entry may not
    sn = list(range(k)) + [k, m - 1]
    tg = [k + 1]
    full = [4096] * len(sn)
    short_last = list(full)
    short_last[k - 1] = 4096 - 7
    assert method(k, m, sn, tg, 4096, short_last) == (_lib.SEC_OK, 1)
    assert method(k, m, sn, tg, 4096, full) == (_lib.SEC_OK, 1)
    assert method(k, m, sn, tg, 4096, [5000] * len(sn)) == (_lib.SEC_OK, 1)  # avail counts to B at most
    for e in (0, k, k + 1):
        short = list(full)
        short[e] = 4095
        assert method(k, m, sn, tg, 4096, short) == (_lib.SEC_OK, 0), e
    assert engine.repair_method(k, m, sn, tg, 4096, avail=short) is False
    # no target but a check row: a row all the same (eligibility alone; such a chunk stays direct)
    assert method(k, m, sn, [], 4096) == (_lib.SEC_OK, 1)


def test_not_eligible():
    # a basis holding a parity row
    assert method(16, 24, [0, 1, 2, 16] + list(range(4, 16)) + [20], [3, 21], 4096) == (_lib.SEC_OK, 0)
    assert method(16, 24, [0, 1, 2, 16] + list(range(4, 16)), [3], 4096) == (_lib.SEC_OK, 0)
    assert method(10, 14, list(range(1, 11)) + [12], [0], 4096) == (_lib.SEC_OK, 0)
    # a shape without the bit-sliced kernels
    assert method(4, 6, [0, 1, 2, 3], [4, 5], 4096) == (_lib.SEC_OK, 0)
    assert method(10, 15, list(range(10)), [12], 4096) == (_lib.SEC_OK, 0)
    # B < 16: the tail kernel
    assert method(16, 24, list(range(16)), [16], 15) == (_lib.SEC_OK, 0)
    assert method(16, 24, list(range(16)), [16], 16) == (_lib.SEC_OK, 1)
    # no target and no check row: nothing to do
    assert method(16, 24, list(range(16)), [], 4096) == (_lib.SEC_OK, 0)


def test_errors_are_sec_repair_check_batch_s_in_its_order():
    E = _lib
    ok, tg = list(range(10)) + [11], [12, 13]
    assert method(10, 14, ok, tg, 4096) == (E.SEC_OK, 1)
    lib = _lib.load()
    sn, tn = np.asarray(ok, np.int32), np.asarray(tg, np.int32)
    assert lib.sec_repair_method(10, 14, sn.ctypes.data, 11, tn.ctypes.data, 2, 4096, None, None) == E.SEC_EINVAL
    out = ctypes.c_int(0)
    assert lib.sec_repair_method(10, 14, None, 11, tn.ctypes.data, 2, 4096, None, ctypes.byref(out)) == E.SEC_EINVAL
    assert lib.sec_repair_method(10, 14, sn.ctypes.data, 11, None, 2, 4096, None, ctypes.byref(out)) == E.SEC_EINVAL
    # SEC_EINVAL (n < 0, ntargets < 0) before SEC_EKM before SEC_ENBLOCKS before SEC_ESHARENUM before
    # SEC_EDUPSHARE before SEC_ESIZE: each case carries every later fault as well
    bad = [0, 0, 99] + list(range(3, 10)) + [11]  # a repeat and an out-of-range number
    big = 1 << 31
    assert method(0, 14, bad, tg, big, n=-1)[0] == E.SEC_EINVAL
    assert method(0, 14, bad, tg, big, nt=-1)[0] == E.SEC_EINVAL
    assert method(0, 14, bad, tg, big, n=3)[0] == E.SEC_EKM
    assert method(15, 14, bad, tg, big)[0] == E.SEC_EKM
    assert method(10, 257, bad, tg, big)[0] == E.SEC_EKM
    assert method(10, 14, bad, tg, big, n=9)[0] == E.SEC_ENBLOCKS
    assert method(10, 10, bad, tg, big)[0] == E.SEC_ENBLOCKS  # n > m
    assert method(10, 14, bad, tg, big)[0] == E.SEC_ESHARENUM  # the range error, though the repeat comes first
    dup = [0, 0] + list(range(2, 10)) + [11]
    assert method(10, 14, dup, [12, 14], big)[0] == E.SEC_ESHARENUM  # a target out of range, before the repeat
    assert method(10, 14, dup, tg, big)[0] == E.SEC_EDUPSHARE
    assert method(10, 14, ok, [12, 12], big)[0] == E.SEC_EDUPSHARE  # a repeated target
    assert method(10, 14, ok, [11], big)[0] == E.SEC_EDUPSHARE  # a target that is held
    assert method(10, 14, ok, tg, big)[0] == E.SEC_ESIZE
    assert method(10, 14, ok, tg, big - 1) == (E.SEC_OK, 1)
    # an error leaves *method alone
    assert method(10, 14, dup, tg, 4096) == (E.SEC_EDUPSHARE, -7)
