"""CPU: sec_repair_matrix, the host arithmetic of piece repair.  Block t of the code word is a
fixed GF(2^8) combination of any k other blocks; the returned matrix, applied with the oracle's
matrix product to the source blocks of a small chunk, must give the oracle's own block t
(oracle/fec_oracle.c through cfec.easy_encode), for data and parity targets alike.  Also the
error table and the layout of sec_rep_chunk."""

import ctypes
import random

import numpy as np
import pytest

from oracle import cfec, zfec_ref
from storb_amd import _lib, engine

SHAPES = [(1, 3), (3, 7), (4, 6), (10, 14), (16, 24), (64, 96)]
B = 7


def _subsets(k, m):
    """(name, k source sharenums in the order handed over) for one shape, seeded."""
    rng = random.Random(1000 * k + m)
    out = []
    if m - k >= 1:
        out.append(("primary", list(range(k))))  # all-primary sources: only parity is left to repair
    if m - k >= k:
        out.append(("secondary", rng.sample(range(k, m), k)))  # no primary among the sources
    if m > k:
        for i in range(3):
            s = rng.sample(range(m), k)  # mixed, in shuffled order
            out.append((f"mixed{i}", s))
    return out


def _cases():
    for k, m in SHAPES:
        for name, src in _subsets(k, m):
            yield pytest.param(k, m, src, id=f"k{k}m{m}-{name}")


@pytest.fixture(scope="module")
def encoded():
    """Per shape: the oracle's m blocks of one seeded chunk with B = 7 and a padded last block."""
    out = {}
    for k, m in SHAPES:
        n = k * B - (2 if k > 1 else 0)
        data = bytes(random.Random(k * 31 + m).randrange(256) for _ in range(n))
        blocks = cfec.easy_encode(data, k, m)
        assert len(blocks) == m and all(len(b) == B for b in blocks)
        out[(k, m)] = blocks
    return out


@pytest.mark.parametrize("k,m,src", list(_cases()))
def test_matrix_rebuilds_oracle_blocks(encoded, k, m, src):
    blocks = encoded[(k, m)]
    rng = random.Random(sum(src) + 7 * k)
    lost = [t for t in range(m) if t not in src]
    targets = rng.sample(lost, len(lost))  # every lost block, unsorted
    if len(targets) > 1 and targets == sorted(targets):
        targets.reverse()
    rm = np.frombuffer(engine.repair_matrix(k, m, src, targets), np.uint8).reshape(len(targets), k)
    have = np.stack([np.frombuffer(blocks[s], np.uint8) for s in src])
    got = zfec_ref.gf_matmul(rm, have)
    for r, t in enumerate(targets):
        assert got[r].tobytes() == blocks[t], (t, src)
    # a subset of the targets gives the same rows
    some = targets[::2]
    rm2 = np.frombuffer(engine.repair_matrix(k, m, src, some), np.uint8).reshape(len(some), k)
    assert rm2.tobytes() == rm[::2].tobytes()


def test_data_target_rows_are_the_decode_matrix_rows():
    k, m, src = 4, 6, [5, 0, 3, 2]
    rm = engine.repair_matrix(k, m, src, [1])
    enc = zfec_ref.encode_matrix(k, m)
    minv = zfec_ref.gf_invert(enc[src])  # rows in the caller's order: columns come out in that order too
    assert rm == minv[1].tobytes()


def _call(k, m, src, tg, nt=None, out=True):
    lib = _lib.load()
    sn = np.array(src, np.int32)
    t = np.array(tg, np.int32)
    o = np.zeros(max(len(tg) * max(k, 1), 1), np.uint8)
    return lib.sec_repair_matrix(k, m, sn.ctypes.data if sn.size else None, t.ctypes.data if t.size else None,
                                 len(tg) if nt is None else nt, o.ctypes.data if out else None), o


def test_error_table():
    ok = [0, 2, 3, 4]
    assert _call(4, 6, ok, [1, 5])[0] == _lib.SEC_OK
    for k, m in [(0, 3), (5, 4), (4, 257)]:
        assert _call(k, m, ok, [1])[0] == _lib.SEC_EKM, (k, m)
    assert _call(4, 6, [0, 2, 3, 6], [1])[0] == _lib.SEC_ESHARENUM  # source >= m
    assert _call(4, 6, [0, 2, 3, -1], [1])[0] == _lib.SEC_ESHARENUM
    assert _call(4, 6, ok, [6])[0] == _lib.SEC_ESHARENUM  # target >= m
    assert _call(4, 6, ok, [-1])[0] == _lib.SEC_ESHARENUM
    assert _call(4, 6, [0, 2, 2, 4], [1])[0] == _lib.SEC_EDUPSHARE  # repeated source
    assert _call(4, 6, ok, [1, 1])[0] == _lib.SEC_EDUPSHARE  # repeated target
    assert _call(4, 6, ok, [1, 3])[0] == _lib.SEC_EDUPSHARE  # a target that is also a source
    assert _call(4, 6, ok, [1], nt=-1)[0] == _lib.SEC_EINVAL
    assert _call(4, 6, ok, [1], out=False)[0] == _lib.SEC_EINVAL
    for bad in ([0, 2, 2, 4], [0, 2, 3, 6]):  # the Python surface raises zfec-style errors
        with pytest.raises(engine.Error):
            engine.repair_matrix(4, 6, bad, [1])
    with pytest.raises(engine.Error):
        engine.repair_matrix(4, 6, ok, [3])
    with pytest.raises(engine.Error):
        engine.repair_matrix(4, 6, [0, 2, 3], [1])  # not k sharenums


def test_no_targets_is_valid_and_writes_nothing():
    rc, o = _call(4, 6, [0, 2, 3, 4], [], nt=0)
    assert rc == _lib.SEC_OK and not o.any()
    lib = _lib.load()
    sn = np.array([0, 2, 3, 4], np.int32)
    assert lib.sec_repair_matrix(4, 6, sn.ctypes.data, None, 0, None) == _lib.SEC_OK
    assert engine.repair_matrix(4, 6, [0, 2, 3, 4], []) == b""


def test_rep_chunk_layout():
    assert ctypes.sizeof(_lib.sec_rep_chunk) == 40
    assert _lib.REP_DTYPE.itemsize == 40
    assert _lib.REP_DTYPE.names == tuple(f for f, _ in _lib.sec_rep_chunk._fields_)
    for name, _ in _lib.sec_rep_chunk._fields_:
        assert _lib.REP_DTYPE.fields[name][1] == getattr(_lib.sec_rep_chunk, name).offset, name
    assert {"sec_repair_matrix", "sec_repair_batch"} <= set(_lib.SYMBOLS)


def test_check_repair_item_raises_like_the_library():
    blocks = [b"ab"] * 4
    engine.check_repair_item(4, 6, blocks, [0, 2, 3, 4], [1, 5])
    for args in [(4, 6, blocks[:3], [0, 2, 3], [1]), (4, 6, [b"ab", b"ab", b"a", b"ab"], [0, 2, 3, 4], [1]),
                 (5, 4, blocks + [b"ab"], [0, 1, 2, 3, 4], []), (4, 6, blocks, [0, 2, 3, 4], [6]),
                 (4, 6, blocks, [0, 2, 3, 4], [1, 1]), (4, 6, blocks, [0, 2, 3, 4], [2])]:
        with pytest.raises(engine.Error):
            engine.check_repair_item(*args)
