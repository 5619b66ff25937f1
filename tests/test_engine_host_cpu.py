"""The engine's host methods (encode_host*, decode_host*) on a CPU-only machine.

An ``Engine`` made with ``Engine.__new__`` gets a fake ``lib`` that implements, on the oracle
(oracle/cfec.py, hashlib), exactly the entry points these methods call.  Each fake reads its
descriptor and address arguments the way the library does (the ``_lib`` dtypes at the addresses
passed) and writes its results to the addresses it was given, so what is checked is the Python
side: descriptor layout, result slicing, clipping by padlen and the joins.  Every expected value
comes from the oracle, never from the code under test.
"""

import ctypes
import hashlib

import numpy as np
import pytest

from oracle import cfec
from storb_amd._lib import COPY_DTYPE, DEC_DTYPE, ENC_DTYPE, SEC_F_ASYNC, SEC_F_HOST, SEC_F_RECOVER, SEC_F_STAGED
from storb_amd.engine import Engine

# (k, m, n): (4, 6, 17) is ragged, (3, 3, 10) has no parity, (2, 3, 0) is an empty chunk
SHAPES = [(1, 2, 1), (4, 6, 17), (3, 3, 10), (16, 24, 100), (2, 3, 0), (8, 11, 4097)]


def _padded_encode(chunk, k, m):
    """easy_encode written out on the oracle's own matrix and field: the chunk zero-padded to k*B,
    cut into k blocks, and rows k..m-1 of ``cfec.encode_matrix`` applied to them."""
    B = -(-len(chunk) // k)
    data = chunk + b"\0" * (k * B - len(chunk))
    blocks = [data[j * B:(j + 1) * B] for j in range(k)]
    rows, mul = cfec.encode_matrix(k, m), cfec.lib().fo_gf_mul
    for r in range(k, m):
        acc = bytearray(B)
        for j in range(k):
            c = rows[r * k + j]
            for x in range(B):
                acc[x] ^= mul(c, blocks[j][x])
        blocks.append(bytes(acc))
    return blocks


def _oracle_encode(chunk, k, m):
    """easy_encode's m blocks.  (16, 24, 100) has more padding (12 bytes) than one block holds
    (B = 7), which easy_encode refuses as easyfec does (and libstorbec: SEC_EBLOCKLEN); its
    blocks come from _padded_encode, the same construction (test_padded_encode_is_easy_encode),
    so that the shape still exercises the descriptor layout and a padlen that drops a whole row."""
    if k == 1 or (k - 1) * -(-len(chunk) // k) <= len(chunk):
        return cfec.easy_encode(chunk, k, m)
    return _padded_encode(chunk, k, m)


def _records(ptr, n, dtype):
    if not n:
        return np.zeros(0, dtype=dtype)
    raw = (ctypes.c_char * (n * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(raw, dtype=dtype)


def _read(ptr, n):
    return ctypes.string_at(ptr, n) if n else b""


def _write(ptr, data):
    if data:
        ctypes.memmove(ptr, data, len(data))


class FakeLib:
    """The entry points of libstorbec.so that the engine's host encode / decode methods call."""

    def __init__(self):
        self.calls = []  # (entry point, chunks or jobs, flags or None)

    def sec_strerror(self, code):
        return b"fake status %d" % code

    def sec_ctx_destroy(self, ctx):
        pass

    def _encode(self, descs, n, src, parity, digests, flags):
        assert flags & SEC_F_HOST and not flags & SEC_F_ASYNC
        slot = 0
        for d in _records(descs, n, ENC_DTYPE):
            k, m, ln = int(d["k"]), int(d["m"]), int(d["n"])
            blocks = _oracle_encode(_read((src or 0) + int(d["in_off"]), ln), k, m)
            assert int(d["parity_stride"]) >= max(len(blocks[0]), 1)
            for r in range(m - k):
                _write((parity or 0) + int(d["parity_off"]) + r * int(d["parity_stride"]), blocks[k + r])
            if digests:
                for j, b in enumerate(blocks):
                    _write(digests + 20 * (slot + j), hashlib.sha1(b).digest())
            slot += m
        return 0

    def sec_encode_batch(self, ctx, descs, n, src, parity, flags):
        self.calls.append(("sec_encode_batch", n, flags))
        return self._encode(descs, n, src, parity, None, flags)

    def sec_encode_digest_batch(self, ctx, descs, n, src, parity, digests, flags):
        self.calls.append(("sec_encode_digest_batch", n, flags))
        assert digests
        return self._encode(descs, n, src, parity, digests, flags)

    def sec_decode_batch_ex(self, ctx, descs, n, sharenums, block_offs, block_avail, blocks, out, flags):
        self.calls.append(("sec_decode_batch_ex", n, flags))
        assert flags & SEC_F_HOST and not flags & SEC_F_ASYNC and block_avail is None
        ds = _records(descs, n, DEC_DTYPE)
        nslots = max((int(d["slot0"]) + int(d["k"]) for d in ds), default=0)
        sn = _records(sharenums, nslots, np.dtype("<i4"))
        bo = _records(block_offs, nslots, np.dtype("<u8"))
        for d in ds:
            k, m, B, padlen, s0 = int(d["k"]), int(d["m"]), int(d["B"]), int(d["padlen"]), int(d["slot0"])
            if not B:
                continue
            nums = [int(x) for x in sn[s0:s0 + k]]
            held = [_read((blocks or 0) + int(a), B) for a in bo[s0:s0 + k]]
            dst = (out or 0) + int(d["out_off"])
            if flags & SEC_F_RECOVER:  # only the missing primaries, in primary order
                whole = cfec.easy_decode(held, nums, 0, k, m)
                missing = [j for j in range(k) if j not in nums]
                _write(dst, b"".join(whole[j * B:(j + 1) * B] for j in missing))
            else:
                _write(dst, cfec.easy_decode(held, nums, padlen, k, m))
        return 0

    def sec_host_copy(self, ctx, jobs, n):
        self.calls.append(("sec_host_copy", n, None))
        for j in _records(jobs, n, COPY_DTYPE):
            if not int(j["len"]):
                continue
            if int(j["src"]):
                ctypes.memmove(int(j["dst"]), int(j["src"]), int(j["len"]))
            else:
                ctypes.memset(int(j["dst"]), 0, int(j["len"]))
        return 0


def _engine(**attrs):
    eng = Engine.__new__(Engine)
    eng.lib = FakeLib()
    eng.device = 0
    eng._ctx = 1
    eng.host_empty = lambda nbytes: np.empty(int(nbytes), dtype=np.uint8)
    for name, value in attrs.items():
        setattr(eng, name, value)
    return eng


@pytest.fixture(scope="module")
def encoded():
    """Per shape (chunk, every block of it by the oracle); computed once, never changed."""
    rng = np.random.default_rng(20260)
    out = []
    for k, m, n in SHAPES:
        chunk = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out.append((chunk, _oracle_encode(chunk, k, m)))
    return out


def _km():
    return [(k, m) for k, m, _ in SHAPES]


def _want_digests(encoded):
    return [[hashlib.sha1(b).digest() for b in blocks] for _, blocks in encoded]


def test_padded_encode_is_easy_encode(encoded):
    for (k, m, n), (chunk, blocks) in zip(SHAPES[:3], encoded):
        assert _padded_encode(chunk, k, m) == cfec.easy_encode(chunk, k, m) == blocks


def test_encode_host(encoded):
    eng = _engine()
    parity = eng.encode_host([c for c, _ in encoded], _km())
    assert parity == [blocks[k:] for (k, _, _), (_, blocks) in zip(SHAPES, encoded)]
    assert all(type(b) is bytes for row in parity for b in row)
    assert [c[0] for c in eng.lib.calls] == ["sec_encode_batch"]
    assert eng.lib.calls[0][1:] == (len(SHAPES), SEC_F_HOST)


def test_encode_host_digests(encoded):
    eng = _engine()
    parity, digs = eng.encode_host([c for c, _ in encoded], _km(), digests=True)
    assert parity == [blocks[k:] for (k, _, _), (_, blocks) in zip(SHAPES, encoded)]
    assert digs == _want_digests(encoded)
    assert eng.lib.calls == [("sec_encode_digest_batch", len(SHAPES), SEC_F_HOST)]


def test_encode_host_accepts_arrays_and_views(encoded):
    eng = _engine()
    chunks = [np.frombuffer(c, dtype=np.uint8) if i % 2 else memoryview(c) for i, (c, _) in enumerate(encoded)]
    assert eng.encode_host(chunks, _km()) == [blocks[k:] for (k, _, _), (_, blocks) in zip(SHAPES, encoded)]


@pytest.mark.parametrize("staged", [False, True])
def test_encode_host_raw(encoded, staged):
    eng = _engine()
    buf, layout = eng.encode_host_raw([c for c, _ in encoded], _km(), staged=staged)
    assert len(layout) == len(SHAPES)
    at = 0
    for (k, m, n), (_, blocks), (off, B, p) in zip(SHAPES, encoded, layout):
        assert (off, B, p) == (at, len(blocks[0]), m - k)  # back to back
        assert [buf[off + r * B:off + (r + 1) * B].tobytes() for r in range(p)] == blocks[k:]
        at += p * B
    assert eng.lib.calls == [("sec_encode_batch", len(SHAPES), SEC_F_HOST | (SEC_F_STAGED if staged else 0))]


def test_encode_host_raw_digests(encoded):
    eng = _engine()
    buf, layout, dig = eng.encode_host_raw([c for c, _ in encoded], _km(), digests=True)
    for (k, m, n), (_, blocks), (off, B, p) in zip(SHAPES, encoded, layout):
        assert [buf[off + r * B:off + (r + 1) * B].tobytes() for r in range(p)] == blocks[k:]
    want = b"".join(d for row in _want_digests(encoded) for d in row)
    assert dig[:len(want)].tobytes() == want
    assert eng.lib.calls == [("sec_encode_digest_batch", len(SHAPES), SEC_F_HOST)]


def test_encode_host_of_nothing():
    eng = _engine()
    assert eng.encode_host([], []) == []
    assert eng.encode_host([], [], digests=True) == ([], [])
    buf, layout = eng.encode_host_raw([], [])
    assert layout == []


def _survivors(k, m, blocks, lost, rng):
    """k (block, sharenum) pairs in shuffled order: every primary not in `lost`, and as many
    parity blocks as primaries were lost."""
    nums = [j for j in range(k) if j not in lost] + list(range(k, m))[:len(lost)]
    order = rng.permutation(len(nums))
    return [blocks[nums[i]] for i in order], [nums[i] for i in order]


def _decode_items(encoded, case):
    """(items, the oracle's bytes per item) for one loss pattern over every shape, plus one item
    whose padlen exceeds B (k = 4, B = 5, padlen = 7: the last row is dropped whole)."""
    rng = np.random.default_rng(7 + len(case))
    items, want = [], []
    for (k, m, n), (chunk, blocks) in zip(SHAPES, encoded):
        e = {"none": 0, "last": min(1, m - k), "most": min(m - k, k)}[case]
        lost = [k - 1] if case == "last" and e else list(rng.permutation(k)[:e])
        held, nums = _survivors(k, m, blocks, [int(x) for x in lost], rng)
        padlen = k * len(blocks[0]) - n
        items.append((k, m, held, nums, padlen))
        want.append(cfec.easy_decode(held, nums, padlen, k, m) if blocks[0] else b"")
        assert want[-1] == chunk
    wide = rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
    blocks = cfec.easy_encode(wide, 4, 6)
    lost = {"none": [], "last": [3], "most": [1, 2]}[case]
    held, nums = _survivors(4, 6, blocks, lost, rng)
    items.append((4, 6, held, nums, 7))
    want.append(cfec.easy_decode(held, nums, 7, 4, 6))
    assert want[-1] == wide[:13]
    return items, want


CASES = ["none", "last", "most"]


@pytest.mark.parametrize("library_join", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_decode_host(encoded, case, library_join):
    eng = _engine(LIBRARY_JOIN=library_join)
    items, want = _decode_items(encoded, case)
    got = eng.decode_host(items)
    assert type(got) is bytes and got == b"".join(want)
    flags = {c[2] for c in eng.lib.calls if c[0] == "sec_decode_batch_ex"}
    if library_join:
        assert flags == {SEC_F_HOST}
    else:  # the GPU is asked only when a primary is missing, and only for the missing rows
        assert flags == (set() if case == "none" else {SEC_F_HOST | SEC_F_RECOVER})
    assert len([c for c in eng.lib.calls if c[0] == "sec_decode_batch_ex"]) <= 1


@pytest.mark.parametrize("library_join", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_decode_host_into(encoded, case, library_join):
    eng = _engine(LIBRARY_JOIN=library_join)
    items, want = _decode_items(encoded, case)
    flat = b"".join(want)
    dst = np.full(len(flat) + 3, 0xA5, dtype=np.uint8)
    assert eng.decode_host_into(items, dst) == len(flat)
    assert dst[:len(flat)].tobytes() == flat
    assert dst[len(flat):].tobytes() == b"\xa5" * 3  # nothing past the result is written
    short = np.zeros(len(flat) - 1, dtype=np.uint8)
    with pytest.raises(ValueError):
        eng.decode_host_into(items, short)


@pytest.mark.parametrize("library_join", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_decode_host_chunks(encoded, case, library_join):
    eng = _engine(LIBRARY_JOIN=library_join)
    items, want = _decode_items(encoded, case)
    got = eng.decode_host_chunks(items)
    assert got == want
    assert all(type(b) is bytes for b in got)
    assert len([c for c in eng.lib.calls if c[0] == "sec_decode_batch_ex"]) <= 1


@pytest.mark.parametrize("method", ["decode_host", "decode_host_chunks"])
def test_decode_join_on_the_copy_threads(encoded, method):
    eng = _engine(LIBRARY_JOIN=False, NATIVE_JOIN_MIN=1)
    items, want = _decode_items(encoded, "most")
    got = getattr(eng, method)(items)
    assert got == (b"".join(want) if method == "decode_host" else want)
    assert any(c[0] == "sec_host_copy" for c in eng.lib.calls)


def test_decode_host_of_nothing():
    for library_join in (True, False):
        eng = _engine(LIBRARY_JOIN=library_join)
        assert eng.decode_host([]) == b""
        assert eng.decode_host_chunks([]) == []
        assert eng.decode_host_into([], np.zeros(4, dtype=np.uint8)) == 0
