"""CPU: the tagged encode's bindings and its Python assembly (piece.encode_chunks_with_tags and the
stream form) with tests/engine_stub.py's oracle engine in place of the HIP context.

The stub's sec_encode_pieces_tags stand-in fills the tag slots from oracle.apdp_ref.tag_value
over the oracle's pieces, and a stand-in challenge system provides the two methods piece.py
calls (tag_key, wrap_tags), so the slot numbering, the APDPTag fields, the ids and the stream's
tuples are checked with no GPU.  The one-shot form runs on an EngineGroup worker whose engine is
the stub (as tests/test_group.py installs it); the stream form runs its windows on the module's
own stream workers, so there piece.get_engine is replaced.  The GPU twin is
tests/test_gpu_encode_tags.py."""

import ctypes
import random

import numpy as np
import pytest

from oracle import apdp_ref, cfec
from storb_amd import _lib, piece
from storb_amd.apdp import APDPTag
from storb_amd.engine import EngineGroup
from tests.engine_stub import OracleHostEngine

PRF_KEY = b"k" * 44


class StandInSystem:
    """What piece.py needs of apdp.ChallengeSystem: tag_key() and wrap_tags(values)."""

    def __init__(self, key):
        self.n, self.e, self.d, self.p, self.q = key
        self.g = pow(123456789, 2, self.n)
        self.prf_key = PRF_KEY
        self.key_calls = 0
        self._memo = {}  # the stub engine and the checks ask for the same pieces' tags

    def tag_key(self):
        self.key_calls += 1
        return self

    def wrap_tags(self, values):
        pv = apdp_ref.prf(self.prf_key, 0)
        return [APDPTag(index=0, tag_value=v, prf_value=pv) for v in values]

    def want(self, data: bytes) -> int:
        if data not in self._memo:
            self._memo[data] = apdp_ref.tag_value(self.n, self.g, self.d, self.prf_key, data)
        return self._memo[data]


class TagOracleEngine(OracleHostEngine):
    """OracleHostEngine whose encode_pieces_into also fills `tags` (256 bytes big-endian per piece
    slot) from the oracle: sec_encode_pieces_tags' contract on the CPU."""

    def encode_pieces_into(self, chunks, shapes, piece_addrs, digests=None, staged=False, gpu_parity_ids=False,
                           tags=None, tag_key=None):
        super().encode_pieces_into(chunks, shapes, piece_addrs, digests, staged, gpu_parity_ids)
        assert (tags is None) == (tag_key is None)
        if tags is None:
            return
        j = 0
        for c, (k, m) in zip(chunks, shapes):
            for b in cfec.easy_encode(bytes(c), k, m):
                tags[256 * j:256 * (j + 1)] = np.frombuffer(tag_key.want(b).to_bytes(256, "big"), np.uint8)
                j += 1


@pytest.fixture(scope="module")
def system():
    return StandInSystem(apdp_ref.test_key(11))


@pytest.fixture
def worker():
    g = EngineGroup([0], engine_factory=TagOracleEngine)
    yield g
    g.close()


def _chunks(seed):
    # storb's shapes: k = 1 (m = 2), k = 2 (m = 3) between them, k = 4 (m = 6), one with padding
    rng = random.Random(seed)
    return [rng.randbytes(n) for n in (1000, 40_000, 200_001, 3000, (1 << 20) + 3, 17)]


def test_symbols_bound():
    lib = _lib.load()
    for name in ("sec_encode_tag_batch", "sec_encode_pieces_tags"):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9


def test_null_ctx_is_einval():
    lib = _lib.load()
    one = ctypes.c_void_p(1)  # never read: the NULL context is refused first
    assert lib.sec_encode_tag_batch(None, one, one, 1, one, one, one, one, 0) == _lib.SEC_EINVAL
    assert lib.sec_encode_pieces_tags(None, one, one, 1, one, one, one, one, _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert lib.sec_encode_pieces_tags(None, None, one, 1, one, one, one, None, _lib.SEC_F_HOST) == _lib.SEC_EINVAL


def _check(chunks, first, out, ids, tags, system, with_ids=True):
    assert [ec.chunk_idx for ec in out] == list(range(first, first + len(chunks)))
    assert len(tags) == len(chunks)
    ks = set()
    pv = apdp_ref.prf(PRF_KEY, 0)
    for i, (c, ec) in enumerate(zip(chunks, out)):
        k, m, B, padlen = piece.chunk_shape(len(c))
        ks.add(k)
        want = cfec.easy_encode(c, k, m)
        assert (ec.k, ec.m, ec.chunk_size, ec.padlen, ec.original_chunk_size) == (k, m, B, padlen, len(c))
        assert [p.data for p in ec.pieces] == want
        assert len(tags[i]) == m
        for j, (w, t) in enumerate(zip(want, tags[i])):
            assert isinstance(t, APDPTag)
            assert (t.index, t.prf_value) == (0, pv)
            assert t.tag_value == system.want(w), (i, j)  # chunk i's slot j, whatever its neighbours' m
        if with_ids:
            assert ids[i] == [piece.piece_hash(w) for w in want]
    return ks


def test_with_tags_slots_fields_and_ids(worker, system):
    chunks = _chunks(1)
    out, ids, tags = worker.submit(0, piece.encode_chunks_with_tags, chunks, system, 5).result()
    ks = _check(chunks, 5, out, ids, tags, system)
    assert len(ks) >= 3  # a chunk's k differs from its neighbours'
    assert worker.engines[0].chunks_encoded == len(chunks)  # one call: no second pass for the tags


def test_with_tags_no_ids(worker, system):
    chunks = _chunks(2)[:3]
    out, ids, tags = worker.submit(0, lambda: piece.encode_chunks_with_tags(chunks, system, piece_ids=False)).result()
    assert ids is None
    _check(chunks, 0, out, None, tags, system, with_ids=False)


def test_with_tags_errors_as_encode_chunks(worker, system):
    with pytest.raises(ValueError):  # an empty chunk: piece_length's error, before any work
        worker.submit(0, piece.encode_chunks_with_tags, [b"abc", b""], system).result()
    assert worker.engines[0].chunks_encoded == 0
    assert worker.submit(0, piece.encode_chunks_with_tags, [], system).result() == ([], [], [])


def test_with_tags_short_middle_slice(worker, system, monkeypatch):
    # easyfec's short middle slice cannot come from chunk_shape's own B; force a shape that has it
    monkeypatch.setattr(piece, "chunk_shape", lambda n: (4, 6, 10, 40 - n))
    with pytest.raises(piece.Error, match="same length"):
        worker.submit(0, piece.encode_chunks_with_tags, [b"x" * 25], system).result()
    with pytest.raises(piece.Error, match="same length"):
        worker.submit(0, lambda: piece.encode_chunks([b"x" * 25], devices=piece._ONE)).result()


def test_stream_tuples(system, monkeypatch):
    eng = TagOracleEngine()
    monkeypatch.setattr(piece, "get_engine", lambda *a: eng)
    chunks = _chunks(3)
    before = system.key_calls
    outs = list(piece.encode_chunks_stream(iter(chunks), 2, piece_ids=True, window_bytes=250_000, tags=system))
    assert all(len(o) == 3 for o in outs)
    _check(chunks, 2, [o[0] for o in outs], [o[1] for o in outs], [o[2] for o in outs], system)
    assert system.key_calls - before >= 3  # several windows, each asking its worker thread's key
    outs = list(piece.encode_chunks_stream(chunks[:2], tags=system))
    assert [o[1] for o in outs] == [None, None]
    _check(chunks[:2], 0, [o[0] for o in outs], None, [o[2] for o in outs], system, with_ids=False)


def test_stream_error_after_the_chunks_before_it(system, monkeypatch):
    eng = TagOracleEngine()
    monkeypatch.setattr(piece, "get_engine", lambda *a: eng)
    chunks = _chunks(4)[:2] + [b""]
    got = []
    with pytest.raises(ValueError):
        for o in piece.encode_chunks_stream(chunks, tags=system):
            got.append(o)
    assert len(got) == 2


def test_stream_tags_with_devices_is_value_error(worker, system):
    with pytest.raises(ValueError, match="devices"):
        piece.encode_chunks_stream([b"abc"], tags=system, devices=worker)


def test_with_ids_unchanged(worker, system):
    chunks = _chunks(5)
    out, ids = worker.submit(0, piece.encode_chunks_with_ids, chunks, 1).result()
    assert [ec.chunk_idx for ec in out] == list(range(1, 1 + len(chunks)))
    for c, ec, hs in zip(chunks, out, ids):
        k, m, _, _ = piece.chunk_shape(len(c))
        want = cfec.easy_encode(c, k, m)
        assert [p.data for p in ec.pieces] == want
        assert hs == [piece.piece_hash(w) for w in want]
    # ... and the tagged call gives the same chunks and ids
    out2, ids2, _ = worker.submit(0, piece.encode_chunks_with_tags, chunks, system, 1).result()
    assert ids2 == ids
    assert [[p.data for p in ec.pieces] for ec in out2] == [[p.data for p in ec.pieces] for ec in out]
