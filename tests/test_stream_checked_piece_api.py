"""CPU: piece.reconstruct_data_stream_checked, the streamed form of reconstruct_data_checked: the
windows, their order, what each window costs, where the errors arrive and what an early close
leaves behind.  The engine is a stub whose calls ARE the oracle (cfec.easy_decode / easy_encode, a
numpy compare), a class of this file's own, so no GPU is needed; the GPU path below it is
tests/test_gpu_check_bs.py's.  Corruptions are applied here, and every expectation is where the
test put them."""

import random
import threading

import numpy as np
import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import check_check_item, check_decode_check_item, check_decode_item


def _oracle_check(k, m, blocks, sharenums):
    data = cfec.easy_decode([bytes(b) for b in blocks[:k]], list(sharenums[:k]), 0, k, m)
    full = cfec.easy_encode(data, k, m)
    bad, first = [], None
    for q in range(k, len(blocks)):
        d = np.flatnonzero(np.frombuffer(full[sharenums[q]], np.uint8) != np.frombuffer(blocks[q], np.uint8))
        if d.size:
            bad.append(q)
            first = int(d[0]) if first is None else min(first, int(d[0]))
    return (None, [], None) if first is None else (first, bad, bytes(b[first] for b in blocks))


class StreamOracleEngine:
    """Engine.decode_check_host, check_host and decode_host on the oracle.  Records its calls (the
    stream worker makes them, so under a lock) and how many are running at any moment."""

    def __init__(self):
        self.calls = []
        self.lock = threading.Lock()
        self.running = 0

    def _enter(self, kind, items):
        with self.lock:
            self.calls.append((kind, items))
            self.running += 1

    def _leave(self):
        with self.lock:
            self.running -= 1

    def decode_check_host(self, items):
        self._enter("decode_check", items)
        try:
            data, checks = b"", []
            for k, m, blocks, sharenums, padlen in items:
                check_decode_check_item(k, m, blocks, sharenums, padlen)
                data += cfec.easy_decode([bytes(b) for b in blocks[:k]], list(sharenums[:k]), padlen, k, m)
                checks.append(_oracle_check(k, m, blocks, sharenums))
            return data, checks
        finally:
            self._leave()

    def check_host(self, items):
        self._enter("check", items)
        try:
            for it in items:
                check_check_item(*it)
            return [_oracle_check(*it) for it in items]
        finally:
            self._leave()

    def decode_host(self, items):
        self._enter("decode", items)
        try:
            for it in items:
                check_decode_item(*it)
            return b"".join(cfec.easy_decode([bytes(b) for b in blocks], list(sn), padlen, k, m)
                            for k, m, blocks, sn, padlen in items)
        finally:
            self._leave()


@pytest.fixture
def stub(monkeypatch):
    eng = StreamOracleEngine()
    monkeypatch.setattr(piece, "get_engine", lambda device=None: eng)
    return eng


def _chunk(k, m, n, chunk_idx, seed):
    data = bytes(random.Random(seed).randrange(256) for _ in range(n))
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    pieces = [piece.Piece(chunk_idx=chunk_idx, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks)]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=k * B - n,
                            original_chunk_size=n)
    return ec, data


def _corrupt(pieces, chunk_idx, piece_idx, offset, value=0x40):
    for p in pieces:
        if (p.chunk_idx, p.piece_idx) == (chunk_idx, piece_idx):
            b = bytearray(p.data)
            b[offset] ^= value
            p.data = bytes(b)
            return
    raise AssertionError("piece not held")


SHAPES = [(4, 6, 4 * 50 - 3), (10, 14, 10 * 17 - 9), (4, 8, 160), (8, 11, 8 * 30 - 5), (4, 6, 97), (16, 24, 16 * 9 - 1)]


def _object(seed=0):
    """Six chunks of mixed shapes: (chunks with their pieces taken out, all pieces shuffled, the data)."""
    made = [_chunk(k, m, n, i, seed + i) for i, (k, m, n) in enumerate(SHAPES)]
    pieces = [p for ec, _ in made for p in ec.pieces]
    random.Random(seed).shuffle(pieces)
    chunks = [ec for ec, _ in made]
    for ec in chunks:
        ec.pieces = []
    return chunks, pieces, [d for _, d in made]


def _fresh(chunks):
    for ec in chunks:
        ec.pieces = []
    return chunks


def _kinds(stub):
    return [k for k, _ in stub.calls]


@pytest.mark.parametrize("window_bytes,nwin", [(1, 6), (400, 3), (1 << 20, 1)])
def test_pairs_match_reconstruct_data_checked(stub, window_bytes, nwin):
    """One, some and all chunks per window (chunk sizes 197, 161, 160, 235, 97, 143: windows of 400
    bytes hold [197, 161], [160, 235], [97, 143])."""
    chunks, pieces, datas = _object(1)
    _corrupt(pieces, 1, 12, 3)   # a parity piece: located
    _corrupt(pieces, 3, 2, 11)   # a data piece: located, decoded again
    want_data, want_checks = piece.reconstruct_data_checked(pieces, _fresh(chunks))
    assert want_data == b"".join(datas)
    stub.calls.clear()
    got = list(piece.reconstruct_data_stream_checked(pieces, _fresh(chunks), window_bytes=window_bytes))
    assert [d for d, _ in got] == datas
    assert [c for _, c in got] == want_checks
    assert [(c.chunk_idx, c.consistent, c.located, c.bad_piece_idx) for _, c in got] == [
        (0, True, False, []), (1, False, True, [12]), (2, True, False, []), (3, False, True, [2]),
        (4, True, False, []), (5, True, False, [])]
    assert _kinds(stub).count("decode_check") == nwin


def test_each_window_costs_one_fused_call_plus_its_own_rounds(stub):
    chunks, pieces, datas = _object(2)
    _corrupt(pieces, 3, 9, 5)    # window 1 (chunks 2, 3), a parity piece
    win = 400  # two chunks per window: [0, 1], [2, 3], [4, 5] (358, 395 and 240 bytes)
    got = list(piece.reconstruct_data_stream_checked(pieces, chunks, window_bytes=win))
    assert [d for d, _ in got] == datas
    # in window order (one worker): clean windows are ONE call; the corrupt one adds one re-check
    # of its one inconsistent chunk and one second decode of it
    assert _kinds(stub) == ["decode_check", "decode_check", "check", "decode", "decode_check"]
    assert [len(it) for k, it in stub.calls] == [2, 2, 1, 1, 2]
    assert [[len(c[2]) for c in it] for k, it in stub.calls if k == "decode_check"] == [[6, 14], [8, 11], [6, 24]]
    assert got[3][1].located and got[3][1].bad_piece_idx == [9] and got[3][1].first_bad_offset == 5


def test_located_chunk_in_the_middle_of_a_window_is_yielded_corrected_in_order(stub):
    chunks, pieces, datas = _object(3)
    _corrupt(pieces, 1, 4, 7)  # a data piece of the middle chunk of window [0, 1, 2]
    win = sum(n for _, _, n in SHAPES[:3])
    got = list(piece.reconstruct_data_stream_checked(pieces, chunks, window_bytes=win))
    assert [c.chunk_idx for _, c in got] == list(range(6))
    assert [d for d, _ in got] == datas
    assert (got[1][1].consistent, got[1][1].located, got[1][1].bad_piece_idx, got[1][1].first_bad_offset) == (
        False, True, [4], 7)


def test_unlocatable_chunk_raises_after_every_earlier_chunk(stub):
    chunks, pieces, datas = _object(4)
    # chunk 4 is (4, 6): two pieces corrupt at the same offset cannot be told apart
    _corrupt(pieces, 4, 1, 20, 0x11)
    _corrupt(pieces, 4, 5, 20, 0xE0)
    win = SHAPES[0][2] + SHAPES[1][2]
    stream = piece.reconstruct_data_stream_checked(pieces, chunks, window_bytes=win)
    got = []
    with pytest.raises(piece.PieceCheckError) as e:
        for pair in stream:
            got.append(pair)
    assert [d for d, _ in got] == datas[:4]
    assert [(c.chunk_idx, c.consistent or c.located) for c in e.value.checks] == [
        (0, True), (1, True), (2, True), (3, True), (4, False)]
    assert e.value.checks[:4] == [c for _, c in got]
    assert "chunk 4" in str(e.value)


def test_too_few_pieces_raises_after_every_earlier_chunk(stub):
    chunks, pieces, datas = _object(5)
    pieces = [p for p in pieces if not (p.chunk_idx == 3 and p.piece_idx < 4)]  # (8, 11): 7 left
    win = 400  # chunk 3 is the second chunk of window [2, 3]: chunk 2 is still decoded and yielded
    got = []
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 3") as e:
        for pair in piece.reconstruct_data_stream_checked(pieces, chunks, window_bytes=win):
            got.append(pair)
    assert not isinstance(e.value, piece.PieceCheckError)
    assert [d for d, _ in got] == datas[:3] and all(c.consistent for _, c in got)


def test_closing_after_the_first_chunk_leaves_no_window_running(stub):
    chunks, pieces, datas = _object(6)
    stream = piece.reconstruct_data_stream_checked(pieces, chunks, window_bytes=1)  # six windows
    first = next(stream)
    assert first[0] == datas[0]
    stream.close()
    # the windows already handed to the worker (the pipeline keeps two in flight) finish or are
    # cancelled; after the worker drains, nothing runs and no further window was started
    def drain():  # every stream worker is single-threaded: a no-op queued behind its work
        for i in range(piece.STREAM_WORKERS):
            piece._pool(f"stream{i}").submit(lambda: None).result()

    drain()
    assert stub.running == 0
    started = _kinds(stub).count("decode_check")
    assert 1 <= started <= 2  # the pipeline keeps two windows in flight; the other four never start
    drain()
    assert _kinds(stub).count("decode_check") == started


def test_empty_object_yields_nothing(stub):
    assert list(piece.reconstruct_data_stream_checked([], [])) == []
    assert stub.calls == []
