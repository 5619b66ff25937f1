"""CPU: piece.decode_chunks_checked / reconstruct_data_checked, the host logic above
Engine.decode_check_host: which pieces are decoded from and which checked, the locate and re-check
rounds shared with check_chunks, the second decode of located chunks and the splice.  The engine
is a stub whose calls ARE the oracle (cfec.easy_decode / easy_encode, a numpy compare), so no GPU
is needed; the GPU path below it is tests/test_gpu_decode_check.py's.  Corruptions are applied
here, and every expectation is where the test put them."""

import random

import numpy as np
import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import check_check_item, check_decode_check_item, check_decode_item, choose_blocks


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


class OracleEngine:
    """Engine.decode_check_host, check_host and decode_host on the oracle; records its calls."""

    def __init__(self):
        self.calls = []

    def decode_check_host(self, items):
        self.calls.append(("decode_check", items))
        data, checks = b"", []
        for k, m, blocks, sharenums, padlen in items:
            check_decode_check_item(k, m, blocks, sharenums, padlen)
            data += cfec.easy_decode([bytes(b) for b in blocks[:k]], list(sharenums[:k]), padlen, k, m)
            checks.append(_oracle_check(k, m, blocks, sharenums))
        return data, checks

    def check_host(self, items):
        self.calls.append(("check", items))
        for it in items:
            check_check_item(*it)
        return [_oracle_check(*it) for it in items]

    def decode_host(self, items):
        self.calls.append(("decode", items))
        for it in items:
            check_decode_item(*it)
        return b"".join(cfec.easy_decode([bytes(b) for b in blocks], list(sn), padlen, k, m)
                        for k, m, blocks, sn, padlen in items)


@pytest.fixture
def stub(monkeypatch):
    eng = OracleEngine()
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


def _corrupt(ec, piece_idx, offset, value=0x40):
    for p in ec.pieces:
        if p.piece_idx == piece_idx:
            b = bytearray(p.data)
            b[offset] ^= value
            p.data = bytes(b)
            return ec
    raise AssertionError("piece not held")


def _drop(ec, lost):
    ec.pieces = [p for p in ec.pieces if p.piece_idx not in lost]
    return ec


def test_clean_chunks_return_the_data_and_are_consistent(stub):
    (a, da), (b, db), (c, dc) = _chunk(4, 6, 4 * 50 - 3, 0, 1), _chunk(10, 14, 10 * 17 - 9, 1, 2), _chunk(4, 8, 160, 2, 3)
    _drop(b, {3, 11})  # a data piece lost: recovered, and two check rows left
    random.Random(5).shuffle(c.pieces)
    c.pieces.append(c.pieces[0])  # held twice: used once
    data, checks = piece.decode_chunks_checked([a, b, c])
    assert data == da + db + dc
    assert checks == [piece.ChunkCheck(chunk_idx=0, checked=6, consistent=True),
                      piece.ChunkCheck(chunk_idx=1, checked=12, consistent=True),
                      piece.ChunkCheck(chunk_idx=2, checked=8, consistent=True)]
    ((kind, items),) = stub.calls  # ONE fused call, nothing else
    assert kind == "decode_check" and [len(it[2]) for it in items] == [6, 12, 8]
    # every distinct held piece is used: choose_blocks' pick first (decoded from), then the rest
    have = [s for s in range(14) if s not in (3, 11)]
    basis = [have[j] for j in choose_blocks(10, 14, have)]
    assert items[1][3] == basis + [s for s in have if s not in basis]
    assert items[2][3] == list(range(8)) and [it[4] for it in items] == [a.padlen, b.padlen, c.padlen]


def test_one_corrupt_piece_with_two_spares_is_located_and_the_bytes_are_correct(stub):
    (a, da), (b, db), (c, dc) = _chunk(4, 6, 4 * 64 - 1, 0, 4), _chunk(10, 14, 10 * 17 - 9, 1, 5), _chunk(4, 6, 80, 2, 6)
    _corrupt(a, 1, 17)   # a data piece: it is decoded from, so the first pass returns wrong bytes
    _corrupt(b, 12, 3)   # a parity piece held as a check row: the first pass's bytes are right
    data, checks = piece.decode_chunks_checked([a, b, c])
    assert [(g.chunk_idx, g.checked, g.consistent, g.first_bad_offset, g.bad_piece_idx, g.located) for g in checks] == [
        (0, 6, False, 17, [1], True), (1, 14, False, 3, [12], True), (2, 6, True, None, [], False)]
    assert data == da + db + dc
    kinds = [k for k, _ in stub.calls]
    assert kinds == ["decode_check", "check", "decode"]  # the fused pass, ONE batched re-check, ONE second decode
    assert [it[3] for it in stub.calls[1][1]] == [[0, 2, 3, 4, 5], [s for s in range(14) if s != 12]]
    again = stub.calls[2][1]
    assert [sorted(it[3]) for it in again] == [[0, 2, 3, 4], list(range(10))]  # from pieces that passed the re-check
    assert [it[4] for it in again] == [a.padlen, b.padlen]
    # without locate the check is reported and the first pass's bytes returned as they are
    stub.calls.clear()
    data2, checks2 = piece.decode_chunks_checked([a, b, c], locate=False)
    assert [(g.consistent, g.first_bad_offset, g.bad_piece_idx, g.located) for g in checks2] == [
        (False, 17, [], False), (False, 3, [], False), (True, None, [], False)]
    assert data2 != da + db + dc and data2[len(da):] == db + dc and len(stub.calls) == 1


def test_located_chunk_in_the_middle_is_spliced(stub):
    (a, da), (b, db), (c, dc) = _chunk(4, 6, 61, 0, 7), _chunk(4, 8, 4 * 40 - 2, 1, 8), _chunk(4, 6, 97, 2, 9)
    _corrupt(_corrupt(b, 2, 30), 6, 9)  # two corrupt pieces at different offsets: two rounds
    data, checks = piece.decode_chunks_checked([a, b, c])
    assert data == da + db + dc
    assert checks[1].bad_piece_idx == [6, 2] and checks[1].located and not checks[1].consistent
    assert [k for k, _ in stub.calls] == ["decode_check", "check", "check", "decode"]


def test_one_spare_only_cannot_be_trusted(stub):
    ec, data = _chunk(4, 6, 4 * 40, 9, 10)
    _corrupt(_drop(ec, {5}), 0, 2)
    got, checks = piece.decode_chunks_checked([ec])
    assert (checks[0].checked, checks[0].consistent, checks[0].first_bad_offset, checks[0].located) == (5, False, 2, False)
    assert got != data and len(got) == len(data)
    clean, dclean = _chunk(4, 6, 33, 3, 11)
    with pytest.raises(piece.PieceCheckError) as e:
        piece.reconstruct_data_checked(ec.pieces + clean.pieces, [clean, ec])
    assert isinstance(e.value, ValueError)
    assert [(c.chunk_idx, c.consistent or c.located) for c in e.value.checks] == [(3, True), (9, False)]


def test_reconstruct_data_checked(stub):
    (a, da), (b, db) = _chunk(4, 6, 4 * 64 - 1, 0, 12), _chunk(10, 14, 10 * 17 - 9, 1, 13)
    pieces = a.pieces + b.pieces
    random.Random(3).shuffle(pieces)
    a.pieces, b.pieces = [], []
    data, checks = piece.reconstruct_data_checked(pieces, [a, b])
    assert data == da + db and all(c.consistent for c in checks)
    # a located chunk is returned corrected, no error
    for p in pieces:
        if (p.chunk_idx, p.piece_idx) == (1, 4):
            p.data = bytes(x ^ 0xFF if i == 5 else x for i, x in enumerate(p.data))
    data, checks = piece.reconstruct_data_checked(pieces, [a, b])
    assert data == da + db and checks[1].located and checks[1].bad_piece_idx == [4]


def test_fewer_than_k_pieces(stub):
    ec, _ = _chunk(4, 6, 40, 9, 14)
    _drop(ec, {0, 1, 5})
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 9"):
        piece.reconstruct_data_checked(ec.pieces, [ec])
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 9"):
        piece.decode_chunks_checked([ec])
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 9"):  # reconstruct_data's own text
        piece.reconstruct_data(ec.pieces, [ec])
    assert stub.calls == []
    assert piece.decode_chunks_checked([]) == (b"", [])


def test_check_chunks_is_unchanged_on_the_same_inputs(stub):
    """The rounds are shared: check_chunks reports what decode_chunks_checked reports, from plain
    check calls only."""
    def inputs():
        (a, _), (b, _), (c, _), (d, _) = (_chunk(4, 6, 4 * 64, 0, 4), _chunk(10, 14, 10 * 17 - 9, 1, 5),
                                          _chunk(4, 6, 80, 2, 6), _chunk(4, 8, 160, 3, 7))
        _corrupt(a, 1, 17)
        _corrupt(b, 12, 3)
        _corrupt(_corrupt(d, 2, 30, 0x11), 6, 30, 0xE0)  # same offset: not located
        return [a, b, c, d]
    want = [(0, 6, False, 17, [1], True), (1, 14, False, 3, [12], True), (2, 6, True, None, [], False),
            (3, 8, False, 30, [], False)]
    got = piece.check_chunks(inputs())
    assert [(g.chunk_idx, g.checked, g.consistent, g.first_bad_offset, g.bad_piece_idx, g.located) for g in got] == want
    assert [k for k, _ in stub.calls] == ["check", "check"] and [len(c[1]) for c in stub.calls] == [4, 2]
    stub.calls.clear()
    _, checks = piece.decode_chunks_checked(inputs())
    assert checks == got
