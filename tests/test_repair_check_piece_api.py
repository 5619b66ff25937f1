"""CPU: piece.repair_chunks_checked / repair_pieces_checked, the host logic above
Engine.repair_check_host: which pieces are repaired from and which checked, the default targets,
the locate and re-check rounds shared with check_chunks, and the second repair of located chunks,
which also regenerates the pieces named corrupt.  The engine is a stub whose calls ARE the oracle
(cfec.easy_decode / easy_encode, a numpy compare), so no GPU is needed; the GPU path below it is
tests/test_gpu_repair_check.py's.  Corruptions are applied here, and every expectation is where the
test put them."""

import hashlib
import random

import numpy as np
import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import check_check_item, check_repair_check_item, check_repair_item, choose_blocks


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


def _oracle_repair(k, m, blocks, sharenums, targets):
    """The targets of the code word that the first k blocks AS HELD span, and their SHA-1."""
    data = cfec.easy_decode([bytes(b) for b in blocks[:k]], list(sharenums[:k]), 0, k, m)
    full = cfec.easy_encode(data, k, m)
    return [full[t] for t in targets], [hashlib.sha1(full[t]).digest() for t in targets]


class OracleEngine:
    """Engine.repair_check_host, check_host and repair_host on the oracle; records its calls."""

    def __init__(self):
        self.calls = []

    def repair_check_host(self, items, digests=False):
        self.calls.append(("repair_check", items))
        out, digs, checks = [], [], []
        for k, m, blocks, sharenums, targets in items:
            check_repair_check_item(k, m, blocks, sharenums, targets)
            o, d = _oracle_repair(k, m, blocks, sharenums, targets)
            out.append(o)
            digs.append(d)
            checks.append(_oracle_check(k, m, blocks, sharenums))
        return (out, digs, checks) if digests else (out, checks)

    def check_host(self, items):
        self.calls.append(("check", items))
        for it in items:
            check_check_item(*it)
        return [_oracle_check(*it) for it in items]

    def repair_host(self, items, digests=False):
        self.calls.append(("repair", items))
        out, digs = [], []
        for k, m, blocks, sharenums, targets in items:
            check_repair_item(k, m, blocks, sharenums, targets)
            o, d = _oracle_repair(k, m, blocks, sharenums, targets)
            out.append(o)
            digs.append(d)
        return (out, digs) if digests else out


@pytest.fixture
def stub(monkeypatch):
    eng = OracleEngine()
    monkeypatch.setattr(piece, "get_engine", lambda device=None: eng)
    return eng


def _chunk(k, m, n, chunk_idx, seed, lost=()):
    data = bytes(random.Random(seed).randrange(256) for _ in range(n))
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    pieces = [piece.Piece(chunk_idx=chunk_idx, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks) if i not in lost]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=k * B - n,
                            original_chunk_size=n)
    return ec, blocks


def _corrupt(ec, piece_idx, offset, value=0x40):
    for p in ec.pieces:
        if p.piece_idx == piece_idx:
            b = bytearray(p.data)
            b[offset] ^= value
            p.data = bytes(b)
            return ec
    raise AssertionError("piece not held")


def test_clean_chunks_are_one_fused_call_and_the_pieces_are_the_oracles(stub):
    (a, ba), (b, bb), (c, bc) = (_chunk(4, 6, 4 * 50 - 3, 0, 1, lost={1}), _chunk(10, 14, 10 * 17 - 9, 1, 2, lost={3, 11}),
                                 _chunk(4, 8, 160, 2, 3, lost={0, 7}))
    random.Random(5).shuffle(c.pieces)
    c.pieces.append(c.pieces[0])  # held twice: used once
    got, checks = piece.repair_chunks_checked([a, b, c], targets=[None, [11, 3], None])
    assert [[(p.piece_idx, p.data) for p in row] for row in got] == [
        [(1, ba[1])], [(11, bb[11]), (3, bb[3])], [(0, bc[0]), (7, bc[7])]]
    assert [[p.piece_type for p in row] for row in got] == [
        [piece.PieceType.Data], [piece.PieceType.Parity, piece.PieceType.Data],
        [piece.PieceType.Data, piece.PieceType.Parity]]
    assert all(type(p) is piece.Piece and p.chunk_idx == i for i, row in enumerate(got) for p in row)
    assert checks == [piece.ChunkCheck(chunk_idx=0, checked=5, consistent=True),
                      piece.ChunkCheck(chunk_idx=1, checked=12, consistent=True),
                      piece.ChunkCheck(chunk_idx=2, checked=6, consistent=True)]
    ((kind, items),) = stub.calls  # ONE fused call, nothing else
    assert kind == "repair_check" and [len(it[2]) for it in items] == [5, 12, 6]
    # every distinct held piece is used: choose_blocks' pick first (repaired from), then the rest
    have = [s for s in range(14) if s not in (3, 11)]
    basis = [have[j] for j in choose_blocks(10, 14, have)]
    assert items[1][3] == basis + [s for s in have if s not in basis]
    assert [it[4] for it in items] == [[1], [11, 3], [0, 7]]


def test_one_corrupt_survivor_with_two_spares_is_located_and_replaced(stub):
    (a, ba), (b, bb), (c, bc) = (_chunk(4, 7, 4 * 64 - 1, 0, 4, lost={1}), _chunk(10, 14, 10 * 17 - 9, 1, 5, lost={0}),
                                 _chunk(4, 6, 80, 2, 6, lost={5}))
    _corrupt(a, 2, 17)   # a data piece: it is repaired from, so the first pass's target is wrong
    _corrupt(b, 12, 3)   # a parity piece held as a check row: the first pass's target is right
    got, checks = piece.repair_chunks_checked([a, b, c], piece_ids=True)
    assert [(g.chunk_idx, g.checked, g.consistent, g.first_bad_offset, g.bad_piece_idx, g.located) for g in checks] == [
        (0, 6, False, 17, [2], True), (1, 13, False, 3, [12], True), (2, 5, True, None, [], False)]
    # the requested targets, then the replacement for the piece named corrupt
    assert [[(p.piece_idx, p.data) for p in row] for row in got] == [
        [(1, ba[1]), (2, ba[2])], [(0, bb[0]), (12, bb[12])], [(5, bc[5])]]
    assert all(type(p) is piece.ProcessedPieceInfo and p.piece_id == hashlib.sha1(p.data).hexdigest()
               for row in got for p in row)
    assert [k for k, _ in stub.calls] == ["repair_check", "check", "repair"]  # ONE re-check, ONE second repair
    assert [it[3] for it in stub.calls[1][1]] == [[0, 3, 4, 5, 6], [s for s in range(1, 14) if s != 12]]
    again = stub.calls[2][1]
    assert [sorted(it[3]) for it in again] == [[0, 3, 4, 5], list(range(1, 11))]  # pieces that passed the re-check
    assert [it[4] for it in again] == [[1, 2], [0, 12]]
    # without locate the check is reported and the first pass's pieces returned as they are
    stub.calls.clear()
    got2, checks2 = piece.repair_chunks_checked([a, b, c], locate=False)
    assert [(g.consistent, g.first_bad_offset, g.bad_piece_idx, g.located) for g in checks2] == [
        (False, 17, [], False), (False, 3, [], False), (True, None, [], False)]
    assert [[p.piece_idx for p in row] for row in got2] == [[1], [0], [5]]
    assert got2[0][0].data != ba[1] and got2[1][0].data == bb[0] and len(stub.calls) == 1


def test_one_spare_only_cannot_be_trusted(stub):
    ec, blocks = _chunk(4, 6, 4 * 40, 9, 10, lost={5})
    _corrupt(ec, 0, 2)
    got, ck = piece.repair_pieces_checked(ec)
    assert (ck.checked, ck.consistent, ck.first_bad_offset, ck.bad_piece_idx, ck.located) == (5, False, 2, [], False)
    # what the first k pieces give, corrupt piece included
    assert [p.piece_idx for p in got] == [5] and got[0].data != blocks[5] and len(got[0].data) == len(blocks[5])
    assert [k for k, _ in stub.calls] == ["repair_check"]


def test_exactly_k_pieces_is_a_plain_repair_reported_consistent(stub):
    ec, blocks = _chunk(4, 6, 4 * 40 - 1, 3, 11, lost={1, 4})
    got, ck = piece.repair_pieces_checked(ec)
    assert [(p.piece_idx, p.data) for p in got] == [(1, blocks[1]), (4, blocks[4])]
    assert ck == piece.ChunkCheck(chunk_idx=3, checked=4, consistent=True)


def test_fewer_than_k_pieces(stub):
    ec, _ = _chunk(4, 6, 40, 9, 14, lost={0, 1, 5})
    with pytest.raises(ValueError, match="Not enough pieces to repair chunk 9"):
        piece.repair_chunks_checked([ec])
    with pytest.raises(ValueError, match="Not enough pieces to repair chunk 9"):
        piece.repair_pieces_checked(ec)
    assert stub.calls == []
    assert piece.repair_chunks_checked([]) == ([], [])
    with pytest.raises(ValueError):
        piece.repair_chunks_checked([ec, ec], targets=[[0]])


def test_target_held_by_the_caller_is_an_error_before_any_call(stub):
    ec, _ = _chunk(4, 6, 4 * 10, 0, 9, lost={1})
    with pytest.raises(piece.Error):
        piece.repair_pieces_checked(ec, targets=[5])  # held, as a check row
    assert stub.calls == []


def test_repair_chunks_is_unchanged_on_the_same_inputs(stub):
    """repair_chunks still reads only choose_blocks' k and makes its single repair call."""
    def inputs():
        (a, _), (b, _) = _chunk(4, 7, 4 * 64 - 1, 0, 4, lost={1}), _chunk(10, 14, 10 * 17 - 9, 1, 5, lost={0})
        _corrupt(a, 2, 17)
        return [a, b]
    got = piece.repair_chunks(inputs())
    ((kind, items),) = stub.calls
    assert kind == "repair" and [len(it[2]) for it in items] == [4, 10]
    for it, ch in zip(items, inputs()):
        have = sorted(p.piece_idx for p in ch.pieces)
        assert it[3] == [have[j] for j in choose_blocks(ch.k, ch.m, have)]
    assert [it[4] for it in items] == [[1], [0]]
    assert [[p.piece_idx for p in row] for row in got] == [[1], [0]]
