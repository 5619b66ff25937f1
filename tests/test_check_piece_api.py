"""CPU: piece.check_chunks / check_pieces, the host logic above Engine.check_host: the basis, the
locate and re-check rounds, what is reported.  The engine is a stub whose check_host IS the oracle
(cfec.easy_decode of the basis, cfec.easy_encode, a numpy compare), so no GPU is needed; the GPU
path below it is tests/test_gpu_check.py's.  Corruptions are applied here, in numpy, and every
expectation is where the test put them."""

import random

import numpy as np
import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import check_check_item, choose_blocks


class OracleCheckEngine:
    """Engine.check_host on the oracle; records the items it was handed."""

    def __init__(self):
        self.calls = []

    def check_host(self, items):
        self.calls.append(items)
        out = []
        for k, m, blocks, sharenums in items:
            check_check_item(k, m, blocks, sharenums)
            data = cfec.easy_decode([bytes(b) for b in blocks[:k]], list(sharenums[:k]), 0, k, m)
            full = cfec.easy_encode(data, k, m)
            bad, first = [], None
            for q in range(k, len(blocks)):
                d = np.flatnonzero(np.frombuffer(full[sharenums[q]], np.uint8) != np.frombuffer(blocks[q], np.uint8))
                if d.size:
                    bad.append(q)
                    first = int(d[0]) if first is None else min(first, int(d[0]))
            out.append((None, [], None) if first is None else (first, bad, bytes(b[first] for b in blocks)))
        return out


@pytest.fixture
def stub(monkeypatch):
    eng = OracleCheckEngine()
    monkeypatch.setattr(piece, "get_engine", lambda device=None: eng)
    return eng


def _chunk(k, m, n, chunk_idx, seed):
    data = bytes(random.Random(seed).randrange(256) for _ in range(n))
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    pieces = [piece.Piece(chunk_idx=chunk_idx, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks)]
    return piece.EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=k * B - n,
                              original_chunk_size=n)


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


def test_clean_chunk_is_consistent(stub):
    got = piece.check_pieces(_chunk(4, 6, 4 * 50 - 3, 7, seed=1))
    assert got == piece.ChunkCheck(chunk_idx=7, checked=6, consistent=True, first_bad_offset=None, bad_piece_idx=[],
                                   located=False)
    assert len(stub.calls) == 1


def test_basis_is_the_choosers_pick(stub):
    ec = _drop(_chunk(4, 8, 4 * 40, 3, seed=2), {2})  # 7 held, in shuffled order, one of them twice
    random.Random(5).shuffle(ec.pieces)
    ec.pieces.append(ec.pieces[0])
    got = piece.check_pieces(ec)
    assert got.consistent and got.checked == 7
    ((item,),) = stub.calls
    have = sorted({p.piece_idx for p in ec.pieces})
    basis = [have[j] for j in choose_blocks(4, 8, have)]
    assert item[3][:4] == basis and {0, 1, 3} <= set(basis)  # every held primary is in the basis
    assert item[3][4:] == [s for s in have if s not in basis]  # the others are the check rows
    by_idx = {p.piece_idx: p.data for p in ec.pieces}
    assert item[2] == [by_idx[s] for s in item[3]]
    # all primaries held: the check rows are the parity pieces, plain encode rows
    stub.calls.clear()
    piece.check_pieces(_chunk(4, 6, 64, 0, seed=3))
    assert stub.calls[0][0][3] == [0, 1, 2, 3, 4, 5]


def test_one_corrupt_piece_per_chunk_is_located_after_one_batched_recheck(stub):
    a = _corrupt(_chunk(4, 6, 4 * 64, 0, seed=4), 1, 17)        # a data piece (in the basis)
    b = _corrupt(_chunk(10, 14, 10 * 17 - 9, 1, seed=5), 12, 3)  # a parity piece (a check row)
    c = _chunk(4, 6, 4 * 20, 2, seed=6)                           # clean
    got = piece.check_chunks([a, b, c])
    assert [(g.chunk_idx, g.checked, g.consistent, g.first_bad_offset, g.bad_piece_idx, g.located) for g in got] == [
        (0, 6, False, 17, [1], True), (1, 14, False, 3, [12], True), (2, 6, True, None, [], False)]
    assert [len(call) for call in stub.calls] == [3, 2]  # the first check, then ONE call re-checking both
    assert [it[3] for it in stub.calls[1]] == [[0, 2, 3, 4, 5], [s for s in range(14) if s != 12]]


def test_locate_off_reports_only_the_check(stub):
    got = piece.check_pieces(_corrupt(_chunk(4, 6, 4 * 64, 0, seed=4), 1, 17), locate=False)
    assert (got.consistent, got.first_bad_offset, got.bad_piece_idx, got.located) == (False, 17, [], False)
    assert len(stub.calls) == 1


def test_two_corrupt_pieces_at_different_offsets_take_two_rounds(stub):
    ec = _corrupt(_corrupt(_chunk(4, 8, 4 * 40, 5, seed=7), 2, 30), 6, 9)
    got = piece.check_pieces(ec)
    assert (got.consistent, got.first_bad_offset, got.located) == (False, 9, True)
    assert got.bad_piece_idx == [6, 2]  # in the order found: offset 9 first
    assert [sorted(call[0][3]) for call in stub.calls] == [
        list(range(8)), [0, 1, 2, 3, 4, 5, 7], [0, 1, 3, 4, 5, 7]]


def test_two_corrupt_pieces_at_the_same_offset_are_not_located(stub):
    """Four check rows, two errors in one column: no single piece explains it (no three columns of
    [R | I] are dependent), so nothing is named."""
    ec = _corrupt(_corrupt(_chunk(4, 8, 4 * 40, 5, seed=8), 2, 30, 0x11), 6, 30, 0xE0)
    got = piece.check_pieces(ec)
    assert (got.consistent, got.first_bad_offset, got.bad_piece_idx, got.located) == (False, 30, [], False)
    assert len(stub.calls) == 1


def test_one_spare_piece_detects_but_cannot_locate(stub):
    ec = _corrupt(_drop(_chunk(4, 6, 4 * 40, 9, seed=9), {5}), 0, 2)
    got = piece.check_pieces(ec)
    assert (got.checked, got.consistent, got.first_bad_offset, got.bad_piece_idx, got.located) == (5, False, 2, [], False)
    assert len(stub.calls) == 1


def test_exactly_k_pieces_have_nothing_to_check(stub):
    got = piece.check_pieces(_corrupt(_drop(_chunk(4, 6, 4 * 40, 9, seed=9), {1, 5}), 0, 2))
    assert (got.checked, got.consistent, got.located) == (4, True, False)


def test_not_enough_pieces(stub):
    ec = _drop(_chunk(4, 6, 4 * 10, 9, seed=10), {0, 1, 5})
    with pytest.raises(ValueError, match="Not enough pieces to check chunk 9"):
        piece.check_pieces(ec)
    with pytest.raises(ValueError):  # what repair_chunks raises for the same chunk
        piece.repair_pieces(ec)
    assert stub.calls == []
    assert piece.check_chunks([]) == []
