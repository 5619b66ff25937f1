"""CPU: piece.repair_pieces / repair_chunks, the host logic above Engine.repair_host: default
targets, the choice of k survivors, piece types and ids, the error for too few pieces.  The engine
is a stub whose repair_host IS the oracle (cfec.easy_decode then cfec.easy_encode), so no GPU is
needed; the GPU path below it is tests/test_gpu_repair.py's."""

import hashlib
import random

import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import check_repair_item, choose_blocks


class OracleRepairEngine:
    """Engine.repair_host on the oracle; records the items it was handed."""

    def __init__(self):
        self.calls = []

    def repair_host(self, items, digests=False):
        self.calls.append(items)
        out, digs = [], []
        for k, m, blocks, sharenums, targets in items:
            check_repair_item(k, m, blocks, sharenums, targets)
            B = len(blocks[0])
            data = cfec.easy_decode([bytes(b) for b in blocks], list(sharenums), 0, k, m)
            assert len(data) == k * B
            full = cfec.easy_encode(data, k, m)
            out.append([full[t] for t in targets])
            digs.append([hashlib.sha1(full[t]).digest() for t in targets])
        return (out, digs) if digests else out


@pytest.fixture
def stub(monkeypatch):
    eng = OracleRepairEngine()
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
    return ec, blocks


def _drop(ec, lost):
    ec.pieces = [p for p in ec.pieces if p.piece_idx not in lost]
    return ec


def test_default_targets_are_the_absent_pieces(stub):
    ec, blocks = _chunk(4, 6, 4 * 50 - 3, 7, seed=1)
    got = piece.repair_pieces(_drop(ec, {1, 5}))
    assert [p.piece_idx for p in got] == [1, 5]
    assert [p.data for p in got] == [blocks[1], blocks[5]]
    assert [p.piece_type for p in got] == [piece.PieceType.Data, piece.PieceType.Parity]
    assert all(p.chunk_idx == 7 and type(p) is piece.Piece for p in got)
    (items,) = stub.calls
    assert items[0][3] == [0, 2, 3, 4] and items[0][4] == [1, 5]


def test_explicit_targets_keep_their_order(stub):
    ec, blocks = _chunk(10, 14, 10 * 33 - 4, 0, seed=2)
    got = piece.repair_pieces(_drop(ec, {0, 9, 12, 13}), targets=[12, 9, 0])
    assert [p.piece_idx for p in got] == [12, 9, 0]
    assert [p.data for p in got] == [blocks[12], blocks[9], blocks[0]]  # block 9: its zero padding included
    assert [p.piece_type for p in got] == [piece.PieceType.Parity, piece.PieceType.Data, piece.PieceType.Data]


def test_more_than_k_survivors_reads_the_chosen_k(stub):
    ec, blocks = _chunk(4, 8, 4 * 40, 3, seed=3)
    _drop(ec, {2})  # 7 survivors, in shuffled order
    random.Random(5).shuffle(ec.pieces)
    got = piece.repair_pieces(ec)
    assert [(p.piece_idx, p.data) for p in got] == [(2, blocks[2])]
    (items,) = stub.calls
    have = sorted(p.piece_idx for p in ec.pieces)
    want = [have[j] for j in choose_blocks(4, 8, have)]
    assert items[0][3] == want and len(want) == 4
    assert {0, 1, 3} <= set(want)  # every present primary is kept
    assert items[0][2] == [blocks[s] for s in want]


def test_piece_ids(stub):
    ec, blocks = _chunk(3, 5, 3 * 21 - 1, 11, seed=4)
    got = piece.repair_pieces(_drop(ec, {0, 4}), piece_ids=True)
    assert all(type(p) is piece.ProcessedPieceInfo for p in got)
    assert [p.piece_id for p in got] == [hashlib.sha1(blocks[0]).hexdigest(), hashlib.sha1(blocks[4]).hexdigest()]
    assert [p.piece_id for p in got] == [piece.piece_hash(p.data) for p in got]


def test_repair_chunks_is_one_call(stub):
    a, ba = _chunk(4, 6, 4 * 64, 0, seed=5)
    b, bb = _chunk(10, 14, 10 * 17 - 9, 1, seed=6)
    c, _ = _chunk(1, 3, 9, 2, seed=7)
    got = piece.repair_chunks([_drop(a, {0}), _drop(b, {3, 11}), c], targets=[None, [11, 3], None])
    assert len(stub.calls) == 1 and len(stub.calls[0]) == 3
    assert [[p.piece_idx for p in row] for row in got] == [[0], [11, 3], []]
    assert got[0][0].data == ba[0] and [p.data for p in got[1]] == [bb[11], bb[3]]
    assert [p.chunk_idx for row in got for p in row] == [0, 1, 1]
    assert piece.repair_chunks([]) == []
    with pytest.raises(ValueError):
        piece.repair_chunks([a, b], targets=[[0]])


def test_not_enough_pieces(stub):
    ec, _ = _chunk(4, 6, 4 * 10, 9, seed=8)
    with pytest.raises(ValueError, match="Not enough pieces to repair chunk 9"):
        piece.repair_pieces(_drop(ec, {0, 1, 5}))
    assert stub.calls == []


def test_target_held_by_the_caller_is_an_error(stub):
    ec, _ = _chunk(4, 6, 4 * 10, 0, seed=9)
    with pytest.raises(piece.Error):
        piece.repair_pieces(_drop(ec, {1, 5}), targets=[0])
