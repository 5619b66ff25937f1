"""CPU: piece.repair_chunks_corrected / repair_pieces_corrected, the host logic above
Engine.repair_correct_host: round one is repair_chunks_checked's fused call, only the chunks it
reports inconsistent go through ONE correcting call whose targets are the requested ones followed
(with heal) by every held piece, which pieces come back, the damaged map, the ids.  The engine is a
stand-in written here: repair_check_host on the oracle (as tests/test_repair_check_piece_api.py's),
repair_correct_host a per-column correction in numpy from engine.repair_matrix (host arithmetic,
the rule tests/test_decode_correct_piece_api.py ties to brute force) with cfec.easy_decode and
cfec.easy_encode behind it.  The GPU path below is tests/test_gpu_repair_correct.py's.  Damage is
applied here, and every expectation is where the test put it."""

import hashlib
import random

import numpy as np
import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import Error, check_check_item, check_repair_check_item, check_repair_correct_item, \
    check_repair_item, repair_matrix


def _gf_tables():
    exp, log = np.zeros(512, np.uint8), np.zeros(256, np.int64)
    v = 1
    for e in range(255):
        exp[e] = exp[e + 255] = v
        log[v] = e
        v <<= 1
        if v & 0x100:
            v ^= 0x11D
    return exp, log


EXP, LOG = _gf_tables()


def gf_mul(c: int, x: np.ndarray) -> np.ndarray:
    if c == 0:
        return np.zeros_like(x)
    return np.where(x == 0, 0, EXP[(LOG[x] + LOG[c]) % 255]).astype(np.uint8)


def gf_div(x: np.ndarray, c: int) -> np.ndarray:
    return np.where(x == 0, 0, EXP[(LOG[x] - LOG[c]) % 255]).astype(np.uint8)


def correct_columns(k, m, blocks, sharenums):
    """Per byte position, sec_check_locate's rule applied to the column of the n blocks: (basis,
    verdict) with basis = the first k blocks as arrays, the one wrong byte of a position put right,
    verdict[p] = -1 a code word, the entry changed, or -2 open."""
    nr = len(blocks) - k
    X = [np.frombuffer(bytes(b), np.uint8).copy() for b in blocks[:k]]
    verdict = np.full(X[0].size, -1, np.int64)
    if nr == 0:
        return X, verdict
    R = np.frombuffer(repair_matrix(k, m, list(sharenums[:k]), list(sharenums[k:])), np.uint8).reshape(nr, k)
    D = []
    for j in range(nr):
        d = np.frombuffer(bytes(blocks[k + j]), np.uint8).copy()
        for s in range(k):
            d ^= gf_mul(int(R[j][s]), X[s])
        D.append(d)
    cnt = sum((d != 0).astype(np.int64) for d in D)
    verdict[cnt > 0] = -2
    if nr < 2:
        return X, verdict
    for j in range(nr):
        verdict[(cnt == 1) & (D[j] != 0)] = k + j
    full = cnt == nr
    for s in range(k):
        if not R[0][s]:
            continue
        e = gf_div(D[0], int(R[0][s]))
        fits = full & (verdict == -2)
        for j in range(1, nr):
            fits &= gf_mul(int(R[j][s]), e) == D[j]
        verdict[fits] = s
        X[s][fits] ^= e[fits]
    return X, verdict


def _code_word(k, m, basis, sharenums):
    """All m blocks of the code word through the k basis blocks (the oracle's)."""
    return cfec.easy_encode(cfec.easy_decode([bytes(b) for b in basis], list(sharenums[:k]), 0, k, m), k, m)


def _oracle_check(k, m, blocks, sharenums):
    full = _code_word(k, m, blocks[:k], sharenums)
    bad, first = [], None
    for q in range(k, len(blocks)):
        d = np.flatnonzero(np.frombuffer(full[sharenums[q]], np.uint8) != np.frombuffer(blocks[q], np.uint8))
        if d.size:
            bad.append(q)
            first = int(d[0]) if first is None else min(first, int(d[0]))
    return (None, [], None) if first is None else (first, bad, bytes(b[first] for b in blocks))


class StandInEngine:
    """Engine.repair_check_host, check_host and repair_host on the oracle, repair_correct_host on
    correct_columns; records its calls."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _with_digests(out, digests, tail):
        digs = [[hashlib.sha1(b).digest() for b in row] for row in out]
        return (out, digs) + tail if digests else (out,) + tail

    def repair_check_host(self, items, digests=False):
        self.calls.append(("repair_check", items))
        out, checks = [], []
        for k, m, blocks, sharenums, targets in items:
            check_repair_check_item(k, m, blocks, sharenums, targets)
            full = _code_word(k, m, blocks[:k], sharenums)
            out.append([full[t] for t in targets])
            checks.append(_oracle_check(k, m, blocks, sharenums))
        return self._with_digests(out, digests, (checks,))

    def check_host(self, items):
        self.calls.append(("check", items))
        for it in items:
            check_check_item(*it)
        return [_oracle_check(*it) for it in items]

    def repair_host(self, items, digests=False):
        self.calls.append(("repair", items))
        out = []
        for k, m, blocks, sharenums, targets in items:
            check_repair_item(k, m, blocks, sharenums, targets)
            full = _code_word(k, m, blocks, sharenums)
            out.append([full[t] for t in targets])
        res = self._with_digests(out, digests, ())
        return res if digests else res[0]

    def repair_correct_host(self, items, digests=False):
        self.calls.append(("repair_correct", items))
        out, cor = [], []
        for k, m, blocks, sharenums, targets in items:
            check_repair_correct_item(k, m, blocks, sharenums, targets)
            X, verdict = correct_columns(k, m, blocks, sharenums)
            full = _code_word(k, m, [x.tobytes() for x in X], sharenums)
            out.append([full[t] for t in targets])
            bad, opened = np.flatnonzero(verdict != -1), np.flatnonzero(verdict == -2)
            cor.append((int(bad[0]) if bad.size else None, int(opened[0]) if opened.size else None,
                        int(np.count_nonzero(verdict >= 0)), int(opened.size),
                        [int(np.count_nonzero(verdict == q)) for q in range(len(blocks))]))
        return self._with_digests(out, digests, (cor,))


@pytest.fixture
def stub(monkeypatch):
    eng = StandInEngine()
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
            return
    raise AssertionError("piece not held")


def _kinds(stub):
    return [c[0] for c in stub.calls]


def _got(pieces):
    return [(p.piece_idx, p.data) for p in pieces]


def test_clean_input_is_round_one_alone(stub):
    (a, ba), (b, bb) = _chunk(4, 6, 4 * 50 - 3, 0, 1), _chunk(10, 14, 10 * 17 - 9, 1, 2, lost={3, 11})
    got, cors = piece.repair_chunks_corrected([a, b])
    assert _kinds(stub) == ["repair_check"]
    assert [_got(row) for row in got] == [[], [(3, bb[3]), (11, bb[11])]]
    assert cors == [piece.ChunkCorrection(chunk_idx=0, checked=6, consistent=True),
                    piece.ChunkCorrection(chunk_idx=1, checked=12, consistent=True)]
    want, checks = piece.repair_chunks_checked([a, b])  # the same round one, the same call
    assert stub.calls[0] == stub.calls[1] and len(stub.calls) == 2
    assert [_got(row) for row in want] == [_got(row) for row in got]
    assert [(c.chunk_idx, c.checked, c.consistent) for c in checks] == [(c.chunk_idx, c.checked, c.consistent)
                                                                        for c in cors]
    assert got[1][0].piece_type == piece.PieceType.Data and got[1][1].piece_type == piece.PieceType.Parity
    assert piece.repair_chunks_corrected([]) == ([], [])


def test_two_pieces_damaged_at_different_offsets_are_healed(stub):
    """RS(4,2), all six held, piece 1 bad at offset 100 and piece 4 at 9000: the dropping route
    names piece 1, is left with one check row and gives up; this one returns both healed."""
    ec, blocks = _chunk(4, 6, 4 * 10000 - 5, 7, 3)
    _corrupt(ec, 1, 100)
    _corrupt(ec, 4, 9000)
    _, (ck,) = piece.repair_chunks_checked([ec])
    assert (ck.consistent, ck.located, ck.bad_piece_idx) == (False, False, [1])  # the gap this closes
    stub.calls.clear()
    got, cor = piece.repair_pieces_corrected(ec, piece_ids=True)
    assert _got(got) == [(1, blocks[1]), (4, blocks[4])]
    assert [p.piece_id for p in got] == [hashlib.sha1(blocks[1]).hexdigest(), hashlib.sha1(blocks[4]).hexdigest()]
    assert all(isinstance(p, piece.ProcessedPieceInfo) and p.chunk_idx == 7 for p in got)
    assert cor == piece.ChunkCorrection(chunk_idx=7, checked=6, consistent=False, first_bad_offset=100,
                                        corrected_positions=2, open_positions=0, first_open_offset=None,
                                        damaged={1: 1, 4: 1})
    assert _kinds(stub) == ["repair_check", "repair_correct"]
    (item,) = stub.calls[1][1]
    assert item[:4] == stub.calls[0][1][0][:4]  # ordered as round one orders them
    assert item[4] == [0, 1, 2, 3, 4, 5]  # no piece absent: the held ones, ascending


def test_fewer_than_k_undamaged_pieces_left(stub):
    """Three pieces of RS(4,2) damaged at three offsets: no k undamaged pieces to repair from."""
    ec, blocks = _chunk(4, 6, 4 * 700, 0, 4)
    _corrupt(ec, 0, 3)
    _corrupt(ec, 2, 350, 0xFF)
    _corrupt(ec, 5, 699, 0x01)
    got, cor = piece.repair_pieces_corrected(ec)
    assert _got(got) == [(0, blocks[0]), (2, blocks[2]), (5, blocks[5])]
    assert (cor.damaged, cor.open_positions, cor.corrected_positions) == ({0: 1, 2: 1, 5: 1}, 0, 3)
    assert all(type(p) is piece.Piece for p in got)


def test_only_inconsistent_chunks_go_in_one_call(stub):
    chunks, blocks = zip(*[_chunk(10, 14, 10 * 300 - ci, ci, 10 + ci, lost={3}) for ci in range(5)])
    _corrupt(chunks[1], 0, 299)
    _corrupt(chunks[1], 0, 5)
    _corrupt(chunks[1], 12, 6)
    _corrupt(chunks[3], 2, 0)
    got, cors = piece.repair_chunks_corrected(list(chunks))
    assert _kinds(stub) == ["repair_check", "repair_correct"]
    again = stub.calls[1][1]
    assert [it[:4] for it in again] == [stub.calls[0][1][1][:4], stub.calls[0][1][3][:4]]
    held = [i for i in range(14) if i != 3]
    assert [it[4] for it in again] == [[3] + held, [3] + held]  # the requested target, then every held piece
    assert [[p.piece_idx for p in row] for row in got] == [[3], [3, 0, 12], [3], [3, 2], [3]]
    for ci, row in enumerate(got):
        assert all(p.data == blocks[ci][p.piece_idx] and p.chunk_idx == ci for p in row)
    assert [c.damaged for c in cors] == [{}, {0: 2, 12: 1}, {}, {2: 1}, {}]
    assert [c.first_bad_offset for c in cors] == [None, 5, None, 0, None]
    assert [c.consistent for c in cors] == [True, False, True, False, True]


def test_explicit_targets_and_no_heal(stub):
    ec, blocks = _chunk(10, 14, 10 * 64, 2, 30, lost={3, 13})
    _corrupt(ec, 7, 9)
    got, cor = piece.repair_pieces_corrected(ec, targets=[13], heal=False, piece_ids=True)
    assert _got(got) == [(13, blocks[13])] and got[0].piece_id == hashlib.sha1(blocks[13]).hexdigest()
    assert cor.damaged == {7: 1}  # named, not returned
    assert stub.calls[-1][1][0][4] == [13]
    got, cor = piece.repair_pieces_corrected(ec, targets=[13, 3])
    assert _got(got) == [(13, blocks[13]), (3, blocks[3]), (7, blocks[7])]
    with pytest.raises(Error):  # an explicit target must be absent
        piece.repair_pieces_corrected(ec, targets=[7])
    with pytest.raises(ValueError, match="one target list"):
        piece.repair_chunks_corrected([ec], [[3], [13]])
    with pytest.raises(ValueError, match="Not enough pieces to repair chunk 2"):
        piece.repair_chunks_corrected([piece.EncodedChunk(pieces=ec.pieces[:9], chunk_idx=2, k=10, m=14,
                                                          chunk_size=64, padlen=0, original_chunk_size=640)])


def test_open_positions_are_reported_and_left_as_the_basis_predicts(stub):
    """One spare piece corrects nothing; two errors at one offset of zfec(10,14) are open."""
    one, b1 = _chunk(4, 6, 4 * 64, 0, 20, lost={1})  # n - k = 1
    _corrupt(one, 0, 9)
    two, b2 = _chunk(10, 14, 10 * 40, 1, 21, lost={13})
    _corrupt(two, 3, 17)
    _corrupt(two, 12, 17, 0x21)
    _corrupt(two, 6, 30)
    got, cors = piece.repair_chunks_corrected([one, two])
    assert [(c.corrected_positions, c.open_positions, c.first_open_offset, c.damaged) for c in cors] == [
        (0, 1, 9, {}), (1, 1, 17, {6: 1})]
    assert [[p.piece_idx for p in row] for row in got] == [[1], [13, 6]]
    assert got[1][1].data == b2[6]
    # the lost pieces: right everywhere but at the open offset, where they are what the basis as held gives
    as_held = _code_word(10, 14, [p.data for p in two.pieces[:10]], list(range(10)))
    assert got[1][0].data[17] == as_held[13][17] != b2[13][17]
    assert [i for i in range(40) if got[1][0].data[i] != b2[13][i]] == [17]
    assert [i for i in range(64) if got[0][0].data[i] != b1[1][i]] == [9]
