"""CPU: piece.decode_chunks_corrected / reconstruct_data_corrected / reconstruct_data_stream_corrected,
the host logic above Engine.decode_correct_host: round one is decode_chunks_checked's fused call,
only the chunks it reports inconsistent go through ONE correcting call, the splice, the damaged
map, where the errors arrive.  The engine is a stand-in written here: decode_check_host on the
oracle (as tests/test_decode_check_piece_api.py's), decode_correct_host a per-column correction in
numpy from engine.repair_matrix (host arithmetic) with cfec.easy_decode behind it.  One test ties
that stand-in to brute force over all single and double errors of RS(4,6) columns, whose verdicts
come from the oracle alone.  The GPU path below is tests/test_gpu_decode_correct.py's.  Damage is
applied here, and every expectation is where the test put it."""

import itertools
import random

import numpy as np
import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import (check_check_item, check_decode_check_item, check_decode_correct_item, check_decode_item,
                              repair_matrix)


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
    """c * x over GF(2^8) / 0x11D, c a constant, x an array of bytes."""
    if c == 0:
        return np.zeros_like(x)
    return np.where(x == 0, 0, EXP[(LOG[x] + LOG[c]) % 255]).astype(np.uint8)


def gf_div(x: np.ndarray, c: int) -> np.ndarray:
    return np.where(x == 0, 0, EXP[(LOG[x] - LOG[c]) % 255]).astype(np.uint8)


def correct_columns(k, m, blocks, sharenums):
    """Per byte position, sec_check_locate's rule applied to the column of the n blocks: (basis,
    verdict) with basis = the first k blocks as arrays, the one wrong byte of a position put right,
    verdict[p] = -1 a code word, the entry changed, or -2 open."""
    n, nr = len(blocks), len(blocks) - k
    X = [np.frombuffer(bytes(b), np.uint8).copy() for b in blocks[:k]]
    B = X[0].size
    verdict = np.full(B, -1, np.int64)
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


class StandInEngine:
    """Engine.decode_check_host, check_host and decode_host on the oracle, decode_correct_host on
    correct_columns; records its calls."""

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

    def decode_correct_host(self, items):
        self.calls.append(("decode_correct", items))
        data, out = b"", []
        for k, m, blocks, sharenums, padlen in items:
            check_decode_correct_item(k, m, blocks, sharenums, padlen)
            X, verdict = correct_columns(k, m, blocks, sharenums)
            data += cfec.easy_decode([x.tobytes() for x in X], list(sharenums[:k]), padlen, k, m)
            bad, opened = np.flatnonzero(verdict != -1), np.flatnonzero(verdict == -2)
            out.append((int(bad[0]) if bad.size else None, int(opened[0]) if opened.size else None,
                        int(np.count_nonzero(verdict >= 0)), int(opened.size),
                        [int(np.count_nonzero(verdict == q)) for q in range(len(blocks))]))
        return data, out


@pytest.fixture
def stub(monkeypatch):
    eng = StandInEngine()
    monkeypatch.setattr(piece, "get_engine", lambda device=None: eng)
    return eng


def test_stand_in_agrees_with_brute_force_on_rs46_columns():
    """Every single error (6 entries x 255 values) and every double error (15 pairs x 255 x 255)
    added to RS(4,6) code words, one column per byte position.  Brute force, from the oracle alone:
    changing entry i alone can give a code word exactly when the other five entries are consistent,
    i.e. when the code word through four of them also passes through the fifth; the value entry i
    must take is that code word's.  The stand-in must name that entry and reach that code word,
    and call open what no entry explains."""
    k, m = 4, 6
    singles = [(i, a, 0, 0) for i in range(m) for a in range(1, 256)]
    vals = np.arange(1, 256)
    a2, b2 = [g.ravel() for g in np.meshgrid(vals, vals, indexing="ij")]
    N = len(singles) + 15 * a2.size
    rng = np.random.default_rng(46)
    word = [np.frombuffer(b, np.uint8).copy()
            for b in cfec.easy_encode(rng.integers(0, 256, k * N, dtype=np.uint8).tobytes(), k, m)]
    held = [w.copy() for w in word]
    wrong = np.zeros((m, N), bool)  # where the test put the errors
    for p, (i, a, _, _) in enumerate(singles):
        held[i][p] ^= a
        wrong[i][p] = True
    at = len(singles)
    for i, j in itertools.combinations(range(m), 2):
        held[i][at:at + a2.size] ^= a2.astype(np.uint8)
        held[j][at:at + a2.size] ^= b2.astype(np.uint8)
        wrong[i][at:at + a2.size] = wrong[j][at:at + a2.size] = True
        at += a2.size
    assert at == N

    # brute force: entry i explains a column iff the code word through four of the others meets the fifth
    explains = np.zeros((m, N), bool)
    through = {}
    for i in range(m):
        rest = [q for q in range(m) if q != i]
        data = cfec.easy_decode([held[q].tobytes() for q in rest[:k]], rest[:k], 0, k, m)
        cw = [np.frombuffer(b, np.uint8) for b in cfec.easy_encode(data, k, m)]
        explains[i] = cw[rest[k]] == held[rest[k]]
        through[i] = cw
    assert explains.sum(axis=0).max() == 1  # distance 3: never two explanations
    assert (explains[:, :len(singles)] == wrong[:, :len(singles)]).all()  # a single error is always found
    assert not (explains & wrong)[:, len(singles):].any()  # a double error is never pinned on one of its own two

    order = [5, 0, 3, 2, 4, 1]  # the basis holds a parity block, and entries are not in block order
    X, verdict = correct_columns(k, m, [held[b].tobytes() for b in order], order)
    want = np.full(N, -2, np.int64)
    for q, b in enumerate(order):
        want[explains[b]] = q
    assert (verdict == want).all()
    for q, b in enumerate(order[:k]):  # the corrected basis lies on the explaining entry's code word
        for i in range(m):
            sel = explains[i]
            assert (X[q][sel] == through[i][b][sel]).all()
        assert (X[q][want == -2] == held[b][want == -2]).all()  # open: left as held


def _chunk(k, m, n, chunk_idx, seed, lost=()):
    data = bytes(random.Random(seed).randrange(256) for _ in range(n))
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    pieces = [piece.Piece(chunk_idx=chunk_idx, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks) if i not in lost]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=k * B - n,
                            original_chunk_size=n)
    return ec, data


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


def test_clean_input_makes_no_correcting_call(stub):
    (a, da), (b, db) = _chunk(4, 6, 4 * 50 - 3, 0, 1), _chunk(10, 14, 10 * 17 - 9, 1, 2, lost={3})
    data, cors = piece.decode_chunks_corrected([a, b])
    assert data == da + db and _kinds(stub) == ["decode_check"]
    assert cors == [piece.ChunkCorrection(chunk_idx=0, checked=6, consistent=True),
                    piece.ChunkCorrection(chunk_idx=1, checked=13, consistent=True)]
    want, checks = piece.decode_chunks_checked([a, b])  # the same round one, the same call
    assert want == data and stub.calls[0] == stub.calls[1]
    assert [(c.chunk_idx, c.checked, c.consistent) for c in checks] == [(c.chunk_idx, c.checked, c.consistent)
                                                                        for c in cors]
    assert piece.decode_chunks_corrected([]) == (b"", [])


def test_two_pieces_damaged_at_different_offsets(stub):
    """RS(4,2), piece 1 bad at offset 100 and piece 4 at 9000: the dropping route names piece 1, is
    left with one check row and gives up; the correcting route returns the chunk."""
    ec, data = _chunk(4, 6, 4 * 10000 - 5, 7, 3)
    _corrupt(ec, 1, 100)
    _corrupt(ec, 4, 9000)
    _, (ck,) = piece.decode_chunks_checked([ec])
    assert (ck.consistent, ck.located, ck.bad_piece_idx) == (False, False, [1])  # the gap this closes
    stub.calls.clear()
    got, (cor,) = piece.decode_chunks_corrected([ec])
    assert got == data
    assert cor == piece.ChunkCorrection(chunk_idx=7, checked=6, consistent=False, first_bad_offset=100,
                                        corrected_positions=2, open_positions=0, first_open_offset=None,
                                        damaged={1: 1, 4: 1})
    assert _kinds(stub) == ["decode_check", "decode_correct"]
    assert piece.reconstruct_data_corrected(list(ec.pieces), [ec])[0] == data


def test_only_inconsistent_chunks_go_in_one_call_and_are_spliced(stub):
    chunks, datas = zip(*[_chunk(4, 6, 4 * 300 - ci, ci, 10 + ci) for ci in range(5)])
    _corrupt(chunks[1], 0, 299)
    _corrupt(chunks[1], 0, 5)
    _corrupt(chunks[1], 5, 6)
    _corrupt(chunks[3], 2, 0)
    got, cors = piece.decode_chunks_corrected(list(chunks))
    assert got == b"".join(datas)
    assert _kinds(stub) == ["decode_check", "decode_correct"]
    assert [len(it[2]) for it in stub.calls[1][1]] == [6, 6]  # chunks 1 and 3, every piece held
    assert stub.calls[1][1] == [stub.calls[0][1][1], stub.calls[0][1][3]]  # ordered as round one orders them
    assert [c.damaged for c in cors] == [{}, {0: 2, 5: 1}, {}, {2: 1}, {}]
    assert [c.first_bad_offset for c in cors] == [None, 5, None, 0, None]
    assert [c.consistent for c in cors] == [True, False, True, False, True]


def test_open_positions_raise(stub):
    """One spare piece corrects nothing; two errors at one offset of zfec(10,14) are open."""
    one, d1 = _chunk(4, 6, 4 * 64, 0, 20, lost={1})  # n - k = 1
    _corrupt(one, 0, 9)
    two, d2 = _chunk(10, 14, 10 * 40, 1, 21)
    _corrupt(two, 3, 17)
    _corrupt(two, 12, 17, 0x21)
    _corrupt(two, 6, 30)
    good, d3 = _chunk(4, 6, 4 * 64, 2, 22)
    data, cors = piece.decode_chunks_corrected([one, two, good])
    assert [(c.corrected_positions, c.open_positions, c.first_open_offset, c.damaged) for c in cors] == [
        (0, 1, 9, {}), (1, 1, 17, {6: 1}), (0, 0, None, {})]
    assert data[len(d1) + len(d2):] == d3
    held = data[len(d1):len(d1) + len(d2)]
    assert [i for i in range(len(d2)) if held[i] != d2[i]] == [3 * 40 + 17]  # offset 30 put right, 17 left as held
    pieces = [p for ch in (one, two, good) for p in ch.pieces]
    with pytest.raises(piece.PieceCorrectionError) as e:
        piece.reconstruct_data_corrected(pieces, [one, two, good])
    assert [c.open_positions for c in e.value.checks] == [1, 1, 0] and "[0, 1]" in str(e.value)
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 2"):
        piece.reconstruct_data_corrected([p for p in pieces if p.chunk_idx != 2], [one, two, good])


def test_stream_yields_until_the_open_chunk(stub):
    chunks, datas = zip(*[_chunk(10, 14, 10 * 80, ci, 30 + ci) for ci in range(4)])
    _corrupt(chunks[0], 3, 7)
    _corrupt(chunks[0], 11, 8)
    _corrupt(chunks[2], 1, 50)
    _corrupt(chunks[2], 2, 50)  # two at one offset, four spare pieces: open
    pieces = [p for ch in chunks for p in ch.pieces]
    seen = []
    with pytest.raises(piece.PieceCorrectionError) as e:
        for data, ck in piece.reconstruct_data_stream_corrected(pieces, list(chunks), window_bytes=1):
            seen.append((data, ck))
    assert [c.chunk_idx for c in e.value.checks] == [0, 1, 2] and e.value.checks[-1].open_positions == 1
    assert len(seen) == 2
    assert seen[0] == (datas[0], piece.ChunkCorrection(chunk_idx=0, checked=14, consistent=False, first_bad_offset=7,
                                                       corrected_positions=2, damaged={3: 1, 11: 1}))
    assert seen[1][0] == datas[1] and seen[1][1].consistent
    clean = [ch for ch in chunks if ch.chunk_idx != 2]
    got = list(piece.reconstruct_data_stream_corrected([p for ch in clean for p in ch.pieces], clean))
    assert b"".join(d for d, _ in got) == datas[0] + datas[1] + datas[3]
