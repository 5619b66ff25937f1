"""CPU: piece.decode_chunks_id_checked / reconstruct_data_id_checked /
reconstruct_data_stream_id_checked: which pieces are hashed and which ids are read, that chunks are
decoded from pieces that passed only, who hashes, where the errors arrive.  The engine is
tests.engine_stub.OracleHostEngine (the oracle behind decode_host) with sha1_host added on
hashlib, so no GPU is needed; the GPU run is tests/test_gpu_decode_ids_piece.py's.  Corruptions are
applied here, and every expectation is where the test put them."""

import hashlib
import random
import threading

import pytest

from oracle import cfec
from storb_amd import piece
from storb_amd.engine import choose_blocks
from tests.engine_stub import OracleHostEngine


class IdsOracleEngine(OracleHostEngine):
    """decode_host is OracleHostEngine's (the oracle behind decode_batch), sha1_host is hashlib's.
    Records its calls (the stream worker makes them, so under a lock)."""

    def __init__(self):
        super().__init__()
        self.calls = []
        self.lock = threading.Lock()
        self.running = 0

    def sha1_host(self, datas):
        with self.lock:
            self.calls.append(("sha1", list(datas)))
        return [hashlib.sha1(bytes(d)).digest() for d in datas]

    def decode_host(self, items):
        with self.lock:
            self.calls.append(("decode", items))
            self.running += 1
        try:
            return super().decode_host(items)
        finally:
            with self.lock:
                self.running -= 1


@pytest.fixture
def stub(monkeypatch):
    eng = IdsOracleEngine()
    monkeypatch.setattr(piece, "get_engine", lambda device=None: eng)
    return eng


def _chunk(k, m, n, chunk_idx, seed):
    """(chunk holding all m pieces, its data, the m recorded ids as 40-hex strings)."""
    data = bytes(random.Random(seed).randrange(256) for _ in range(n))
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    pieces = [piece.Piece(chunk_idx=chunk_idx, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks)]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=k * B - n,
                            original_chunk_size=n)
    return ec, data, [hashlib.sha1(b).hexdigest() for b in blocks]


def _corrupt(pieces, chunk_idx, piece_idx, offset, value=0x40):
    for p in pieces:
        if (p.chunk_idx, p.piece_idx) == (chunk_idx, piece_idx):
            b = bytearray(p.data)
            b[offset] ^= value
            p.data = bytes(b)
            return
    raise AssertionError("piece not held")


def _drop(ec, lost):
    ec.pieces = [p for p in ec.pieces if p.piece_idx not in lost]
    return ec


def _kinds(stub):
    return [c[0] for c in stub.calls]


def test_all_ids_good_is_one_decode_from_the_chosen_pieces(stub):
    (a, da, ia), (b, db, ib), (c, dc, ic) = (_chunk(4, 6, 4 * 50 - 3, 0, 1), _chunk(10, 14, 10 * 17 - 9, 1, 2),
                                             _chunk(4, 8, 160, 2, 3))
    _drop(b, {3, 11})  # a data piece lost: recovered
    random.Random(5).shuffle(c.pieces)
    c.pieces.append(c.pieces[0])  # held twice: hashed and used once
    data, checks = piece.decode_chunks_id_checked([a, b, c], [ia, ib, ic])
    assert data == da + db + dc
    assert checks == [piece.ChunkIdCheck(chunk_idx=0, checked=6, ok=True, bad_piece_idx=[], decodable=True),
                      piece.ChunkIdCheck(chunk_idx=1, checked=12, ok=True, bad_piece_idx=[], decodable=True),
                      piece.ChunkIdCheck(chunk_idx=2, checked=8, ok=True, bad_piece_idx=[], decodable=True)]
    ((kind, items),) = stub.calls  # ONE decode call; the hashing ran on the thread pool
    assert kind == "decode" and [len(it[2]) for it in items] == [4, 10, 4]
    have = [s for s in range(14) if s not in (3, 11)]
    assert items[1][3] == [have[j] for j in choose_blocks(10, 14, have)]  # choose_blocks' pick
    assert [it[4] for it in items] == [a.padlen, b.padlen, c.padlen]


def test_bad_spare_piece_leaves_the_bytes_alone(stub):
    (a, da, ia), (b, db, ib) = _chunk(4, 6, 4 * 64 - 1, 0, 4), _chunk(10, 14, 10 * 17 - 9, 1, 5)
    _corrupt(b.pieces, 1, 12, 3)  # a parity piece
    data, checks = piece.decode_chunks_id_checked([a, b], [ia, ib])
    assert data == da + db
    assert (checks[1].ok, checks[1].bad_piece_idx, checks[1].decodable, checks[1].checked) == (False, [12], True, 14)
    assert checks[0].ok and _kinds(stub) == ["decode"]


def test_bad_data_piece_with_a_spare_is_not_decoded_from(stub):
    (a, da, ia), (b, db, ib), (c, dc, ic) = (_chunk(4, 6, 61, 0, 7), _chunk(4, 8, 4 * 40 - 2, 1, 8),
                                             _chunk(4, 6, 97, 2, 9))
    _corrupt(b.pieces, 1, 2, 30)  # a data piece of the middle chunk: choose_blocks would pick it
    _corrupt(b.pieces, 1, 6, 9)   # and a parity piece
    data, checks = piece.decode_chunks_id_checked([a, b, c], [ia, ib, ic])
    assert data == da + db + dc
    assert (checks[1].ok, checks[1].bad_piece_idx, checks[1].decodable) == (False, [2, 6], True)
    assert _kinds(stub) == ["decode"]  # ONE decode, from good pieces only
    items = stub.calls[0][1]
    assert len(items[1][2]) == 4 and not {2, 6} & set(items[1][3]) and items[1][4] == b.padlen


def test_fewer_than_k_good_pieces_cannot_be_trusted(stub):
    ec, data, ids = _chunk(4, 6, 4 * 40, 9, 10)
    _corrupt(_drop(ec, {4, 5}).pieces, 9, 0, 2)
    got, checks = piece.decode_chunks_id_checked([ec], [ids])
    assert (checks[0].checked, checks[0].ok, checks[0].bad_piece_idx, checks[0].decodable) == (4, False, [0], False)
    assert got != data and len(got) == len(data) and _kinds(stub) == ["decode"]  # what the first k decode to
    clean, dclean, iclean = _chunk(4, 6, 33, 3, 11)
    with pytest.raises(piece.PieceIdError) as e:
        piece.reconstruct_data_id_checked(ec.pieces + clean.pieces, [clean, ec], [iclean, ids])
    assert isinstance(e.value, ValueError) and "[9]" in str(e.value)
    assert [(c.chunk_idx, c.decodable) for c in e.value.checks] == [(3, True), (9, False)]


def test_hex_and_bytes_ids_and_a_mapping(stub):
    ec, data, ids = _chunk(4, 6, 50, 0, 12)
    assert piece.decode_chunks_id_checked([ec], [[bytes.fromhex(x) for x in ids]])[0] == data
    assert piece.decode_chunks_id_checked([ec], [[x.upper() for x in ids]])[1][0].ok
    _drop(ec, {1, 4})
    got, checks = piece.decode_chunks_id_checked([ec], [{i: ids[i] for i in (0, 2, 3, 5)}])  # only the held ones are read
    assert got == data and checks[0].ok and checks[0].checked == 4
    wrong = list(ids)
    wrong[5] = ids[4]  # another piece's id
    assert piece.decode_chunks_id_checked([ec], [wrong])[1][0].bad_piece_idx == [5]


def test_missing_or_malformed_id_is_a_value_error_before_any_call(stub):
    ec, _, ids = _chunk(4, 6, 50, 7, 13)
    with pytest.raises(ValueError, match="No recorded id for piece 5 of chunk 7"):
        piece.decode_chunks_id_checked([ec], [ids[:5]])
    with pytest.raises(ValueError, match="No recorded id for piece 2 of chunk 7"):
        piece.decode_chunks_id_checked([ec], [ids[:2] + [None] + ids[3:]])
    with pytest.raises(ValueError):
        piece.decode_chunks_id_checked([ec], [ids[:2] + [ids[2][:38]] + ids[3:]])  # 19 bytes
    with pytest.raises(ValueError):
        piece.decode_chunks_id_checked([ec], [])  # one id list per chunk
    assert stub.calls == []
    assert piece.decode_chunks_id_checked([], []) == (b"", [])


def test_fewer_than_k_pieces(stub):
    ec, _, ids = _chunk(4, 6, 40, 9, 14)
    _drop(ec, {0, 1, 5})
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 9"):
        piece.reconstruct_data_id_checked(ec.pieces, [ec], [ids])
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 9"):
        piece.decode_chunks_id_checked([ec], [ids])
    assert stub.calls == []


def test_method_rule_chooses_per_call(stub, monkeypatch):
    ec, data, ids = _chunk(4, 6, 50, 0, 15)
    _corrupt(ec.pieces, 0, 5, 1)
    seen = []
    monkeypatch.setattr(piece, "_ids_on_gpu", lambda n, b: seen.append((n, b)) or True)
    got, checks = piece.decode_chunks_id_checked([ec], [ids])
    assert got == data and checks[0].bad_piece_idx == [5]
    assert seen == [(6, 13)] and _kinds(stub) == ["sha1", "decode"]  # ONE SHA-1 call over every held piece
    assert stub.calls[0][1] == [p.data for p in ec.pieces]
    stub.calls.clear()
    monkeypatch.setattr(piece, "_ids_on_gpu", lambda n, b: False)
    assert piece.decode_chunks_id_checked([ec], [ids]) == (got, checks) and _kinds(stub) == ["decode"]
    assert not piece._ids_on_gpu(10 ** 6, 1)  # the default: the thread pool everywhere


SHAPES = [(4, 6, 4 * 50 - 3), (10, 14, 10 * 17 - 9), (4, 8, 160), (8, 11, 8 * 30 - 5), (4, 6, 97), (16, 24, 16 * 9 - 1)]


def _object(seed=0):
    made = [_chunk(k, m, n, i, seed + i) for i, (k, m, n) in enumerate(SHAPES)]
    pieces = [p for ec, _, _ in made for p in ec.pieces]
    random.Random(seed).shuffle(pieces)
    chunks = [ec for ec, _, _ in made]
    for ec in chunks:
        ec.pieces = []
    return chunks, pieces, [d for _, d, _ in made], [i for _, _, i in made]


def _fresh(chunks):
    for ec in chunks:
        ec.pieces = []
    return chunks


@pytest.mark.parametrize("window_bytes,nwin", [(1, 6), (400, 3), (1 << 20, 1)])
def test_stream_yields_in_order_what_reconstruct_returns(stub, window_bytes, nwin):
    chunks, pieces, datas, ids = _object(1)
    _corrupt(pieces, 1, 12, 3)   # a parity piece
    _corrupt(pieces, 3, 2, 11)   # a data piece: not decoded from
    want_data, want_checks = piece.reconstruct_data_id_checked(pieces, _fresh(chunks), ids)
    assert want_data == b"".join(datas)
    stub.calls.clear()
    got = list(piece.reconstruct_data_stream_id_checked(pieces, _fresh(chunks), ids, window_bytes=window_bytes))
    assert [d for d, _ in got] == datas
    assert [c for _, c in got] == want_checks
    assert [(c.chunk_idx, c.ok, c.bad_piece_idx, c.decodable) for _, c in got] == [
        (0, True, [], True), (1, False, [12], True), (2, True, [], True), (3, False, [2], True),
        (4, True, [], True), (5, True, [], True)]
    assert _kinds(stub).count("decode") == nwin


def test_stream_errors_arrive_after_every_earlier_chunk(stub):
    chunks, pieces, datas, ids = _object(4)
    pieces = [p for p in pieces if not (p.chunk_idx == 4 and p.piece_idx in (2, 3))]  # (4, 6): exactly k left
    _corrupt(pieces, 4, 1, 20)
    got = []
    with pytest.raises(piece.PieceIdError) as e:
        for pair in piece.reconstruct_data_stream_id_checked(pieces, chunks, ids, window_bytes=SHAPES[0][2] + SHAPES[1][2]):
            got.append(pair)
    assert [d for d, _ in got] == datas[:4] and "chunk 4" in str(e.value)
    assert [(c.chunk_idx, c.decodable) for c in e.value.checks] == [(0, True), (1, True), (2, True), (3, True), (4, False)]
    chunks, pieces, datas, ids = _object(5)
    pieces = [p for p in pieces if not (p.chunk_idx == 3 and p.piece_idx < 4)]  # (8, 11): 7 left
    got = []
    with pytest.raises(ValueError, match="Not enough pieces to reconstruct chunk 3") as e2:
        for pair in piece.reconstruct_data_stream_id_checked(pieces, chunks, ids, window_bytes=400):
            got.append(pair)
    assert not isinstance(e2.value, piece.PieceIdError) and [d for d, _ in got] == datas[:3]


def test_closing_the_stream_early_leaves_no_window_running(stub):
    chunks, pieces, datas, ids = _object(6)
    stream = piece.reconstruct_data_stream_id_checked(pieces, chunks, ids, window_bytes=1)  # six windows
    assert next(stream)[0] == datas[0]
    stream.close()

    def drain():  # every stream worker is single-threaded: a no-op queued behind its work
        for i in range(piece.STREAM_WORKERS):
            piece._pool(f"stream{i}").submit(lambda: None).result()

    drain()
    assert stub.running == 0
    started = _kinds(stub).count("decode")
    assert 1 <= started <= 2  # the pipeline keeps two windows in flight; the other four never start
    drain()
    assert _kinds(stub).count("decode") == started
    assert list(piece.reconstruct_data_stream_id_checked([], [], [])) == []
