"""GPU: piece.reconstruct_data_id_checked and its stream form on the device, with each hashing method
(the SHA-1 kernel through Engine.sha1_host, and hashlib on the thread pool).  Pieces =
cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c), recorded ids = hashlib.sha1 of them; junk
pieces are noise put in here, and the expected bytes are the chunks themselves."""

import hashlib

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import piece  # noqa: E402
from storb_amd.engine import pinned_bytes  # noqa: E402


def _object(junk):
    """Three 64 KiB RS(4,6) chunks with every piece held: (chunks, datas, recorded ids as hex).  junk:
    (chunk, piece) pairs whose held bytes are replaced by noise."""
    n, k, m = 64 << 10, 4, 6
    B = -(-n // k)
    datas, chunks, ids = [], [], []
    for ci in range(3):
        data = np.random.default_rng(700 + ci).integers(0, 256, n - ci, dtype=np.uint8).tobytes()
        blocks = cfec.easy_encode(data, k, m)
        ids.append([hashlib.sha1(b).hexdigest() for b in blocks])
        held = [np.random.default_rng(ci * 10 + i).integers(0, 256, B, dtype=np.uint8).tobytes() if (ci, i) in junk else b
                for i, b in enumerate(blocks)]
        pieces = [piece.Piece(chunk_idx=ci, piece_idx=i, data=b,
                              piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
                  for i, b in enumerate(held)]
        chunks.append(piece.EncodedChunk(pieces=pieces, chunk_idx=ci, k=k, m=m, chunk_size=B,
                                         padlen=k * B - len(data), original_chunk_size=len(data)))
        datas.append(data)
    return chunks, datas, ids


@pytest.mark.parametrize("on_gpu", [False, True], ids=["pool-ids", "gpu-ids"])
@pytest.mark.parametrize("junk,bad", [({(1, 5)}, [[], [5], []]), ({(1, 2), (2, 4)}, [[], [2], [4]]),
                                      ({(0, 0), (0, 3)}, [[0, 3], [], []])],
                         ids=["junk-parity", "junk-data", "two-junk-data"])
def test_piece_api_end_to_end(monkeypatch, on_gpu, junk, bad):
    """A junk parity piece leaves the bytes alone; junk data pieces are named and not decoded from
    (the chunk is recovered from the good pieces on the GPU), and the bytes equal the original."""
    monkeypatch.setattr(piece, "_ids_on_gpu", lambda npieces, piece_bytes: on_gpu)
    chunks, datas, ids = _object(junk)
    pieces = [p for ch in chunks for p in ch.pieces]
    got, checks = piece.reconstruct_data_id_checked(pieces, chunks, ids)
    assert got == b"".join(datas)
    assert [(c.checked, c.ok, c.bad_piece_idx, c.decodable) for c in checks] == [(6, not b, b, True) for b in bad]
    for ch in chunks:
        ch.pieces = []
    pairs = list(piece.reconstruct_data_stream_id_checked(pieces, chunks, ids, window_bytes=100 << 10))  # 1 + 1 + 1
    assert [d for d, _ in pairs] == datas and [c for _, c in pairs] == checks
    assert pinned_bytes()[0] == 0


@pytest.mark.parametrize("on_gpu", [False, True], ids=["pool-ids", "gpu-ids"])
def test_fewer_than_k_good_pieces(monkeypatch, on_gpu):
    monkeypatch.setattr(piece, "_ids_on_gpu", lambda npieces, piece_bytes: on_gpu)
    chunks, datas, ids = _object({(2, 0), (2, 3), (2, 5)})
    pieces = [p for ch in chunks for p in ch.pieces]
    with pytest.raises(piece.PieceIdError) as e:
        piece.reconstruct_data_id_checked(pieces, chunks, ids)
    assert [(c.chunk_idx, c.decodable, c.bad_piece_idx) for c in e.value.checks] == [
        (0, True, []), (1, True, []), (2, False, [0, 3, 5])]
    got = []
    with pytest.raises(piece.PieceIdError):
        for pair in piece.reconstruct_data_stream_id_checked(pieces, chunks, ids, window_bytes=1):
            got.append(pair)
    assert [d for d, _ in got] == datas[:2]
