"""CPU: the ``max_errors`` keyword of piece.decode_chunks_corrected, reconstruct_data_corrected,
reconstruct_data_stream_corrected, repair_chunks_corrected and repair_pieces_corrected: what reaches
the engine, the unchanged default, the counting of several pieces changed at one offset, and the
symbols and wrappers behind it.  The engine is the stand-in of tests/test_decode_correct_piece_api.py
and tests/test_repair_correct_piece_api.py (round one on the oracle) with correcting calls that take
``max_errors`` and judge every column with engine.check_correct (host arithmetic, itself tied to
brute force in tests/test_check_correct.py); the GPU path is tests/test_gpu_correct_multi.py's."""

import ctypes
import inspect

import numpy as np
import pytest

from oracle import cfec
from storb_amd import _lib, piece
from storb_amd.engine import Engine, check_correct
from tests import test_decode_correct_piece_api as dec_api
from tests import test_repair_correct_piece_api as rep_api
from tests.test_decode_correct_piece_api import _chunk, _corrupt


def _judge(k, m, blocks, sharenums, max_errors):
    """Every column through check_correct -> (corrected basis blocks, (first, first_open, corrected,
    open, hits))."""
    n, B = len(blocks), len(blocks[0])
    fixed_rows = [bytearray(b) for b in blocks]
    hits, bad, opened, ncor = [0] * n, [], [], 0
    for p in range(B):
        col = bytes(b[p] for b in blocks)
        fixed, changed = check_correct(k, m, sharenums, col, max_errors)
        if changed == 0:
            continue
        bad.append(p)
        if changed < 0:
            opened.append(p)
            continue
        ncor += 1
        for j in range(n):
            if fixed[j] != col[j]:
                hits[j] += 1
                fixed_rows[j][p] = fixed[j]
    return ([bytes(r) for r in fixed_rows[:k]],
            (bad[0] if bad else None, opened[0] if opened else None, ncor, len(opened), hits))


class StandIn(dec_api.StandInEngine, rep_api.StandInEngine):
    """Both stand-ins' round-one calls; the correcting calls take max_errors and record it."""

    def decode_correct_host(self, items, **kw):
        self.calls.append(("decode_correct", items, kw))
        data, out = b"", []
        for k, m, blocks, sharenums, padlen in items:
            basis, found = _judge(k, m, blocks, sharenums, kw.get("max_errors", 1))
            data += cfec.easy_decode(basis, list(sharenums[:k]), padlen, k, m)
            out.append(found)
        return data, out

    def repair_correct_host(self, items, digests=False, **kw):
        self.calls.append(("repair_correct", items, kw))
        out, cor = [], []
        for k, m, blocks, sharenums, targets in items:
            basis, found = _judge(k, m, blocks, sharenums, kw.get("max_errors", 1))
            full = rep_api._code_word(k, m, basis, sharenums)
            out.append([full[t] for t in targets])
            cor.append(found)
        return self._with_digests(out, digests, (cor,))


@pytest.fixture
def stub(monkeypatch):
    eng = StandIn()
    monkeypatch.setattr(piece, "get_engine", lambda device=None: eng)
    return eng


def _two_at_one_offset(ci=0):
    """zfec(16,24), every piece held, pieces 2 and 19 damaged at the same two offsets; piece 7 alone
    at a third."""
    ec, data = _chunk(16, 24, 16 * 48 - 5, ci, 70 + ci)
    for at in (10, 40):
        _corrupt(ec, 2, at, 0x01)
        _corrupt(ec, 19, at, 0x80)
    _corrupt(ec, 7, 20)
    return ec, data


def test_the_default_passes_no_keyword_and_leaves_both_offsets_open(stub):
    ec, data = _two_at_one_offset()
    got, (ck,) = piece.decode_chunks_corrected([ec])
    assert [c[0] for c in stub.calls] == ["decode_check", "decode_correct"] and stub.calls[1][2] == {}
    assert (ck.corrected_positions, ck.open_positions, ck.first_open_offset, ck.damaged) == (1, 2, 10, {7: 1})
    assert got != data
    stub.calls.clear()
    _, (ck1,) = piece.decode_chunks_corrected([ec], max_errors=1)  # spelled out: the same call
    assert stub.calls[1][2] == {} and ck1 == ck
    with pytest.raises(piece.PieceCorrectionError, match="one piece per offset"):
        piece.reconstruct_data_corrected(list(ec.pieces), [ec])


@pytest.mark.parametrize("max_errors,kw", [(None, {"max_errors": 0}), (2, {"max_errors": 2}), (4, {"max_errors": 4})])
def test_several_pieces_per_offset(stub, max_errors, kw):
    ec, data = _two_at_one_offset()
    got, (ck,) = piece.decode_chunks_corrected([ec], max_errors=max_errors)
    assert got == data and stub.calls[1][2] == kw
    # an offset with two pieces changed counts once in corrected_positions and once per piece in damaged
    assert ck == piece.ChunkCorrection(chunk_idx=0, checked=24, consistent=False, first_bad_offset=10,
                                       corrected_positions=3, open_positions=0, first_open_offset=None,
                                       damaged={2: 2, 7: 1, 19: 2})
    assert piece.reconstruct_data_corrected(list(ec.pieces), [ec], max_errors=max_errors)[0] == data
    streamed = list(piece.reconstruct_data_stream_corrected(list(ec.pieces), [ec], max_errors=max_errors))
    assert [d for d, _ in streamed] == [data] and streamed[0][1] == ck


def test_clean_input_launches_round_one_alone_whatever_the_keyword(stub):
    ec, data = _chunk(16, 24, 16 * 48, 0, 5)
    assert piece.decode_chunks_corrected([ec], max_errors=None)[0] == data
    assert piece.repair_chunks_corrected([ec], max_errors=None)[0] == [[]]
    assert [c[0] for c in stub.calls] == ["decode_check", "repair_check"]


def test_repair_heals_both_pieces(stub):
    ec, _ = _two_at_one_offset()
    clean, _ = _chunk(16, 24, 16 * 48 - 5, 0, 70)
    want = {p.piece_idx: p.data for p in clean.pieces}
    ec.pieces = [p for p in ec.pieces if p.piece_idx != 23]  # one piece lost as well: 23 held, r = 7
    pieces, ck = piece.repair_pieces_corrected(ec, max_errors=None)
    assert stub.calls[1][0] == "repair_correct" and stub.calls[1][2] == {"max_errors": 0}
    assert [p.piece_idx for p in pieces] == [23, 2, 7, 19] and all(p.data == want[p.piece_idx] for p in pieces)
    assert (ck.corrected_positions, ck.open_positions, ck.damaged) == (3, 0, {2: 2, 7: 1, 19: 2})
    stub.calls.clear()
    pieces, ck = piece.repair_pieces_corrected(ec)  # the default: no keyword, both offsets open
    assert stub.calls[1][2] == {} and (ck.open_positions, ck.damaged) == (2, {7: 1})
    assert [p.piece_idx for p in pieces] == [23, 7]
    (pieces,), (ck,) = piece.repair_chunks_corrected([ec], max_errors=2, piece_ids=True)
    assert stub.calls[-1][2] == {"max_errors": 2} and ck.open_positions == 0
    assert [p.piece_idx for p in pieces] == [23, 2, 7, 19]


def test_three_at_one_offset_with_a_bound_of_two_is_open(stub):
    ec, data = _two_at_one_offset()
    _corrupt(ec, 5, 10, 0x33)
    _, (ck,) = piece.decode_chunks_corrected([ec], max_errors=2)
    assert (ck.open_positions, ck.first_open_offset, ck.corrected_positions) == (1, 10, 2)
    with pytest.raises(piece.PieceCorrectionError, match="pieces correctable per offset"):
        piece.reconstruct_data_corrected(list(ec.pieces), [ec], max_errors=2)
    assert piece.decode_chunks_corrected([ec], max_errors=None)[0] == data  # the code's limit is 4


@pytest.mark.parametrize("bad", [0, -1])
def test_a_bound_below_one_is_refused(stub, bad):
    ec, _ = _chunk(4, 6, 40, 0, 1)
    for call in (lambda: piece.decode_chunks_corrected([ec], max_errors=bad),
                 lambda: piece.repair_chunks_corrected([ec], max_errors=bad),
                 lambda: list(piece.reconstruct_data_stream_corrected(list(ec.pieces), [ec], max_errors=bad))):
        with pytest.raises(ValueError, match="max_errors"):
            call()
    assert stub.calls == []


def test_symbols_and_signatures():
    lib = _lib.load()
    for name in ("sec_decode_correct_ex_batch", "sec_repair_correct_ex_batch", "sec_check_correct"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.sec_abi_version() == 1  # additions only
    for op in ("decode", "repair"):  # the namesake's arguments with max_errors in front of the flags
        old, new = _lib._SIGS[f"sec_{op}_correct_batch"][1], _lib._SIGS[f"sec_{op}_correct_ex_batch"][1]
        assert new == old[:-1] + [ctypes.c_int, ctypes.c_uint]
    for fn in (Engine.decode_correct_batch, Engine.decode_correct_host, Engine.repair_correct_batch,
               Engine.repair_correct_host):
        assert inspect.signature(fn).parameters["max_errors"].default == 1
    for fn in (piece.decode_chunks_corrected, piece.reconstruct_data_corrected, piece.reconstruct_data_stream_corrected,
               piece.repair_chunks_corrected, piece.repair_pieces_corrected):
        p = inspect.signature(fn).parameters["max_errors"]
        assert p.default == 1 and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_null_context_is_einval():
    """Without a device there is no context, so this checks the NULL context only: SEC_EINVAL whatever
    max_errors and the flags are.  That max_errors < 0, SEC_F_RECOVER and SEC_F_HOST | SEC_F_ASYNC are
    refused on their own, and the error order, is tests/test_gpu_correct_multi.py's
    test_errors_before_any_device_work, which has a context.  sec_check_correct needs none: its
    max_errors < 0 is checked here."""
    lib = _lib.load()
    d = np.zeros(1, dtype=_lib.DCHK_DTYPE)
    d[0] = (0, 64, 0, 0, 6, 4, 6, 0)
    r = np.zeros(1, dtype=_lib.RCHK_DTYPE)
    r[0] = (64, 0, 0, 1, 5, 4, 6)
    sn, bo = np.arange(6, dtype=np.int32), np.zeros(6, np.uint64)
    res = np.zeros(1, dtype=_lib.COR_RESULT_DTYPE)
    out = np.zeros(512, np.uint8)
    tn, to = np.array([5], np.int32), np.zeros(1, np.uint64)
    for T, flags in ((0, 0), (-1, 0), (0, _lib.SEC_F_RECOVER), (0, _lib.SEC_F_HOST | _lib.SEC_F_ASYNC)):
        assert lib.sec_decode_correct_ex_batch(None, d.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                               out.ctypes.data, res.ctypes.data, None, T, flags) == _lib.SEC_EINVAL
        assert lib.sec_repair_correct_ex_batch(None, r.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                               tn.ctypes.data, to.ctypes.data, out.ctypes.data, None, res.ctypes.data,
                                               None, T, flags) == _lib.SEC_EINVAL
    ch = ctypes.c_int32(0)
    assert lib.sec_check_correct(4, 6, sn.ctypes.data, 6, out.ctypes.data, -1, out.ctypes.data + 8,
                                 ctypes.byref(ch)) == _lib.SEC_EINVAL
