"""GPU: the bit-sliced check kernel (sec_check_bs_kernel) under sec_check_batch and
sec_decode_check_batch, against expectations that never come from another HIP path.  Blocks =
cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c); corruptions are single flipped bytes put into
the buffer image in numpy, and what the check must report follows from where the test put them, as
in tests/test_gpu_check.py: a flip in a check row flags that row; a flip in a data block flags every
held check row (the code is MDS: no parity coefficient is zero); `first` is the lowest flipped
position and `column` the entries' bytes there.  With nothing lost, `out` of a decode + check is
the data blocks as held, in block order, cut at k*B - padlen.

Every case runs with SEC_CHECK_BS = 1 and = 0 and both are compared with the placement; under 1
the context's bit-sliced counter must rise by the eligible chunks.  Every chunk has padlen > 0 and
hands block k-1 over with block_avail = B - padlen, read in place: each entry sits in a buffer of
0xFF, so a read past an avail shows up as a difference, and the buffer must be byte-identical after
every call.  `out` is 0xFF-filled too and compared whole, guard bytes included."""

import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, DCHK_DTYPE  # noqa: E402
from storb_amd.engine import check_locate  # noqa: E402

UNTOUCHED = 0xEE  # row_bad / column before the call
SHAPES = [(10, 14), (8, 12), (16, 24), (32, 48), (64, 96), (8, 11)]
# one lane piece; a piece moved back to end at B; a wave span's edge; a workgroup's edge (4 spans);
# ragged ends
SIZES = [16, 17, 31, 2047, 2048, 2049, 4096 + 21, 8192 + 33]
PADLEN = 3


@functools.lru_cache(maxsize=None)
def _blocks(k, m, B, padlen, seed):
    """The oracle's m blocks of a seeded chunk of k*B - padlen bytes (block k-1 zero-padded)."""
    n = k * B - padlen
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes() + b"\0" * padlen
    blocks = cfec.easy_encode(data, k, m)
    assert len(blocks) == m and all(len(b) == B for b in blocks)
    return blocks


def spec(k, m, B, entries, flips=(), padlen=PADLEN, seed=None):
    """One chunk: blocks `entries` held, the first k the basis (and what a decode + check copies).
    flips: (entry position, byte position) of bytes XORed with 0x5A.  Block k-1, wherever it is
    among the entries, is handed over with block_avail = B - padlen."""
    assert len(set(entries)) == len(entries) >= k
    return dict(k=k, m=m, B=B, entries=list(entries), flips=list(flips), padlen=padlen,
                seed=seed if seed is not None else 1000 * k + m + B)


def flipped(s, *flips):
    return dict(s, flips=list(flips))


def eligible(s):
    k, e = s["k"], s["entries"]
    return (s["k"], s["m"]) in SHAPES and s["B"] >= 16 and len(e) > k and sorted(e[:k]) == list(range(k))


def _layout(specs):
    """The buffer image, both calls' arrays (offsets relative to the buffers), the expected image
    of `out` and, per chunk, what the check must report."""
    chk = np.zeros(len(specs), dtype=CHK_DTYPE)
    dchk = np.zeros(len(specs), dtype=DCHK_DTYPE)
    sn, bo, av, want, parts, outs = [], [], [], [], [], []
    cur, ocur = 3, 7
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        blocks = _blocks(k, s["m"], B, s["padlen"], s["seed"])
        held, avail = [], []
        for b in s["entries"]:
            a = B - s["padlen"] if b == k - 1 else B
            held.append(bytearray(blocks[b][:a]))
            avail.append(a)
        for e, p in s["flips"]:
            assert p < avail[e], "a flip must land on a byte that is in memory"
            held[e][p] ^= 0x5A
        chk[i] = (B, len(sn), n, k, s["m"], 0)
        dchk[i] = (ocur, B, s["padlen"], len(sn), n, k, s["m"], 0)
        if sorted(s["entries"][:k]) == list(range(k)):  # nothing lost: the data blocks as held
            by_num = {b: held[j] for j, b in enumerate(s["entries"][:k])}
            exp = b"".join(bytes(by_num[j]) for j in range(k))
        else:  # the oracle's decode of the first k entries as held
            exp = cfec.easy_decode([bytes(h) + b"\0" * (B - len(h)) for h in held[:k]], s["entries"][:k],
                                   s["padlen"], k, s["m"])
        assert len(exp) == k * B - s["padlen"]
        outs.append((ocur, exp))
        ocur += len(exp) + 9 + (i % 2)  # guard bytes between the chunks, odd and even starts
        for j in range(n):
            sn.append(s["entries"][j])
            bo.append(cur)
            av.append(avail[j])
            parts.append((cur, bytes(held[j])))
            cur += B + 5 + 2 * (j % 7)  # odd and even starts; what lies between stays 0xFF
        if s["flips"] and n > k:
            first = min(p for _, p in s["flips"])
            rows = set(range(k, n)) if any(e < k for e, _ in s["flips"]) else {e for e, _ in s["flips"]}
            column = bytes(held[j][first] if first < avail[j] else 0 for j in range(n))
            want.append((first, rows, column))
        else:
            want.append(None)
    src = np.full(cur + 64, 0xFF, np.uint8)
    for o, b in parts:
        src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    out = np.full(ocur + 64, 0xFF, np.uint8)
    for o, b in outs:
        out[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return SimpleNamespace(chk=chk, dchk=dchk, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), src=src, out=out, want=want, specs=specs,
                           eligible=sum(eligible(s) for s in specs),
                           direct=sum(not eligible(s) and len(s["entries"]) > s["k"] for s in specs))


def _verify(L, res, rb, col, what):
    res = np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=CHK_RESULT_DTYPE)
    for i, (s, w) in enumerate(zip(L.specs, L.want)):
        s0, n, k = int(L.chk[i]["slot0"]), len(s["entries"]), s["k"]
        tag = f"{what}, chunk {i}"
        if w is None:
            assert int(res[i]["first"]) == CHK_CONSISTENT and int(res[i]["nbad"]) == 0, f"{tag}: clean"
            assert not rb[s0:s0 + n].any(), f"{tag}: a flag on a clean chunk"
            assert (col[s0:s0 + n] == UNTOUCHED).all(), f"{tag}: column of a consistent chunk was written"
            continue
        first, rows, column = w
        assert int(res[i]["first"]) == first, f"{tag}: first {int(res[i]['first'])} != {first}"
        assert int(res[i]["nbad"]) == len(rows), f"{tag}: nbad"
        assert {j for j in range(n) if rb[s0 + j]} == rows and set(rb[s0:s0 + n].tolist()) <= {0, 1}, f"{tag}: row_bad"
        assert col[s0:s0 + n].tobytes() == column, f"{tag}: column"
        if n - k >= 2 and len({e for e, p in s["flips"] if p == first}) == 1:
            assert check_locate(k, s["m"], s["entries"], column) == next(e for e, p in s["flips"] if p == first), tag


def _call(engine, L, dsrc, decode):
    nslots = len(L.sn)
    res = torch.zeros(16 * len(L.specs), dtype=torch.uint8, device="cuda")
    rb = torch.full((nslots,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    col = torch.full((nslots,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    offs = L.bo + np.uint64(dsrc.data_ptr())
    dout = None
    if decode:
        dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
        engine.decode_check_batch(L.dchk, L.sn, offs, 0, dout, res, block_avail=L.av, row_bad=rb, column=col)
    else:
        engine.check_batch(L.chk, L.sn, offs, 0, res, block_avail=L.av, row_bad=rb, column=col)
    return res.cpu().numpy(), rb.cpu().numpy(), col.cpu().numpy(), None if dout is None else dout.cpu().numpy()


def run_three(engine, specs):
    """check and decode + check with SEC_CHECK_BS = 1 and = 0, each against the placement."""
    L = _layout(specs)
    dsrc = torch.from_numpy(L.src).cuda()
    got = {}
    for opt in (1, 0):
        with engine.options(SEC_CHECK_BS=opt):
            for decode in (False, True):
                what = f"SEC_CHECK_BS={opt} {'decode + check' if decode else 'check'}"
                b0, d0 = engine.check_methods()
                res, rb, col, out = _call(engine, L, dsrc, decode)
                b1, d1 = engine.check_methods()
                assert (b1 - b0, d1 - d0) == ((L.eligible, L.direct) if opt else (0, L.eligible + L.direct)), what
                _verify(L, res, rb, col, what)
                if decode:
                    d = np.flatnonzero(out != L.out)
                    assert d.size == 0, f"{what}: out differs at {d[:8].tolist()} ({d.size} bytes)"
                got[(opt, decode)] = (res.tobytes(), rb.tobytes(), col.tobytes())
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    assert len(set(got.values())) == 1, "the four calls disagree"
    return L


def _shuffled(k, m, B, nrows=None):
    rng = random.Random(k * 100003 + m * 101 + B)
    basis = rng.sample(range(k), k)
    rows = rng.sample(range(k, m), m - k if nrows is None else nrows)
    return basis + rows


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("k,m", SHAPES)
def test_shapes_and_sizes(engine, k, m, B):
    """Clean; one flipped byte in a parity piece at 0, B-1, 2047 / 2048 where B allows and in the
    overlap of the moved-back last piece; one in a data piece (every held row bad); two flips in
    different pieces at different positions (`first` the lower).  Basis and rows shuffled, every
    parity row held."""
    s = spec(k, m, B, _shuffled(k, m, B))
    n = m
    at = [0, B - 1] + [p for p in (2047, 2048) if p < B]
    if B % 16:  # the last unclamped piece's last byte: the piece moved back to end at B holds it too
        at.append(B // 16 * 16 - 1)
    cases = [s] + [flipped(s, (k + i % (n - k), p)) for i, p in enumerate(at)]
    not_last = next(j for j in range(k) if s["entries"][j] != k - 1)
    last = s["entries"].index(k - 1)
    cases.append(flipped(s, (not_last, B // 2)))
    cases.append(flipped(s, (last, B - PADLEN - 1)))  # block k-1's last byte in memory
    cases.append(flipped(s, (k, B - 2), (k + 1, 5)))
    cases.append(flipped(s, (n - 1, B - 1), (not_last, 7)))
    L = run_three(engine, cases)
    assert L.eligible == len(cases)


def test_parity_subsets(engine):
    """zfec(64,96) with rows held only in group 0, only in group 1 and in both; zfec(16,24) with 3 of
    its 8 rows, in shuffled entry order; one row only."""
    B = 4096 + 21
    rng = random.Random(96)
    basis = rng.sample(range(64), 64)
    g0 = rng.sample(range(64, 80), 5)
    g1 = rng.sample(range(80, 96), 7)
    both = rng.sample(range(64, 96), 9)
    assert any(r < 80 for r in both) and any(r >= 80 for r in both)
    cases = []
    for rows in (g0, g1, both, [95]):
        s = spec(64, 96, B, basis + rows)
        cases += [s, flipped(s, (64 + len(rows) - 1, B - 1)), flipped(s, (17, 2048))]
        if len(rows) > 1:
            cases.append(flipped(s, (64, 4096), (65, 4095)))
    s = spec(16, 24, B, _shuffled(16, 24, B, 3))
    cases += [s, flipped(s, (18, 0)), flipped(s, (16, B - 1), (17, B - 2)), flipped(s, (3, 100))]
    L = run_three(engine, cases)
    assert L.eligible == len(cases)


def test_one_mixed_call(engine):
    """An eligible (16,24) chunk, one whose basis holds a parity row, a (4,6) chunk and an n == k
    chunk in one call: all four right, the counters move by (1, 2), one timed launch unit."""
    B = 4096 + 21
    a = spec(16, 24, B, _shuffled(16, 24, B))
    lost = [s for s in range(24) if s not in (2, 9)]  # primaries 2 and 9 lost: rows 16, 17 stand in
    b = spec(16, 24, B, lost[:16] + lost[16:])
    c = spec(4, 6, B, [5, 0, 3, 2, 4, 1])
    d = spec(16, 24, B, list(range(16)))
    for specs in ([a, b, c, d], [flipped(a, (20, 4097)), flipped(b, (17, 33)), flipped(c, (4, B - 1)), d],
                  [flipped(a, (5, 2047)), flipped(b, (1, 0)), c, flipped(d, (0, 0))]):
        L = run_three(engine, specs)
        assert (L.eligible, L.direct) == (1, 2)
    L = _layout([a, b, c, d])
    dsrc = torch.from_numpy(L.src).cuda()
    engine.set_timing(True)
    try:
        with engine.options(SEC_CHECK_BS=1):
            for decode, kind in ((False, "check"), (True, "decode_check")):
                engine.collect_timing(kind)
                b0 = engine.check_methods()
                _call(engine, L, dsrc, decode)
                ms, launches = engine.collect_timing(kind)
                assert launches == 1 and ms > 0, kind
                b1 = engine.check_methods()
                assert (b1[0] - b0[0], b1[1] - b0[1]) == (1, 2)
    finally:
        engine.set_timing(False)


def _host_item(s, decode):
    k, B = s["k"], s["B"]
    blocks = _blocks(k, s["m"], B, s["padlen"], s["seed"])
    held = [bytearray(blocks[b]) for b in s["entries"]]
    for e, p in s["flips"]:
        held[e][p] ^= 0x5A
    it = (k, s["m"], [bytes(h) for h in held], s["entries"])
    return it + (s["padlen"],) if decode else it


def test_host_mode_on_a_wide_case(engine):
    """decode_check_host and check_host (staged: every entry B long) on zfec(32,48)."""
    B = 4096 + 21
    s = spec(32, 48, B, _shuffled(32, 48, B))
    specs = [s, flipped(s, (40, B - 1)), flipped(s, (3, 2048))]
    for opt in (1, 0):
        with engine.options(SEC_CHECK_BS=opt):
            b0 = engine.check_methods()
            data, checks = engine.decode_check_host([_host_item(x, True) for x in specs])
            plain = engine.check_host([_host_item(x, False) for x in specs])
            b1 = engine.check_methods()
        assert (b1[0] - b0[0], b1[1] - b0[1]) == ((6, 0) if opt else (0, 6))
        want = b""
        for x in specs:
            it = _host_item(x, True)
            by_num = dict(zip(it[3][:32], it[2][:32]))
            want += b"".join(by_num[j] for j in range(32))[:32 * B - PADLEN]
        assert data == want
        assert checks == plain
        assert checks[0] == (None, [], None)
        assert checks[1][:2] == (B - 1, [40]) and checks[2][:2] == (2048, list(range(32, 48)))
        assert check_locate(32, 48, s["entries"], checks[2][2]) == 3


def _encoded(k, m, n, chunk_idx, seed):
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    pieces = [piece.Piece(chunk_idx=chunk_idx, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks)]
    return piece.EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=k * B - n,
                              original_chunk_size=n), data


def _flip(pieces, chunk_idx, piece_idx, offset):
    for p in pieces:
        if (p.chunk_idx, p.piece_idx) == (chunk_idx, piece_idx):
            b = bytearray(p.data)
            b[offset] ^= 0x5A
            p.data = bytes(b)
            return
    raise AssertionError("piece not held")


def test_decode_chunks_checked_end_to_end():
    """A (32,48) chunk with every piece held and one corrupt parity piece: located, the bytes right,
    and the first pass went down the bit-sliced path (choose_blocks picked the data pieces)."""
    eng = piece.get_engine()
    ec, data = _encoded(32, 48, 32 * 5000 - 11, 4, 3248)
    _flip(ec.pieces, 4, 41, 4999)
    with eng.options(SEC_CHECK_BS=1):
        b0 = eng.check_methods()
        got, checks = piece.decode_chunks_checked([ec])
        b1 = eng.check_methods()
    assert got == data
    ck = checks[0]
    assert (ck.checked, ck.consistent, ck.first_bad_offset, ck.bad_piece_idx, ck.located) == (48, False, 4999, [41], True)
    assert b1[0] - b0[0] == 2 and b1[1] == b0[1]  # the fused pass and the re-check without piece 41


def test_stream_checked_three_windows():
    """Three windows of two (16,24) chunks, one corrupt piece in the second window: the bytes
    against the oracle's input, the checks as placed."""
    n = 16 * 3000 - 5
    made = [_encoded(16, 24, n, i, 1624 + i) for i in range(6)]
    pieces = [p for ec, _ in made for p in ec.pieces]
    random.Random(7).shuffle(pieces)
    _flip(pieces, 3, 6, 1234)  # a data piece of the second window's second chunk
    chunks = [ec for ec, _ in made]
    for ec in chunks:
        ec.pieces = []
    got = list(piece.reconstruct_data_stream_checked(pieces, chunks, window_bytes=2 * n))
    assert [d for d, _ in got] == [d for _, d in made]
    assert [(c.chunk_idx, c.checked, c.consistent, c.first_bad_offset, c.bad_piece_idx, c.located) for _, c in got] == [
        (i, 24, i != 3, 1234 if i == 3 else None, [6] if i == 3 else [], i == 3) for i in range(6)]
