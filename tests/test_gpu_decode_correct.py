"""GPU: sec_decode_correct_batch against expectations that never come from the code under test.
Blocks = cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c); damage is bytes XORed into the buffer
image in numpy at places the test chose.  So the expected output is the ORIGINAL chunk wherever a
position carries at most one damaged entry (and the chunk has two check rows or more), the expected
hits are the flips the test put into each entry, and the expected open positions are those where it
put two (in shapes with n - k >= 3) or any (n - k == 1); there `out` is cfec.easy_decode of the
basis as held.  A second witness: engine.check_locate (host arithmetic) on the damaged columns must
name the entry the call counted.

Layout of every case as in tests/test_gpu_decode_check.py: each entry sits in a buffer of 0xFF at
odd and even starts, so a short entry (block_avail < B) is followed by 0xFF bytes and a read past
its avail shows up as a difference; the buffer must be byte-identical after every call.  `out` is
0xFF-filled too, every chunk's bytes at an odd or even start with guard bytes around them, and is
compared whole."""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, COR_RESULT_DTYPE, DCHK_DTYPE  # noqa: E402
from storb_amd.engine import Engine, Error, check_locate, get_engine, pinned_bytes  # noqa: E402

UNTOUCHED = 0xEEEEEEEE  # entry_hits before the call
WITNESSED = 48  # damaged columns per chunk put before check_locate


@functools.lru_cache(maxsize=None)
def _chunk(k, m, B, padlen, seed):
    """A seeded chunk of k*B - padlen bytes and the oracle's m blocks of it."""
    n = k * B - padlen
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    blocks = cfec.easy_encode(data + b"\0" * padlen, k, m)
    assert len(blocks) == m and all(len(b) == B for b in blocks)
    return data, blocks


def spec(k, m, B, entries, flips=(), padlen=0, short=False, seed=None):
    """One chunk: blocks `entries` held, the first k the basis, the rest the check rows.  flips:
    (entry position, byte position[, xor value, default 0x5A]).  short: block k-1, wherever it is
    among the entries, is handed over with block_avail = B - padlen."""
    assert len(set(entries)) == len(entries) >= k
    flips = [(f[0], f[1], f[2] if len(f) > 2 else 0x5A) for f in flips]
    assert len({(e, p) for e, p, _ in flips}) == len(flips) and all(v for _, _, v in flips)
    return dict(k=k, m=m, B=B, entries=list(entries), flips=flips, padlen=padlen, short=short,
                seed=seed if seed is not None else 1000 * k + m + B)


def flipped(s, *flips):
    return spec(s["k"], s["m"], s["B"], s["entries"], flips, s["padlen"], s["short"], s["seed"])


def _held(s):
    k, B = s["k"], s["B"]
    _, blocks = _chunk(k, s["m"], B, s["padlen"], s["seed"])
    held, avail = [], []
    for b in s["entries"]:
        a = B - s["padlen"] if s["short"] and b == k - 1 else B
        held.append(bytearray(blocks[b][:a]))
        avail.append(a)
    for e, p, v in s["flips"]:
        assert p < avail[e], "a flip must land on a byte that is in memory"
        held[e][p] ^= v
    return held, avail


def _expect(s, held):
    """(out bytes, first, first_open, corrected, open, hits per entry, {position: entry or -2})."""
    k, B, n = s["k"], s["B"], len(s["entries"])
    data, _ = _chunk(k, s["m"], B, s["padlen"], s["seed"])
    nr = n - k
    at = {}
    for e, p, _ in s["flips"]:
        at.setdefault(p, []).append(e)
    basis = [bytes(h) + b"\0" * (B - len(h)) for h in held[:k]]
    as_held = cfec.easy_decode(basis, s["entries"][:k], s["padlen"], k, s["m"])
    if nr == 0:  # nothing to check: a plain decode, consistent whatever the bytes
        return as_held, None, None, 0, 0, [0] * n, {}
    exp = bytearray(data)
    hits, verdict, opened = [0] * n, {}, []
    for p, es in sorted(at.items()):
        if nr >= 2 and len(es) == 1:
            hits[es[0]] += 1
            verdict[p] = es[0]
            continue
        assert nr == 1 or nr >= 3, "two flips at one position of a distance-3 code prove nothing"
        opened.append(p)
        verdict[p] = -2
        for row in range(k):
            if row * B + p < len(exp):
                exp[row * B + p] = as_held[row * B + p]
    return (bytes(exp), min(at) if at else None, min(opened) if opened else None, sum(hits), len(opened), hits,
            verdict)


def _layout(specs):
    descs = np.zeros(len(specs), dtype=DCHK_DTYPE)
    sn, bo, av, want, parts, outs = [], [], [], [], [], []
    cur, ocur = 3, 7
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        held, avail = _held(s)
        descs[i] = (ocur, B, s["padlen"], len(sn), n, k, s["m"], 0)
        w = _expect(s, held)
        columns = {p: bytes(held[j][p] if p < avail[j] else 0 for j in range(n)) for p in w[6]}
        want.append(w[1:] + (columns,))
        outs.append((ocur, w[0]))
        ocur += len(w[0]) + 9 + (i % 2)  # guard bytes between the chunks, odd and even starts
        for j in range(n):
            sn.append(s["entries"][j])
            bo.append(cur)
            av.append(avail[j])
            parts.append((cur, bytes(held[j])))
            cur += B + 5 + 2 * j  # odd and even starts; what lies between stays 0xFF
    src = np.full(cur + 64, 0xFF, np.uint8)
    for o, b in parts:
        src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    out = np.full(ocur + 64, 0xFF, np.uint8)
    for o, b in outs:
        out[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return SimpleNamespace(descs=descs, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), src=src, out=out, want=want, specs=specs)


def _opt(v):
    return None if int(v) == CHK_CONSISTENT else int(v)


def _verify(L, res, hits):
    res = np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=COR_RESULT_DTYPE)
    for i, (s, w) in enumerate(zip(L.specs, L.want)):
        first, first_open, corrected, opened, want_hits, verdict, columns = w
        s0, n = int(L.descs[i]["slot0"]), len(s["entries"])
        got = (_opt(res[i]["first"]), _opt(res[i]["first_open"]), int(res[i]["corrected"]), int(res[i]["open"]))
        assert got == (first, first_open, corrected, opened), f"chunk {i}: {got}"
        if hits is not None:
            assert hits[s0:s0 + n].tolist() == want_hits, f"chunk {i}: hits"
        for p in sorted(verdict)[:WITNESSED]:  # the host rule names the entry the test damaged
            assert check_locate(s["k"], s["m"], s["entries"], columns[p]) == verdict[p], f"chunk {i}: position {p}"


def _out_diff(got, want):
    d = np.flatnonzero(got != want)
    return f"out differs at {d[:8].tolist()} ({d.size} bytes)" if d.size else ""


def run_device(engine, L, dsrc=None, asynchronous=False, use_avail=True, with_hits=True):
    if dsrc is None:
        dsrc = torch.from_numpy(L.src).cuda()
    dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
    res = torch.zeros(24 * len(L.specs), dtype=torch.uint8, device="cuda")
    hits = torch.from_numpy(np.full(len(L.sn), UNTOUCHED, np.uint32).view(np.int32)).cuda() if with_hits else None
    engine.decode_correct_batch(L.descs, L.sn, L.bo + np.uint64(dsrc.data_ptr()), 0, dout, res,
                                block_avail=L.av if use_avail else None, entry_hits=hits, asynchronous=asynchronous)
    if asynchronous:
        engine.sync()
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    assert not _out_diff(dout.cpu().numpy(), L.out)
    _verify(L, res.cpu().numpy(), hits.cpu().numpy().view(np.uint32) if with_hits else None)
    return dsrc


def run_host(eng, L):
    src = L.src.copy()
    out = np.full(L.out.size, 0xFF, np.uint8)
    res = np.zeros(len(L.specs), dtype=COR_RESULT_DTYPE)
    hits = np.full(len(L.sn), UNTOUCHED, np.uint32)
    eng.decode_correct_batch(L.descs, L.sn, L.bo, src, out, res, block_avail=L.av, entry_hits=hits, host=True)
    assert np.array_equal(src, L.src), "the source buffer was written"
    assert not _out_diff(out, L.out)
    _verify(L, res, hits)


def run_both(engine, specs, **kw):
    L = _layout(specs)
    run_device(engine, L, **kw)
    run_host(engine, L)


# RS(4,6) from blocks {5, 0, 3, 2}: primary 1 is lost (e = 1) and is also a check row; the other is 4
E46 = [5, 0, 3, 2, 4, 1]
E46_ALL = [0, 1, 2, 3, 4, 5]  # e = 0: copies and two check rows


def _edges(B):
    """Position 0, B - 1, and both sides of every boundary the kernel has: its 16-position lanes,
    its 4096-position tiles, and the last whole lane's end (where the byte-wise lane takes over)."""
    whole = B // 16 * 16
    return sorted({p for p in (0, B - 1, 15, 16, 31, 32, 4095, 4096, whole - 1, whole) if 0 <= p < B})


@pytest.mark.parametrize("entries", [E46, E46_ALL], ids=["e1", "e0"])
@pytest.mark.parametrize("B", [1, 5, 15, 16, 17, 63, 257, 4099])
def test_block_sizes(engine, B, entries):
    """The tail kernel only (B < 16), exactly one lane, a straddling lane, several lanes, a second
    tile.  Clean; flips in a check row only; in a present-primary basis entry; in the basis entry
    that is a parity block (e1) or primary 0 (e0); in two different entries at different positions."""
    s = spec(4, 6, B, entries)
    ps = _edges(B)
    two = [(q % 2 * 5, p, 1 + (p % 255)) for q, p in enumerate(ps)]  # entries 0 and 5 in turn
    run_both(engine, [s, flipped(s, *[(4, p) for p in ps]), flipped(s, *[(2, p, 0xFF) for p in ps]),
                      flipped(s, *[(0, p, 0x01) for p in ps]), flipped(s, *two)], use_avail=False)


Z1014_SHORT = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 9, 8, 4, 12, 10], padlen=4, short=True)  # e = 2, nr = 2
Z1014_ALL = spec(10, 14, 6554, [3, 0, 9, 1, 7, 5, 6, 2, 8, 4, 12, 10, 13, 11], padlen=4, short=True)  # nr = 4


def test_short_block(engine):
    """zfec(10,14), B = 6554, padlen 4, block 9 handed over with avail = B - 4 (0xFF behind it).  A
    flip at avail - 1 of the short entry, and flips of full entries in the ragged end behind it."""
    short_at = Z1014_SHORT["entries"].index(9)
    run_both(engine, [Z1014_SHORT, flipped(Z1014_SHORT, (short_at, 6549)),
                      flipped(Z1014_SHORT, (1, 6553), (11, 6551), (short_at, 0), (0, 6550, 0x80))])


_P16 = [s for s in range(16) if s not in (0, 5)]
Z1624 = spec(16, 24, 259, _P16[::-1] + [19, 16] + [23, 17, 20, 18, 22, 21])  # e = 2, six check rows


def test_recovered_and_copied_rows(engine):
    """zfec(16,24), B = 259, data pieces 0 and 5 absent: flips in a basis parity row and in a present
    primary; both recovered rows and the copied row must come out right."""
    run_both(engine, [Z1624, flipped(Z1624, (14, 7), (14, 258), (3, 100), (3, 255), (15, 256, 0x11), (20, 8))])


_B32 = [40, 33] + [s for s in range(32) if s not in (0, 13)][::-1]
Z3248 = spec(32, 48, 130, _B32 + [0, 13] + [s for s in range(32, 48) if s not in (40, 33)])  # all 48 held, nr = 16
_B64 = list(range(1, 64)) + [64]
Z6496 = spec(64, 96, 33, _B64 + list(range(65, 81)))  # data piece 0 absent, 80 held: e = 1, nr = 16


def test_row_groups(engine):
    """More than one group of check rows (nr = 16), over k = 32 with e = 2 and over k = 64 with
    e = 1: flips in a check row of the second group, in basis entries, in the ragged end."""
    run_both(engine, [Z3248, flipped(Z3248, (32 + 12, 5), (0, 64), (31, 129), (17, 128, 0xC3)),
                      Z6496, flipped(Z6496, (63, 0), (64 + 15, 31), (5, 32, 0x02), (40, 16))])


def test_two_errors_at_one_position_are_open(engine):
    """zfec(10,14) with all 14 held (distance 5): two flips at one position are reported open and
    left as held, another position with one flip is corrected."""
    s = flipped(Z1014_ALL, (2, 3000), (12, 3000, 0x21), (7, 41))
    L = _layout([s])
    assert L.want[0][:4] == (41, 3000, 1, 1)
    run_device(engine, L)
    run_host(engine, L)
    run_both(engine, [flipped(Z1014_ALL, (0, 6553), (1, 6553, 0x03), (13, 6552))])  # in the ragged end


def test_one_check_row_corrects_nothing(engine):
    """n - k = 1 (RS(4,6) with five held): every damaged position is open and corrected == 0."""
    s = spec(4, 6, 257, [5, 0, 3, 2, 1])
    L = _layout([s, flipped(s, (4, 0), (1, 100), (0, 256))])
    assert L.want[1][:4] == (0, 0, 0, 3)
    run_device(engine, L)
    run_host(engine, L)


def test_plain_decode(engine):
    """n == k: reported consistent, a plain decode of the blocks as held."""
    run_both(engine, [spec(4, 6, 4099, [5, 0, 3, 2]), spec(4, 6, 17, [0, 1, 2, 3], flips=[(1, 3)]),
                      spec(4, 6, 4101, [0, 1, 2, 3], padlen=7, short=True)])


def _junk(s, entry, seed):
    """`s` with one whole entry replaced by random bytes."""
    _, blocks = _chunk(s["k"], s["m"], s["B"], s["padlen"], s["seed"])
    true = np.frombuffer(blocks[s["entries"][entry]], np.uint8)
    junk = np.random.default_rng(seed).integers(0, 256, true.size, dtype=np.uint8)
    diff = true ^ junk
    return flipped(s, *[(entry, int(p), int(diff[p])) for p in np.flatnonzero(diff)]), int(np.count_nonzero(diff))


@pytest.mark.parametrize("entry", [2, 5])
def test_whole_piece_junk(engine, entry):
    """One whole piece replaced by random bytes, RS(4,6) B = 4099: corrected equals the positions
    where the random byte differs from the true one, and the hits fall on that entry only."""
    s, ndiff = _junk(spec(4, 6, 4099, E46), entry, 77 + entry)
    L = _layout([s])
    assert 4000 < ndiff <= 4099 and L.want[0][2] == ndiff and L.want[0][4][entry] == ndiff
    run_device(engine, L)
    run_host(engine, L)


def _mixed():
    s46 = spec(4, 6, 4099, E46)
    return [Z1014_SHORT, flipped(s46, (4, 4095), (0, 4096), (3, 4098)), s46,
            flipped(Z1624, (14, 7), (3, 255)), spec(4, 6, 5, E46_ALL), flipped(spec(4, 6, 5, E46_ALL), (1, 4)),
            flipped(Z3248, (32 + 12, 5), (31, 129)), Z1624, flipped(Z1014_ALL, (2, 3000), (12, 3000, 0x21), (7, 41)),
            spec(4, 6, 17, [0, 1, 2, 3], flips=[(1, 3)]), flipped(spec(4, 6, 257, [5, 0, 3, 2, 1]), (1, 100)),
            _junk(spec(4, 6, 63, E46_ALL), 1, 5)[0], Z6496, flipped(Z6496, (63, 0), (64 + 15, 31)),
            flipped(Z1014_SHORT, (7, 6549))]


def test_mixed_batch_twice_from_the_cached_plan(engine):
    """Every shape of this file in one call with clean chunks between; then the same plan on data
    changed in place (all clean): no count is left over from the first call."""
    L1 = _layout(_mixed())
    L2 = _layout([flipped(s) for s in _mixed()])
    assert L1.descs.tobytes() == L2.descs.tobytes() and np.array_equal(L1.bo, L2.bo)
    dsrc = run_device(engine, L1)
    dsrc.copy_(torch.from_numpy(L2.src))
    run_device(engine, L2, dsrc)
    run_device(engine, L1, asynchronous=True, with_hits=False)
    run_host(engine, L1)


def test_host_mode_is_staged_over_several_slabs():
    eng = Engine(0, options={"SEC_SLAB_BYTES": 1 << 16})
    try:
        run_host(eng, _layout(_mixed()))
        assert eng.host_paths() == (0, 0, 1)
        assert eng.check_methods() == (0, 0) and eng.decode_methods() == (0, 0, 0, 0)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_timing_kind_decode_correct(engine):
    engine.set_timing(True)
    try:
        for kind in ("decode_correct", "decode_check", "decode", "check"):
            engine.collect_timing(kind)
        run_device(engine, _layout([flipped(Z1624, (3, 100))]))
        ms, launches = engine.collect_timing("decode_correct")
        assert launches == 1 and ms > 0
        for kind in ("decode_check", "decode", "check"):
            assert engine.collect_timing(kind) == (0.0, 0)
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    """Each error code in sec_decode_check_batch's order; no buffer is touched (the addresses handed
    over do not exist, and the results stay as they were)."""
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=DCHK_DTYPE)
    d[0] = (0, 64, 3, 0, 6, 4, 6, 0)
    bo = np.zeros(8, np.uint64)  # never dereferenced: every call fails first
    res = np.full(24, 0x77, dtype=np.uint8).view(COR_RESULT_DTYPE)
    before = res.tobytes()
    OUT = 0x1000  # never dereferenced either

    def call(sn, flags=0, desc=d, results=True, offs=True, out=OUT):
        sn = None if sn is None else np.array(sn, np.int32)
        return lib.sec_decode_correct_batch(ctx, desc.ctypes.data, 1, None if sn is None else sn.ctypes.data,
                                            bo.ctypes.data if offs else None, None, None, out,
                                            res.ctypes.data if results else None, None, flags)

    def desc(**kw):
        bad = d.copy()
        for f, v in kw.items():
            bad[f] = v
        return bad

    ok = [0, 2, 3, 4, 1, 5]
    assert call(ok, flags=_lib.SEC_F_STAGED | _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_GPU_PARITY_IDS) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call(None) == _lib.SEC_EINVAL
    assert call(ok, offs=False) == _lib.SEC_EINVAL
    assert call(ok, results=False) == _lib.SEC_EINVAL
    assert call(ok, out=None) == _lib.SEC_EINVAL  # k*B - padlen bytes to write
    assert call(ok, desc=desc(n=-1)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1, k=5, m=4)) == _lib.SEC_EINVAL  # before SEC_EKM
    assert call(ok, desc=desc(k=5, m=4)) == _lib.SEC_EKM
    assert call(ok, desc=desc(k=7, m=6, n=3)) == _lib.SEC_EKM  # before SEC_ENBLOCKS
    assert call(ok, desc=desc(n=3)) == _lib.SEC_ENBLOCKS
    assert call(ok + [9], desc=desc(n=7)) == _lib.SEC_ENBLOCKS  # n > m, before SEC_ESHARENUM
    assert call([0, 2, 3, 6, 1, 5]) == _lib.SEC_ESHARENUM
    assert call([0, 0, 3, 4, 1, 6]) == _lib.SEC_ESHARENUM  # before SEC_EDUPSHARE
    assert call([0, 2, 3, 4, 1, 3]) == _lib.SEC_EDUPSHARE
    assert call([0, 2, 3, 4, 1, 3], desc=desc(padlen=4 * 64 + 1)) == _lib.SEC_EDUPSHARE  # before SEC_EPADLEN
    assert call(ok, desc=desc(padlen=4 * 64 + 1)) == _lib.SEC_EPADLEN
    assert call(ok, desc=desc(B=1 << 31, padlen=(1 << 33) + 1)) == _lib.SEC_EPADLEN  # before SEC_ESIZE
    assert call(ok, desc=desc(B=1 << 31)) == _lib.SEC_ESIZE
    assert res.tobytes() == before


def test_decode_correct_host_from_bytes(engine):
    specs = _mixed()
    items, want = [], b""
    for s in specs:
        held, _ = _held(dict(s, short=False))
        items.append((s["k"], s["m"], [bytes(b) for b in held], s["entries"], s["padlen"]))
        want += _expect(s, held)[0]
    data, results = engine.decode_correct_host(items)
    assert data == want
    for s, it, got in zip(specs, items, results):
        assert got == _expect(s, [bytearray(b) for b in it[2]])[1:6]
    assert engine.decode_correct_host([]) == (b"", [])
    assert pinned_bytes()[0] == 0
    with pytest.raises(Error):
        engine.decode_correct_host([(4, 6, [b"ab"] * 5, [0, 2, 3, 4, 4], 0)])


def _encoded(ci, data, k, m, damage):
    """An EncodedChunk of `data` with every piece held; damage: (piece_idx, offset) bytes flipped."""
    B = -(-len(data) // k)
    held = [bytearray(b) for b in cfec.easy_encode(data + b"\0" * (k * B - len(data)), k, m)]
    for idx, at in damage:
        held[idx][at] ^= 0x01
    pieces = [piece.Piece(chunk_idx=ci, piece_idx=i, data=bytes(b),
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(held)]
    return piece.EncodedChunk(pieces=pieces, chunk_idx=ci, k=k, m=m, chunk_size=B, padlen=k * B - len(data),
                              original_chunk_size=len(data))


def _datas(n, count, seed):
    return [np.random.default_rng(seed + ci).integers(0, 256, n - ci, dtype=np.uint8).tobytes() for ci in range(count)]


def test_clean_download_launches_nothing_new():
    """Clean input through piece.decode_chunks_corrected: no launch of the correcting kernels, and
    output and verdicts equal decode_chunks_checked's."""
    datas = _datas(256 << 10, 3, 500)
    chunks = [_encoded(ci, d, 4, 6, []) for ci, d in enumerate(datas)]
    eng = get_engine()
    eng.set_timing(True)
    try:
        eng.collect_timing("decode_correct")
        eng.collect_timing("decode_check")
        got, cors = piece.decode_chunks_corrected(chunks)
        assert eng.collect_timing("decode_correct") == (0.0, 0)
        assert eng.collect_timing("decode_check")[1] >= 1  # round one, the call decode_chunks_checked makes
    finally:
        eng.set_timing(False)
    want, checks = piece.decode_chunks_checked(chunks)
    assert got == want == b"".join(datas)
    assert [(c.chunk_idx, c.checked, c.consistent, c.first_bad_offset) for c in cors] == [
        (c.chunk_idx, c.checked, c.consistent, c.first_bad_offset) for c in checks]
    assert all(c.damaged == {} and c.corrected_positions == 0 and c.open_positions == 0 for c in cors)


def test_two_pieces_damaged_at_different_offsets_end_to_end():
    """RS(4,2), piece 1 bad at offset 100 and piece 4 bad at 9000: decode_chunks_checked names one,
    is left with one check row and ends located=False; the corrected decode returns the chunk."""
    datas = _datas(256 << 10, 3, 600)
    chunks = [_encoded(0, datas[0], 4, 6, []), _encoded(1, datas[1], 4, 6, [(1, 100), (4, 9000)]),
              _encoded(2, datas[2], 4, 6, [(5, 0)])]
    _, checks = piece.decode_chunks_checked(chunks)
    assert not checks[1].consistent and not checks[1].located
    got, cors = piece.decode_chunks_corrected(chunks)
    assert got == b"".join(datas)
    assert [(c.consistent, c.first_bad_offset, c.corrected_positions, c.open_positions, c.damaged) for c in cors] == [
        (True, None, 0, 0, {}), (False, 100, 2, 0, {1: 1, 4: 1}), (False, 0, 1, 0, {5: 1})]
    pieces = [p for ch in chunks for p in ch.pieces]
    assert piece.reconstruct_data_corrected(pieces, chunks)[0] == b"".join(datas)
    assert b"".join(d for d, _ in piece.reconstruct_data_stream_corrected(pieces, chunks)) == b"".join(datas)
    assert pinned_bytes()[0] == 0
