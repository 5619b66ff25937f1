"""GPU: sec_check_batch against expectations that never come from another HIP path.  Blocks =
cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c); corruptions are single flipped bytes put into
the buffer image in numpy, and what the check must report follows from where the test put them:
a flip in a check row flags that row; a flip in a basis block flags every check row (the code is
MDS: every coefficient of a check row over the basis is nonzero); `first` is the lowest flipped
position and `column` the entries' bytes there.

Layout of every case: each entry sits in a buffer of 0xFF at odd and even starts, so a short entry
(block_avail < B) is followed by 0xFF bytes and a read past its avail shows up as a difference.
The buffer must be byte-identical after every call."""

import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE  # noqa: E402
from storb_amd.engine import Engine, Error, check_locate, pinned_bytes  # noqa: E402

UNTOUCHED = 0xEE  # row_bad / column before the call


@functools.lru_cache(maxsize=None)
def _blocks(k, m, B, padlen, seed):
    """The oracle's m blocks of a seeded chunk of k*B - padlen bytes (block k-1 zero-padded)."""
    n = k * B - padlen
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes() + b"\0" * padlen
    blocks = cfec.easy_encode(data, k, m)
    assert len(blocks) == m and all(len(b) == B for b in blocks)
    return blocks


def spec(k, m, B, entries, flips=(), padlen=0, short=False, seed=None):
    """One chunk: blocks `entries` held (the first k the basis).  flips: (entry position, byte
    position) of bytes XORed with 0x5A.  short: block k-1, wherever it is among the entries, is
    handed over with block_avail = B - padlen (its zero padding not in memory)."""
    assert len(set(entries)) == len(entries) >= k
    return dict(k=k, m=m, B=B, entries=list(entries), flips=list(flips), padlen=padlen, short=short,
                seed=seed if seed is not None else 1000 * k + m + B)


def flipped(s, *flips):
    return dict(s, flips=list(flips))


def _layout(specs):
    """The buffer image, the call's arrays (offsets relative to the buffer) and, per chunk, what
    the check must report."""
    descs = np.zeros(len(specs), dtype=CHK_DTYPE)
    sn, bo, av, want = [], [], [], []
    cur = 3
    parts = []
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        blocks = _blocks(k, s["m"], B, s["padlen"], s["seed"])
        descs[i] = (B, len(sn), n, k, s["m"], 0)
        held, avail = [], []
        for j, b in enumerate(s["entries"]):
            a = B - s["padlen"] if s["short"] and b == k - 1 else B
            held.append(bytearray(blocks[b][:a]))
            avail.append(a)
        for e, p in s["flips"]:
            assert p < avail[e], "a flip must land on a byte that is in memory"
            held[e][p] ^= 0x5A
        for j in range(n):
            sn.append(s["entries"][j])
            bo.append(cur)
            av.append(avail[j])
            parts.append((cur, bytes(held[j])))
            cur += B + 5 + 2 * j  # odd and even starts; what lies between stays 0xFF
        if s["flips"]:
            first = min(p for _, p in s["flips"])
            rows = set(range(k, n)) if any(e < k for e, _ in s["flips"]) else {e for e, _ in s["flips"]}
            column = bytes(held[j][first] if first < avail[j] else 0 for j in range(n))
            want.append((first, rows, column))
        else:
            want.append(None)
    src = np.full(cur + 64, 0xFF, np.uint8)
    for o, b in parts:
        src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return SimpleNamespace(descs=descs, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), src=src, want=want, specs=specs)


def _verify(L, res, rb, col, locate=True):
    res = np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=CHK_RESULT_DTYPE)
    for i, (s, w) in enumerate(zip(L.specs, L.want)):
        s0, n, k = int(L.descs[i]["slot0"]), len(s["entries"]), s["k"]
        if w is None:
            assert int(res[i]["first"]) == CHK_CONSISTENT and int(res[i]["nbad"]) == 0, f"chunk {i}: clean"
            assert not rb[s0:s0 + n].any(), f"chunk {i}: a flag on a clean chunk"
            assert (col[s0:s0 + n] == UNTOUCHED).all(), f"chunk {i}: column of a consistent chunk was written"
            continue
        first, rows, column = w
        assert int(res[i]["first"]) == first, f"chunk {i}: first"
        assert int(res[i]["nbad"]) == len(rows), f"chunk {i}: nbad"
        assert {j for j in range(n) if rb[s0 + j]} == rows and set(rb[s0:s0 + n].tolist()) <= {0, 1}, f"chunk {i}"
        assert col[s0:s0 + n].tobytes() == column, f"chunk {i}: column"
        who = check_locate(k, s["m"], s["entries"], column)
        if locate and n - k >= 2 and len({e for e, p in s["flips"] if p == first}) == 1:
            assert who == next(e for e, p in s["flips"] if p == first), f"chunk {i}: locate"
        elif n - k < 2:
            assert who == -2


def run_device(engine, L, dsrc=None, asynchronous=False, use_avail=True, outputs=True):
    nslots = len(L.sn)
    if dsrc is None:
        dsrc = torch.from_numpy(L.src).cuda()
    res = torch.zeros(16 * len(L.specs), dtype=torch.uint8, device="cuda")
    rb = torch.full((nslots,), UNTOUCHED, dtype=torch.uint8, device="cuda") if outputs else None
    col = torch.full((nslots,), UNTOUCHED, dtype=torch.uint8, device="cuda") if outputs else None
    engine.check_batch(L.descs, L.sn, L.bo + np.uint64(dsrc.data_ptr()), 0, res,
                       block_avail=L.av if use_avail else None, row_bad=rb, column=col, asynchronous=asynchronous)
    if asynchronous:
        engine.sync()
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    if outputs:
        _verify(L, res.cpu().numpy(), rb.cpu().numpy(), col.cpu().numpy())
    return np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)


E46 = [5, 0, 3, 2, 4, 1]  # RS(4,6): basis {5,0,3,2} in that order, check rows 4 and 1


# ---- device mode ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 4101, 33001])
def test_clean_block_sizes(engine, B):
    """The tail kernel only (B < 16), exactly one lane, one clamped lane, a ragged last tile,
    several tiles."""
    run_device(engine, _layout([spec(4, 6, B, E46)]), use_avail=False)


@pytest.mark.parametrize("B", [4101, 33001])
def test_one_flip_in_a_check_row(engine, B):
    """Positions 0, 15, 16, around a tile boundary, valid-1 = B-1; and, with a short basis block
    (valid = B - 5), valid-1, valid (the ragged part) and B-1."""
    cases = [flipped(spec(4, 6, B, E46), (4 + (i % 2), p)) for i, p in enumerate([0, 15, 16, 4095, 4096, B - 1])]
    short = spec(4, 6, B, E46, padlen=5, short=True)
    cases += [flipped(short, (5, p)) for p in (B - 6, B - 5, B - 1)]
    run_device(engine, _layout(cases))


@pytest.mark.parametrize("B", [17, 4101])
def test_one_flip_in_a_basis_block(engine, B):
    """Every check row is flagged and locate names the basis entry, whichever slot it is
    normalised into."""
    run_device(engine, _layout([flipped(spec(4, 6, B, E46), (e, p)) for e, p in [(0, 0), (1, B - 1), (2, 16), (3, 7)]]))


def test_two_flips_report_the_lower_position(engine):
    s = spec(4, 6, 33001, E46)
    run_device(engine, _layout([flipped(s, (4, 20000), (5, 4097)), flipped(s, (5, 30000), (2, 12345)),
                                flipped(s, (4, 77), (5, 77))]))


@pytest.mark.parametrize("padlen", [1, 3, 4101])
def test_short_blocks(engine, padlen):
    """Block k-1 read in place with avail = B - padlen (0xFF behind it), as a basis entry and as a
    check row: clean.  A nonzero predicted byte past the check row's avail is detected: a basis
    byte flipped at a position >= avail."""
    B = 4101
    basis = spec(4, 6, B, [3, 0, 5, 2, 4, 1], padlen=padlen, short=True)
    row = spec(4, 6, B, [5, 0, 4, 2, 3, 1], padlen=padlen, short=True)
    run_device(engine, _layout([basis, row, flipped(row, (1, B - padlen)), flipped(row, (2, B - 1)),
                                flipped(basis, (4, B - 1))]))


_SRC96 = random.Random(6496).sample(range(96), 96)
ROW_GROUPS = {
    "10,14": spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 12, 8, 9, 7, 10, 1, 4]),
    "16,24": spec(16, 24, 4105, [s for s in range(24) if s not in (1, 4, 9, 14, 16, 19, 21, 23)][::-1] +
                  [19, 1, 23, 9, 16, 4, 21, 14]),
    "3,12": spec(3, 12, 5003, [10, 1, 6, 11, 0, 9, 2, 8, 3, 7, 4, 5]),
    "64,96": spec(64, 96, 2055, _SRC96, seed=6496),  # shuffled basis, 32 rows = four groups, wide-k loop
    "1,3": spec(1, 3, 4097, [2, 1, 0]),
}


@pytest.mark.parametrize("name", list(ROW_GROUPS))
def test_row_groups(engine, name):
    """Clean, one flip in a row of the last group, and one in a basis block."""
    s = ROW_GROUPS[name]
    n, B = len(s["entries"]), s["B"]
    run_device(engine, _layout([s, flipped(s, (n - 1, B - 3)), flipped(s, (s["k"] // 2, B // 2))]))


def test_nothing_to_check(engine):
    """n == k: consistent, and no kernel of the check is timed."""
    engine.set_timing(True)
    try:
        engine.collect_timing("check")
        run_device(engine, _layout([spec(4, 6, 4101, [5, 0, 3, 2]), spec(10, 14, 17, list(range(10)))]))
        assert engine.collect_timing("check") == (0.0, 0)
    finally:
        engine.set_timing(False)


def _mixed(corrupt):
    """Seven shapes in one call; `corrupt` picks which chunks carry a flip."""
    a, b, c = ROW_GROUPS["10,14"], spec(4, 6, 33001, E46), ROW_GROUPS["3,12"]
    specs = [a, spec(4, 6, 17, E46), spec(4, 6, 4101, [0, 1, 2, 3]), c,
             spec(4, 6, 7, [3, 0, 5, 2, 4, 1], padlen=2, short=True), ROW_GROUPS["64,96"], ROW_GROUPS["1,3"], b]
    flips = {0: (12, 6000), 3: (1, 5002), 4: (5, 6), 5: (95, 2054), 7: (4, 32999)}
    return [flipped(s, flips[i]) if i in corrupt else s for i, s in enumerate(specs)]


def test_mixed_batch_twice_from_the_cached_plan(engine):
    """The second call reuses the plan on data changed in place: one chunk healed, others
    corrupted.  Its results must be the new data's (no flag left over from the first call)."""
    L1, L2 = _layout(_mixed({0, 4, 5})), _layout(_mixed({3, 4, 7}))
    assert L1.descs.tobytes() == L2.descs.tobytes() and np.array_equal(L1.bo, L2.bo)
    dsrc = torch.from_numpy(L1.src).cuda()
    run_device(engine, L1, dsrc)
    dsrc.copy_(torch.from_numpy(L2.src))
    run_device(engine, L2, dsrc)
    dsrc.copy_(torch.from_numpy(_layout(_mixed(set())).src))
    run_device(engine, _layout(_mixed(set())), dsrc)


def test_async_then_sync(engine):
    run_device(engine, _layout(_mixed({0, 7})), asynchronous=True)


def test_results_alone(engine):
    """row_bad and column are optional."""
    res = run_device(engine, _layout(_mixed({3})), outputs=False)
    assert [int(r["first"]) for r in res] == [CHK_CONSISTENT] * 3 + [5002] + [CHK_CONSISTENT] * 4
    assert [int(r["nbad"]) for r in res] == [0, 0, 0, 9, 0, 0, 0, 0]


def test_timing_kind_check(engine):
    engine.set_timing(True)
    try:
        engine.collect_timing("check")
        run_device(engine, _layout([ROW_GROUPS["10,14"]]))
        ms, launches = engine.collect_timing("check")
        assert launches == 1 and ms > 0
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=CHK_DTYPE)
    d[0] = (64, 0, 6, 4, 6, 0)
    bo = np.zeros(8, np.uint64)  # never dereferenced: every call fails first
    res = np.zeros(1, dtype=CHK_RESULT_DTYPE)

    def call(sn, flags=0, desc=d, results=True, offs=True):
        sn = None if sn is None else np.array(sn, np.int32)
        return lib.sec_check_batch(ctx, desc.ctypes.data, 1, None if sn is None else sn.ctypes.data,
                                   bo.ctypes.data if offs else None, None, None,
                                   res.ctypes.data if results else None, None, None, flags)

    def desc(**kw):
        bad = d.copy()
        for f, v in kw.items():
            bad[f] = v
        return bad

    ok = [0, 2, 3, 4, 1, 5]
    assert call(ok, flags=_lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_STAGED | _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC) == _lib.SEC_EINVAL
    assert call(None) == _lib.SEC_EINVAL
    assert call(ok, offs=False) == _lib.SEC_EINVAL
    assert call(ok, results=False) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1, k=5, m=4)) == _lib.SEC_EINVAL  # before SEC_EKM
    assert call(ok, desc=desc(k=5, m=4)) == _lib.SEC_EKM
    assert call(ok, desc=desc(k=7, m=6, n=3)) == _lib.SEC_EKM  # before SEC_ENBLOCKS
    assert call(ok, desc=desc(n=3)) == _lib.SEC_ENBLOCKS
    assert call(ok + [9], desc=desc(n=7)) == _lib.SEC_ENBLOCKS  # n > m, before SEC_ESHARENUM
    assert call([0, 2, 3, 6, 1, 5]) == _lib.SEC_ESHARENUM
    assert call([0, 2, 3, 4, 1, -1]) == _lib.SEC_ESHARENUM
    assert call([0, 0, 3, 4, 1, 6]) == _lib.SEC_ESHARENUM  # before SEC_EDUPSHARE
    assert call([0, 2, 2, 4, 1, 5]) == _lib.SEC_EDUPSHARE  # within the basis
    assert call([0, 2, 3, 4, 1, 1]) == _lib.SEC_EDUPSHARE  # within the check rows
    assert call([0, 2, 3, 4, 1, 3]) == _lib.SEC_EDUPSHARE  # a check row that is a basis block
    assert call([0, 2, 3, 4, 1, 3], desc=desc(B=1 << 31)) == _lib.SEC_EDUPSHARE  # before SEC_ESIZE
    assert call(ok, desc=desc(B=1 << 31)) == _lib.SEC_ESIZE


# ---- host mode --------------------------------------------------------------------------
def run_host(eng, L, src=None):
    nslots = len(L.sn)
    src = L.src.copy() if src is None else src
    res = np.zeros(len(L.specs), dtype=CHK_RESULT_DTYPE)
    rb, col = np.full(nslots, UNTOUCHED, np.uint8), np.full(nslots, UNTOUCHED, np.uint8)
    eng.check_batch(L.descs, L.sn, L.bo, src, res, block_avail=L.av, row_bad=rb, column=col, host=True)
    assert np.array_equal(src, L.src), "the source buffer was written"
    _verify(L, res, rb, col)


def test_host_numpy_buffers_are_staged(engine):
    z0, r0, s0 = engine.host_paths()
    run_host(engine, _layout(_mixed({0, 4, 7})))
    assert engine.host_paths() == (z0, r0, s0 + 1)  # never zero-copy, never page-locked
    assert pinned_bytes()[0] == 0  # the slabs went back to the pool
    run_host(engine, _layout(_mixed({3})))  # the cached plan, other data


def test_host_several_slabs():
    """The staging pipeline over more slabs than it has slots: 64 KiB slabs, so every chunk of
    the mix but the small ones is a slab of its own (results scattered per slab)."""
    eng = Engine(0, options={"SEC_SLAB_BYTES": 1 << 16})
    try:
        run_host(eng, _layout(_mixed({0, 3, 5, 7}) + [ROW_GROUPS["16,24"]]))
        assert eng.host_paths() == (0, 0, 1)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_host_pinned_buffers_are_staged_too(engine):
    L = _layout(_mixed({4, 7})[3:])
    psrc = engine.host_empty(L.src.size)
    psrc[:] = L.src
    z0, r0, s0 = engine.host_paths()
    run_host(engine, L, psrc)
    assert engine.host_paths() == (z0, r0, s0 + 1)
    assert pinned_bytes()[0] == 0


def test_check_host_from_bytes(engine):
    specs = _mixed({0, 3})[:5]
    items = []
    for s in specs:
        blocks = [bytearray(_blocks(s["k"], s["m"], s["B"], s["padlen"], s["seed"])[b]) for b in s["entries"]]
        for e, p in s["flips"]:
            blocks[e][p] ^= 0x5A
        items.append((s["k"], s["m"], [bytes(b) for b in blocks], s["entries"]))
    got = engine.check_host(items)
    for (k, m, blocks, entries), s, (first, bad, column) in zip(items, specs, got):
        if not s["flips"]:
            assert (first, bad, column) == (None, [], None)
            continue
        (e, p), = s["flips"]
        assert first == p and column == bytes(b[p] for b in blocks)
        assert bad == (list(range(k, len(entries))) if e < k else [e])
        assert check_locate(k, m, entries, column) == e
    assert engine.check_host([]) == []
    assert pinned_bytes()[0] == 0
    with pytest.raises(Error):
        engine.check_host([(4, 6, [b"ab"] * 5, [0, 2, 3, 4, 4])])


def test_check_then_repair_end_to_end():
    """piece.check_pieces on a 256 KiB RS(4,2) chunk with one byte of a data piece flipped: the
    piece is located, and repair_pieces from the others returns the oracle's block."""
    n = 256 << 10
    data = np.random.default_rng(256).integers(0, 256, n, dtype=np.uint8).tobytes()
    k, m = 4, 6
    B = -(-n // k)
    blocks = cfec.easy_encode(data, k, m)
    bad_idx, at = 2, 40000
    held = [bytearray(b) for b in blocks]
    held[bad_idx][at] ^= 0x01
    pieces = [piece.Piece(chunk_idx=5, piece_idx=i, data=bytes(b),
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(held)]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=5, k=k, m=m, chunk_size=B, padlen=k * B - n, original_chunk_size=n)
    got = piece.check_pieces(ec)
    assert (got.chunk_idx, got.checked, got.consistent, got.first_bad_offset) == (5, 6, False, at)
    assert got.bad_piece_idx == [bad_idx] and got.located
    ec.pieces = [p for p in pieces if p.piece_idx not in got.bad_piece_idx]
    fixed = piece.repair_pieces(ec, targets=got.bad_piece_idx)
    assert [(p.piece_idx, p.data) for p in fixed] == [(bad_idx, blocks[bad_idx])]
    ec.pieces = sorted(ec.pieces + fixed, key=lambda p: p.piece_idx)
    assert piece.check_pieces(ec).consistent
