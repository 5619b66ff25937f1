"""GPU: sec_decode_check_batch against expectations that never come from another HIP path.  Blocks
= cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c); corruptions are single flipped bytes put
into the buffer image in numpy.  The expected output is cfec.easy_decode of the first k entries AS
HELD, flips included; the expected results follow from where the test put the flips, as in
tests/test_gpu_check.py: a flip in a check row flags that row and leaves `out` correct, a flip in a
basis block flags every check row (the code is MDS: every coefficient is nonzero) and changes every
recovered row at that position.

Layout of every case: each entry sits in a buffer of 0xFF at odd and even starts, so a short entry
(block_avail < B) is followed by 0xFF bytes and a read past its avail shows up as a difference; the
buffer must be byte-identical after every call.  `out` is 0xFF-filled too, every chunk's bytes at
an odd or even start with guard bytes around them, and is compared whole."""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, DCHK_DTYPE, DEC_DTYPE  # noqa: E402
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
    """One chunk: blocks `entries` held, the first k decoded from (and the check's basis), the rest
    the check rows.  flips: (entry position, byte position) of bytes XORed with 0x5A.  short: block
    k-1, wherever it is among the entries, is handed over with block_avail = B - padlen."""
    assert len(set(entries)) == len(entries) >= k
    return dict(k=k, m=m, B=B, entries=list(entries), flips=list(flips), padlen=padlen, short=short,
                seed=seed if seed is not None else 1000 * k + m + B)


def flipped(s, *flips):
    return dict(s, flips=list(flips))


def _held(s):
    """The chunk's entries as held (flips applied, a short entry cut at its avail) and their avail."""
    k, B = s["k"], s["B"]
    blocks = _blocks(k, s["m"], B, s["padlen"], s["seed"])
    held, avail = [], []
    for b in s["entries"]:
        a = B - s["padlen"] if s["short"] and b == k - 1 else B
        held.append(bytearray(blocks[b][:a]))
        avail.append(a)
    for e, p in s["flips"]:
        assert p < avail[e], "a flip must land on a byte that is in memory"
        held[e][p] ^= 0x5A
    return held, avail


def _layout(specs, recover=False):
    """The buffer image, the call's arrays (offsets relative to the buffers), the expected image of
    `out` and, per chunk, what the check must report."""
    descs = np.zeros(len(specs), dtype=DCHK_DTYPE)
    sn, bo, av, want, parts, outs = [], [], [], [], [], []
    cur, ocur = 3, 7
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        held, avail = _held(s)
        descs[i] = (ocur, B, s["padlen"], len(sn), n, k, s["m"], 0)
        # the oracle's decode of the first k entries as held, bytes past an entry's avail zero
        basis = [bytes(h) + b"\0" * (B - len(h)) for h in held[:k]]
        if recover:
            whole = cfec.easy_decode(basis, s["entries"][:k], 0, k, s["m"])
            exp = b"".join(whole[j * B:(j + 1) * B] for j in range(k) if j not in s["entries"][:k])
        else:
            exp = cfec.easy_decode(basis, s["entries"][:k], s["padlen"], k, s["m"])
        outs.append((ocur, exp))
        ocur += len(exp) + 9 + (i % 2)  # guard bytes between the chunks, odd and even starts
        for j in range(n):
            sn.append(s["entries"][j])
            bo.append(cur)
            av.append(avail[j])
            parts.append((cur, bytes(held[j])))
            cur += B + 5 + 2 * j  # odd and even starts; what lies between stays 0xFF
        if s["flips"] and n > k:
            first = min(p for _, p in s["flips"])
            rows = set(range(k, n)) if any(e < k for e, _ in s["flips"]) else {e for e, _ in s["flips"]}
            column = bytes(held[j][first] if first < avail[j] else 0 for j in range(n))
            want.append((first, rows, column))
        else:
            want.append(None)  # (n == k: nothing to check, consistent whatever the bytes)
    src = np.full(cur + 64, 0xFF, np.uint8)
    for o, b in parts:
        src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    out = np.full(ocur + 64, 0xFF, np.uint8)
    for o, b in outs:
        out[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return SimpleNamespace(descs=descs, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), src=src, out=out, want=want, specs=specs, recover=recover)


def _verify(L, res, rb, col):
    res = np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=CHK_RESULT_DTYPE)
    for i, (s, w) in enumerate(zip(L.specs, L.want)):
        s0, n, k = int(L.descs[i]["slot0"]), len(s["entries"]), s["k"]
        if w is None:
            assert int(res[i]["first"]) == CHK_CONSISTENT and int(res[i]["nbad"]) == 0, f"chunk {i}: clean"
            if rb is not None:
                assert not rb[s0:s0 + n].any(), f"chunk {i}: a flag on a clean chunk"
                assert (col[s0:s0 + n] == UNTOUCHED).all(), f"chunk {i}: column of a consistent chunk was written"
            continue
        first, rows, column = w
        assert int(res[i]["first"]) == first, f"chunk {i}: first"
        assert int(res[i]["nbad"]) == len(rows), f"chunk {i}: nbad"
        if rb is None:
            continue
        assert {j for j in range(n) if rb[s0 + j]} == rows and set(rb[s0:s0 + n].tolist()) <= {0, 1}, f"chunk {i}"
        assert col[s0:s0 + n].tobytes() == column, f"chunk {i}: column"
        if n - k >= 2 and len({e for e, p in s["flips"] if p == first}) == 1:
            assert check_locate(k, s["m"], s["entries"], column) == next(e for e, p in s["flips"] if p == first)


def _out_diff(got, want):
    d = np.flatnonzero(got != want)
    return f"out differs at {d[:8].tolist()} ({d.size} bytes)" if d.size else ""


def run_device(engine, L, dsrc=None, asynchronous=False, use_avail=True, outputs=True):
    nslots = len(L.sn)
    if dsrc is None:
        dsrc = torch.from_numpy(L.src).cuda()
    dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
    res = torch.zeros(16 * len(L.specs), dtype=torch.uint8, device="cuda")
    rb = torch.full((nslots,), UNTOUCHED, dtype=torch.uint8, device="cuda") if outputs else None
    col = torch.full((nslots,), UNTOUCHED, dtype=torch.uint8, device="cuda") if outputs else None
    engine.decode_check_batch(L.descs, L.sn, L.bo + np.uint64(dsrc.data_ptr()), 0, dout, res,
                              block_avail=L.av if use_avail else None, row_bad=rb, column=col,
                              asynchronous=asynchronous, recover_only=L.recover)
    if asynchronous:
        engine.sync()
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    assert not _out_diff(dout.cpu().numpy(), L.out)
    _verify(L, res.cpu().numpy(), rb.cpu().numpy() if outputs else None, col.cpu().numpy() if outputs else None)
    return dsrc, dout, res, rb, col


# RS(4,6) decoded from blocks {5, 0, 3, 2} in that order: primary 1 is lost (e = 1) and is also a
# check row, so the recovered row and the stored block 1 must agree; the other check row is block 4
E46 = [5, 0, 3, 2, 4, 1]
# ... and from {5, 0, 3, 4}: primaries 1 and 2 lost (e = 2), both held as the two check rows
E46_E2 = [5, 0, 3, 4, 2, 1]


# ---- device mode ------------------------------------------------------------------------
@pytest.mark.parametrize("entries", [E46, E46_E2], ids=["e1", "e2"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 4101, 33001])
def test_block_sizes_clean_and_single_flips(engine, B, entries):
    """The tail kernel only (B < 16), exactly one lane, one clamped lane, a ragged last tile,
    several tiles.  Clean; one flip in a check row; in a present-primary basis entry; in a parity
    basis entry."""
    s = spec(4, 6, B, entries)
    run_device(engine, _layout([s, flipped(s, (4 + B % 2, B // 2)), flipped(s, (1, B - 1)), flipped(s, (0, B // 3))]),
               use_avail=False)


def test_copy_and_check_only_and_plain_decode(engine):
    """All six held in order (e = 0: copies and check rows, nothing recovered), clean and flipped;
    n == k (no check rows): a plain decode, consistent whatever the bytes."""
    a = spec(4, 6, 4101, [0, 1, 2, 3, 4, 5])
    b = spec(4, 6, 4101, [5, 0, 3, 2])
    c = spec(4, 6, 4101, [0, 1, 2, 3], padlen=7, short=True)  # nothing to compute at all
    run_device(engine, _layout([a, flipped(a, (5, 4100)), flipped(a, (2, 0)), b, flipped(b, (0, 77)), c]))


Z1014_BASIS_SHORT = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 9, 8, 4, 12, 10], padlen=4, short=True)  # e = 2
Z1014_ROW_SHORT = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 1, 8, 4, 9, 12], padlen=4, short=True)  # e = 2
Z1014_E0 = spec(10, 14, 6554, [3, 0, 9, 1, 7, 5, 6, 2, 8, 4, 12, 10, 13, 11], padlen=4, short=True)  # four rows


@pytest.mark.parametrize("s,short_at", [(Z1014_BASIS_SHORT, 7), (Z1014_ROW_SHORT, 10), (Z1014_E0, 2)],
                         ids=["basis-short", "row-short", "e0"])
def test_short_block_in_place(engine, s, short_at):
    """zfec(10,14), B = 6554, padlen 4, block 9 handed over with avail = B - 4 (0xFF behind it), in
    the basis and as a check row.  Flips at 0, at 6549 (the short entry's last byte in memory) and
    at 6553 of a full-length entry."""
    n = len(s["entries"])
    full_basis, full_row = 1, n - 1
    assert short_at not in (full_basis, full_row)
    run_device(engine, _layout([s, flipped(s, (short_at, 0)), flipped(s, (short_at, 6549)), flipped(s, (full_basis, 6553)),
                                flipped(s, (full_row, 6553)), flipped(s, (full_row, 6549))]))


_P16 = [s for s in range(16) if s not in (1, 4, 9)]
Z1624 = spec(16, 24, 4101, _P16[::-1] + [16, 19, 21] + [23, 17, 20, 18, 22])  # e = 3, five rows: one 8-row group
_P32 = [s for s in range(32) if s not in (0, 13, 31)]
Z3248 = spec(32, 48, 4101, [40, 33] + _P32[::-1] + [47] + [32, 45, 39, 36, 42, 34])  # e = 3, six rows: 8 + 1
_Q32 = [s for s in range(32) if s not in (2, 3, 5, 8, 13, 21, 30, 31, 17, 11)]
Z3248_E10 = spec(32, 48, 4101, _Q32 + list(range(32, 42)) + [47, 44, 42], seed=324810)  # e = 10: 8 stored, 2 + 3


@pytest.mark.parametrize("s", [Z1624, Z3248, Z3248_E10], ids=["16,24", "32,48", "32,48-e10"])
def test_row_groups(engine, s):
    """Mixed store and compare rows in one 8-row group over a 16-slot batch; the wide-k loop with
    two groups, the first mixed (only the group with r0 == 0 copies); a second group that is mixed
    too.  Clean, a flip in the last check row, one in a basis block."""
    n, B = len(s["entries"]), s["B"]
    run_device(engine, _layout([s, flipped(s, (n - 1, B - 3)), flipped(s, (s["k"] // 2, B // 2))]))


def _mixed(corrupt):
    """Several shapes in one call, mixed order; `corrupt` picks which chunks carry a flip."""
    specs = [Z1014_BASIS_SHORT, spec(4, 6, 17, E46), spec(4, 6, 4101, [0, 1, 2, 3]), Z1624,
             spec(4, 6, 7, [3, 0, 5, 2, 4, 1], padlen=2, short=True), Z3248, spec(4, 6, 33001, E46_E2), Z1014_E0]
    flips = {0: (11, 6000), 1: (2, 16), 3: (20, 4100), 4: (5, 6), 5: (1, 2054), 6: (4, 32999), 7: (4, 1)}
    return [flipped(s, flips[i]) if i in corrupt else s for i, s in enumerate(specs)]


def test_mixed_batch_twice_from_the_cached_plan(engine):
    """The second call reuses the plan on data changed in place: chunks healed, others corrupted.
    Its results must be the new data's (no flag left over from the first call)."""
    L1, L2, L3 = _layout(_mixed({0, 4, 5})), _layout(_mixed({1, 3, 6, 7})), _layout(_mixed(set()))
    assert L1.descs.tobytes() == L2.descs.tobytes() and np.array_equal(L1.bo, L2.bo)
    dsrc = run_device(engine, L1)[0]
    dsrc.copy_(torch.from_numpy(L2.src))
    run_device(engine, L2, dsrc)
    dsrc.copy_(torch.from_numpy(L3.src))
    run_device(engine, L3, dsrc)


def test_recover_only(engine):
    """SEC_F_RECOVER in device mode: just the e recovered rows, B bytes each, in primary order; a
    chunk with e = 0 writes nothing.  The check is the same."""
    run_device(engine, _layout(_mixed({0, 3, 6}), recover=True))
    run_device(engine, _layout([spec(4, 6, B, E46_E2, flips=[(0, B - 1)]) for B in (1, 15, 17)], recover=True))


def test_async_then_sync(engine):
    run_device(engine, _layout(_mixed({0, 6})), asynchronous=True)


def test_results_alone(engine):
    """row_bad and column are optional."""
    res = run_device(engine, _layout(_mixed({3})), outputs=False)[2]
    res = np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)
    assert [int(r["first"]) for r in res] == [CHK_CONSISTENT] * 3 + [4100] + [CHK_CONSISTENT] * 4
    assert [int(r["nbad"]) for r in res] == [0, 0, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("recover", [False, True])
def test_same_as_check_then_decode(engine, recover):
    """For the same arrays `out` equals sec_decode_batch_ex's and the results sec_check_batch's:
    every shape of this file, clean and corrupt."""
    L = _layout(_mixed({0, 1, 5, 7}) + [Z3248_E10, Z1014_ROW_SHORT, flipped(spec(4, 6, 4101, [0, 1, 2, 3, 4, 5]), (1, 9))],
                recover=recover)
    dsrc, dout, res, rb, col = run_device(engine, L)
    offs = L.bo + np.uint64(dsrc.data_ptr())
    dec = np.zeros(len(L.specs), dtype=DEC_DTYPE)
    chk = np.zeros(len(L.specs), dtype=CHK_DTYPE)
    for i, d in enumerate(L.descs):
        dec[i] = (d["out_off"], d["B"], d["padlen"], d["slot0"], d["k"], d["m"])
        chk[i] = (d["B"], d["slot0"], d["n"], d["k"], d["m"], 0)
    dout2 = torch.full_like(dout, 0xFF)
    engine.decode_batch(dec, L.sn, offs, 0, dout2, block_avail=L.av, recover_only=recover)
    res2, rb2, col2 = torch.zeros_like(res), torch.full_like(rb, UNTOUCHED), torch.full_like(col, UNTOUCHED)
    engine.check_batch(chk, L.sn, offs, 0, res2, block_avail=L.av, row_bad=rb2, column=col2)
    assert torch.equal(dout, dout2)
    assert torch.equal(res, res2) and torch.equal(rb, rb2) and torch.equal(col, col2)


def test_timing_kind_decode_check(engine):
    engine.set_timing(True)
    try:
        engine.collect_timing("decode_check")
        engine.collect_timing("decode")
        engine.collect_timing("check")
        run_device(engine, _layout([Z1624]))
        ms, launches = engine.collect_timing("decode_check")
        assert launches == 1 and ms > 0
        assert engine.collect_timing("decode") == (0.0, 0) and engine.collect_timing("check") == (0.0, 0)
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    """Each error code in the documented order; no buffer is touched (the addresses handed over do
    not exist, and the results stay as they were)."""
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=DCHK_DTYPE)
    d[0] = (0, 64, 3, 0, 6, 4, 6, 0)
    bo = np.zeros(8, np.uint64)  # never dereferenced: every call fails first
    res = np.full(1, 0x77, dtype=np.uint8).repeat(16).view(CHK_RESULT_DTYPE)
    before = res.tobytes()
    OUT = 0x1000  # never dereferenced either

    def call(sn, flags=0, desc=d, results=True, offs=True, out=OUT):
        sn = None if sn is None else np.array(sn, np.int32)
        return lib.sec_decode_check_batch(ctx, desc.ctypes.data, 1, None if sn is None else sn.ctypes.data,
                                          bo.ctypes.data if offs else None, None, None, out,
                                          res.ctypes.data if results else None, None, None, flags)

    def desc(**kw):
        bad = d.copy()
        for f, v in kw.items():
            bad[f] = v
        return bad

    ok = [0, 2, 3, 4, 1, 5]
    assert call(ok, flags=_lib.SEC_F_STAGED | _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_GPU_PARITY_IDS) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC | _lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call(None) == _lib.SEC_EINVAL
    assert call(ok, offs=False) == _lib.SEC_EINVAL
    assert call(ok, results=False) == _lib.SEC_EINVAL
    assert call(ok, out=None) == _lib.SEC_EINVAL  # k*B - padlen bytes to write
    assert call(ok, out=None, flags=_lib.SEC_F_RECOVER) == _lib.SEC_EINVAL  # primary 1 is recovered
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
    assert call([0, 2, 3, 4, 1, 3], desc=desc(padlen=4 * 64 + 1)) == _lib.SEC_EDUPSHARE  # before SEC_EPADLEN
    assert call(ok, desc=desc(padlen=4 * 64 + 1)) == _lib.SEC_EPADLEN
    assert call(ok, desc=desc(B=1 << 31, padlen=(1 << 33) + 1)) == _lib.SEC_EPADLEN  # before SEC_ESIZE
    assert call(ok, desc=desc(B=1 << 31)) == _lib.SEC_ESIZE
    assert res.tobytes() == before


# ---- host mode --------------------------------------------------------------------------
def run_host(eng, L, src=None):
    nslots = len(L.sn)
    src = L.src.copy() if src is None else src
    out = np.full(L.out.size, 0xFF, np.uint8)
    res = np.zeros(len(L.specs), dtype=CHK_RESULT_DTYPE)
    rb, col = np.full(nslots, UNTOUCHED, np.uint8), np.full(nslots, UNTOUCHED, np.uint8)
    eng.decode_check_batch(L.descs, L.sn, L.bo, src, out, res, block_avail=L.av, row_bad=rb, column=col, host=True,
                           recover_only=L.recover)
    assert np.array_equal(src, L.src), "the source buffer was written"
    assert not _out_diff(out, L.out)
    _verify(L, res, rb, col)


@pytest.mark.parametrize("recover", [False, True])
def test_host_numpy_buffers_are_staged(engine, recover):
    z0, r0, s0 = engine.host_paths()
    run_host(engine, _layout(_mixed({0, 4, 6}), recover=recover))
    assert engine.host_paths() == (z0, r0, s0 + 1)  # never zero-copy, never page-locked
    assert pinned_bytes()[0] == 0  # the slabs went back to the pool
    run_host(engine, _layout(_mixed({3}), recover=recover))  # the cached plan, other data


def test_host_several_slabs():
    """The staging pipeline over more slabs than it has slots: 64 KiB slabs, so every chunk of the
    mix but the small ones is a slab of its own (output and results scattered per slab)."""
    eng = Engine(0, options={"SEC_SLAB_BYTES": 1 << 16})
    try:
        run_host(eng, _layout(_mixed({0, 3, 5, 6}) + [Z3248_E10]))
        assert eng.host_paths() == (0, 0, 1)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_decode_check_host_from_bytes(engine):
    specs = _mixed({0, 3, 6}) + [flipped(spec(4, 6, 4101, [0, 1, 2, 3, 4, 5]), (2, 40))]
    items, want = [], b""
    for s in specs:
        held, _ = _held(dict(s, short=False))
        items.append((s["k"], s["m"], [bytes(b) for b in held], s["entries"], s["padlen"]))
        want += cfec.easy_decode([bytes(b) for b in held[:s["k"]]], s["entries"][:s["k"]], s["padlen"], s["k"], s["m"])
    data, checks = engine.decode_check_host(items)
    assert data == want
    for (k, m, blocks, entries, _), s, (first, bad, column) in zip(items, specs, checks):
        if not s["flips"] or len(entries) == k:
            assert (first, bad, column) == (None, [], None)
            continue
        (e, p), = s["flips"]
        assert first == p and column == bytes(b[p] for b in blocks)
        assert bad == (list(range(k, len(entries))) if e < k else [e])
        assert check_locate(k, m, entries, column) == e
    assert engine.decode_check_host([]) == (b"", [])
    assert pinned_bytes()[0] == 0
    with pytest.raises(Error):
        engine.decode_check_host([(4, 6, [b"ab"] * 5, [0, 2, 3, 4, 4], 0)])
    with pytest.raises(Error):
        engine.decode_check_host([(4, 6, [b"ab"] * 5, [0, 2, 3, 4, 5], 9)])


def test_decode_chunks_checked_end_to_end():
    """piece.decode_chunks_checked on 256 KiB RS(4,2) chunks: a clean one, one with a byte of a
    data piece flipped (decoded from: located, and the second decode returns the right bytes), one
    with a flipped parity piece.  Expected bytes are the chunks themselves."""
    n, k, m = 256 << 10, 4, 6
    B = -(-n // k)
    datas, chunks = [], []
    for ci, (bad_idx, at) in enumerate([(None, 0), (2, 40000), (5, B - 1)]):
        data = np.random.default_rng(300 + ci).integers(0, 256, n - ci, dtype=np.uint8).tobytes()
        held = [bytearray(b) for b in cfec.easy_encode(data, k, m)]
        if bad_idx is not None:
            held[bad_idx][at] ^= 0x01
        pieces = [piece.Piece(chunk_idx=ci, piece_idx=i, data=bytes(b),
                              piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
                  for i, b in enumerate(held)]
        chunks.append(piece.EncodedChunk(pieces=pieces, chunk_idx=ci, k=k, m=m, chunk_size=B,
                                         padlen=k * B - len(data), original_chunk_size=len(data)))
        datas.append(data)
    got, checks = piece.decode_chunks_checked(chunks)
    assert got == b"".join(datas)
    assert [(c.consistent, c.first_bad_offset, c.bad_piece_idx, c.located) for c in checks] == [
        (True, None, [], False), (False, 40000, [2], True), (False, B - 1, [5], True)]
    got, checks = piece.reconstruct_data_checked([p for ch in chunks for p in ch.pieces], chunks)
    assert got == b"".join(datas) and [c.located for c in checks] == [False, True, True]
    assert pinned_bytes()[0] == 0
