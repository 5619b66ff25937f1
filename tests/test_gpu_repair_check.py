"""GPU: sec_repair_check_batch against expectations that never come from another HIP path.  Blocks
= cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c); corruptions are single flipped bytes put
into the buffer image in numpy.  The expected targets are cfec.easy_encode(cfec.easy_decode(the
first k entries AS HELD, flips included, bytes past an entry's avail zero))[target]; the expected
digests hashlib.sha1 of those; the expected results follow from where the test put the flips, as in
tests/test_gpu_decode_check.py: a flip in a check row flags that row and leaves the targets correct,
a flip in a basis block flags every check row (the code is MDS: every coefficient is nonzero) and
changes every target at that position.

Layout of every case: each entry sits in a buffer of 0xFF at odd and even starts, so a short entry
(block_avail < B) is followed by 0xFF bytes and a read past its avail shows up as a difference; the
buffer must be byte-identical after every call.  Every target sits at an odd or even address of its
own between 0xFF guard bytes in a buffer that is compared whole, so a store past B, or a 16-byte
store that straddles a neighbour, shows."""

import functools
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, RCHK_DTYPE, REP_DTYPE  # noqa: E402
from storb_amd.engine import Engine, Error, check_locate, pinned_bytes  # noqa: E402

UNTOUCHED = 0xEE  # row_bad / column / digests before the call


@functools.lru_cache(maxsize=None)
def _blocks(k, m, B, padlen, seed):
    """The oracle's m blocks of a seeded chunk of k*B - padlen bytes (block k-1 zero-padded)."""
    n = k * B - padlen
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes() + b"\0" * padlen
    blocks = cfec.easy_encode(data, k, m)
    assert len(blocks) == m and all(len(b) == B for b in blocks)
    return blocks


def spec(k, m, B, entries, targets, flips=(), padlen=0, short=False, seed=None):
    """One chunk: blocks `entries` held, the first k repaired from (and the check's basis), the rest
    the check rows; blocks `targets` regenerated, in that order.  flips: (entry position, byte
    position) of bytes XORed with 0x5A.  short: block k-1, wherever it is among the entries, is
    handed over with block_avail = B - padlen."""
    assert len(set(entries)) == len(entries) >= k and not set(entries) & set(targets)
    return dict(k=k, m=m, B=B, entries=list(entries), targets=list(targets), flips=list(flips), padlen=padlen,
                short=short, seed=seed if seed is not None else 1000 * k + m + B)


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


@functools.lru_cache(maxsize=None)
def _oracle_targets(k, m, entries, targets, basis):
    """The oracle's blocks `targets` of the code word that the basis as held spans."""
    full = cfec.easy_encode(cfec.easy_decode(list(basis), list(entries), 0, k, m), k, m)
    return [full[t] for t in targets]


def _expected_targets(s, held):
    k, B = s["k"], s["B"]
    basis = tuple(bytes(h) + b"\0" * (B - len(h)) for h in held[:k])
    return _oracle_targets(k, s["m"], tuple(s["entries"][:k]), tuple(s["targets"]), basis)


def _layout(specs):
    """The buffer image, the call's arrays (offsets relative to the buffers), the expected image of
    the target buffer, the expected digests and, per chunk, what the check must report."""
    descs = np.zeros(len(specs), dtype=RCHK_DTYPE)
    sn, bo, av, tn, to, want, parts, outs = [], [], [], [], [], [], [], []
    cur, ocur = 3, 7
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        held, avail = _held(s)
        descs[i] = (B, len(sn), len(tn), len(s["targets"]), n, k, s["m"])
        for j, (t, exp) in enumerate(zip(s["targets"], _expected_targets(s, held))):
            assert len(exp) == B
            tn.append(t)
            to.append(ocur)
            outs.append((ocur, exp))
            ocur += B + 9 + (j + i) % 2  # guard bytes between the targets, odd and even starts
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
    dig = np.full(20 * len(tn) + 12, UNTOUCHED, np.uint8)
    for j, (o, b) in enumerate(outs):
        out[o:o + len(b)] = np.frombuffer(b, np.uint8)
        dig[20 * j:20 * j + 20] = np.frombuffer(hashlib.sha1(b).digest(), np.uint8)
    return SimpleNamespace(descs=descs, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), tn=np.array(tn, np.int32), to=np.array(to, np.uint64),
                           src=src, out=out, dig=dig, want=want, specs=specs)


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


def _diff(what, got, want):
    d = np.flatnonzero(got != want)
    return f"{what} differs at {d[:8].tolist()} ({d.size} bytes)" if d.size else ""


def run_device(engine, L, dsrc=None, asynchronous=False, use_avail=True, outputs=True, digests=True):
    nslots = len(L.sn)
    if dsrc is None:
        dsrc = torch.from_numpy(L.src).cuda()
    dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
    ddig = torch.full((L.dig.size,), UNTOUCHED, dtype=torch.uint8, device="cuda") if digests else None
    res = torch.zeros(16 * len(L.specs), dtype=torch.uint8, device="cuda")
    rb = torch.full((max(nslots, 1),), UNTOUCHED, dtype=torch.uint8, device="cuda") if outputs else None
    col = torch.full((max(nslots, 1),), UNTOUCHED, dtype=torch.uint8, device="cuda") if outputs else None
    engine.repair_check_batch(L.descs, L.sn, L.bo + np.uint64(dsrc.data_ptr()), 0, L.tn, L.to, dout, res,
                              block_avail=L.av if use_avail else None, digests=ddig, row_bad=rb, column=col,
                              asynchronous=asynchronous)
    if asynchronous:
        engine.sync()
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    assert not _diff("out", dout.cpu().numpy(), L.out)
    if digests:
        assert not _diff("digests", ddig.cpu().numpy(), L.dig)
    _verify(L, res.cpu().numpy(), rb.cpu().numpy() if outputs else None, col.cpu().numpy() if outputs else None)
    return dsrc, dout, res, rb, col, ddig


# RS(4,6) with piece 1 lost: repaired from blocks {0, 2, 3, 4}, block 5 the one spare.  One store row and
# one compare row share a tile over the 4-slot batch.
E46, T46 = [0, 2, 3, 4, 5], [1]


# ---- device mode ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 4101, 65536 + 16])
def test_block_sizes_clean_and_single_flips(engine, B):
    """The tail kernel only (B < 16), exactly one lane, one clamped lane, a ragged last tile,
    several tiles.  Clean; one flip in the check row (middle, byte 0, last byte); one in a basis
    block (last byte, byte 0)."""
    s = spec(4, 6, B, E46, T46)
    run_device(engine, _layout([s, flipped(s, (4, B // 2)), flipped(s, (4, 0)), flipped(s, (4, B - 1)),
                                flipped(s, (1, B - 1)), flipped(s, (0, 0)), flipped(s, (3, B // 3))]), use_avail=False)


# zfec(10,14), B = 6554, padlen 4: block 9 handed over with avail = B - 4 and 0xFF behind it
Z1014_BASIS_SHORT = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 9, 8, 4, 12, 10], [7, 1], padlen=4, short=True)
Z1014_ROW_SHORT = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 1, 8, 4, 9, 12], [10, 7], padlen=4, short=True)
# ... and block 9 lost: regenerated with its zero padding, beside parity block 13
Z1014_LAST_LOST = spec(10, 14, 6554, [8, 0, 2, 3, 11, 5, 6, 1, 7, 4, 10, 12], [9, 13], padlen=4)


@pytest.mark.parametrize("s,short_at", [(Z1014_BASIS_SHORT, 7), (Z1014_ROW_SHORT, 10), (Z1014_LAST_LOST, None)],
                         ids=["basis-short", "row-short", "last-lost"])
def test_short_last_data_block(engine, s, short_at):
    """Block k-1 in place from the chunk buffer, once as a basis entry and once as a check row: the
    positions [B - 4, B) are the ragged end.  Flips at 0, at 6549 (the short entry's last byte in
    memory) and at 6553 of full-length entries.  Block k-1 as a target keeps its zero padding."""
    n = len(s["entries"])
    full_basis, full_row = 1, n - 1
    assert short_at not in (full_basis, full_row)
    specs = [s, flipped(s, (full_basis, 6553)), flipped(s, (full_row, 6553)), flipped(s, (full_row, 6549))]
    if short_at is not None:
        specs += [flipped(s, (short_at, 0)), flipped(s, (short_at, 6549))]
    else:
        want9 = _expected_targets(s, _held(s)[0])[0]
        assert want9[-4:] == b"\0" * 4 and want9 == _blocks(10, 14, 6554, 4, s["seed"])[9]
    run_device(engine, _layout(specs))


Z1014_3T = spec(10, 14, 4101, [13, 0, 2, 3, 11, 5, 6, 9, 8, 4, 12], [7, 10, 1])  # 3 targets + 1 spare: one group
# k = 20, m = 40: 12 targets + 8 spares = 20 rows over the wide-k loop in three row groups: stores only,
# 4 stores + 4 compares, compares only
_B2040 = [39, 0, 2, 22, 4, 5, 6, 31, 8, 9, 10, 11, 27, 13, 14, 15, 16, 35, 18, 19]
_S2040 = [20, 1, 38, 3, 25, 12, 33, 17]
_T2040 = [s for s in range(40) if s not in _B2040 + _S2040][::-1]
Z2040 = spec(20, 40, 4101, _B2040 + _S2040, _T2040)


def test_row_groups_16_slot_batch(engine):
    s = Z1014_3T
    run_device(engine, _layout([s, flipped(s, (10, 4100)), flipped(s, (4, 2050))]))


def test_row_groups_wide_k_three_groups(engine):
    """A flip in a spare of the mixed group (check row 1), one in a spare of the compare-only group
    (check row 6), one in a basis block, which flags all eight."""
    s = Z2040
    assert len(s["targets"]) == 12 and len(s["entries"]) == 28
    run_device(engine, _layout([s, flipped(s, (20 + 1, 4098)), flipped(s, (20 + 6, 17)), flipped(s, (9, 2050))]))


def _degenerate(corrupt):
    """Plain checks (no target), plain repairs (n == k), chunks with neither, and full ones between."""
    specs = [spec(4, 6, 4101, [0, 2, 3, 4, 5, 1], []),                 # ntargets == 0: a check, two rows
             spec(4, 6, 4101, [5, 0, 3, 2], [4, 1]),                   # n == k: a repair
             spec(4, 6, 4101, [5, 0, 3, 2], []),                       # both: nothing to launch
             spec(4, 6, 17, E46, T46),
             spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 9, 8, 4, 12, 10], [], padlen=4, short=True),
             spec(4, 6, 7, [3, 0, 5, 2], [1], padlen=2, short=True),   # the tail kernel, a short basis entry
             spec(4, 6, 9, [3, 0, 5, 2], []),                          # both, in the tail range
             Z1014_3T]
    flips = {0: (1, 4000), 1: (2, 5), 3: (4, 16), 4: (11, 6000), 5: (0, 3), 7: (10, 77)}
    return [flipped(s, flips[i]) if i in corrupt else s for i, s in enumerate(specs)]


def test_degenerate_forms_twice_from_the_cached_plan(engine):
    """The second and third calls reuse the plan on data changed in place: chunks healed, others
    corrupted.  Their results must be the new data's (no flag left over from the call before)."""
    L1, L2, L3 = _layout(_degenerate({0, 3, 5})), _layout(_degenerate({1, 4, 7})), _layout(_degenerate(set()))
    assert L1.descs.tobytes() == L2.descs.tobytes() and np.array_equal(L1.bo, L2.bo) and np.array_equal(L1.to, L2.to)
    dsrc = run_device(engine, L1)[0]
    dsrc.copy_(torch.from_numpy(L2.src))
    run_device(engine, L2, dsrc)
    dsrc.copy_(torch.from_numpy(L3.src))
    run_device(engine, L3, dsrc)


def test_nothing_to_launch_alone(engine):
    """A call whose every chunk has neither a target nor a check row: consistent, nothing written."""
    run_device(engine, _layout([spec(4, 6, 4101, [5, 0, 3, 2], []), spec(4, 6, 3, [0, 1, 2, 3], [])]))


def _mixed(corrupt):
    specs = [Z1014_BASIS_SHORT, spec(4, 6, 17, E46, T46), Z1014_3T, spec(4, 6, 7, [3, 0, 5, 2, 4], [1], padlen=2, short=True),
             Z2040, spec(4, 6, 33001, [5, 0, 3, 2, 4], [1]), Z1014_LAST_LOST]
    flips = {0: (11, 6000), 1: (2, 16), 2: (10, 4100), 3: (4, 6), 4: (22, 2054), 5: (4, 32999), 6: (4, 1)}
    return [flipped(s, flips[i]) if i in corrupt else s for i, s in enumerate(specs)]


def test_async_then_sync(engine):
    run_device(engine, _layout(_mixed({0, 5})), asynchronous=True)


def test_row_bad_and_column_null(engine):
    run_device(engine, _layout(_mixed({2, 4})), outputs=False)


def test_results_alone(engine):
    """digests, row_bad and column are optional."""
    res = run_device(engine, _layout(_mixed({2})), outputs=False, digests=False)[2]
    res = np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)
    assert [int(r["first"]) for r in res] == [CHK_CONSISTENT] * 2 + [4100] + [CHK_CONSISTENT] * 4
    assert [int(r["nbad"]) for r in res] == [0, 0, 1, 0, 0, 0, 0]


def test_same_as_repair_then_check(engine):
    """For the same arrays the targets and digests equal sec_repair_batch's and the results
    sec_check_batch's: every shape of this file, clean and corrupt."""
    L = _layout(_mixed({0, 1, 4, 6}) + _degenerate({0, 1, 5}) + [Z1014_ROW_SHORT, flipped(Z2040, (3, 9))])
    dsrc, dout, res, rb, col, ddig = run_device(engine, L)
    offs = L.bo + np.uint64(dsrc.data_ptr())
    rep = np.zeros(len(L.specs), dtype=REP_DTYPE)
    chk = np.zeros(len(L.specs), dtype=CHK_DTYPE)
    for i, d in enumerate(L.descs):
        rep[i] = (d["B"], d["slot0"], d["tgt0"], d["ntargets"], d["k"], d["m"], 0)
        chk[i] = (d["B"], d["slot0"], d["n"], d["k"], d["m"], 0)
    dout2, ddig2 = torch.full_like(dout, 0xFF), torch.full_like(ddig, UNTOUCHED)
    engine.repair_batch(rep, L.sn, offs, 0, L.tn, L.to, dout2, block_avail=L.av, digests=ddig2)
    res2, rb2, col2 = torch.zeros_like(res), torch.full_like(rb, UNTOUCHED), torch.full_like(col, UNTOUCHED)
    engine.check_batch(chk, L.sn, offs, 0, res2, block_avail=L.av, row_bad=rb2, column=col2)
    assert torch.equal(dout, dout2) and torch.equal(ddig, ddig2)
    assert torch.equal(res, res2) and torch.equal(rb, rb2) and torch.equal(col, col2)


def test_timing_kind_repair_check(engine):
    engine.set_timing(True)
    try:
        for kind in ("repair_check", "repair", "check", "decode_check"):
            engine.collect_timing(kind)
        run_device(engine, _layout([Z1014_3T, spec(4, 6, 7, [3, 0, 5, 2, 4], [1])]))
        ms, launches = engine.collect_timing("repair_check")
        assert launches == 1 and ms > 0
        for kind in ("repair", "check", "decode_check"):
            assert engine.collect_timing(kind) == (0.0, 0), kind
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    """Each error code in the documented order; nothing is touched: `out`, the digests and the
    results stay as they were (the block addresses handed over do not exist)."""
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=RCHK_DTYPE)
    d[0] = (64, 0, 0, 1, 5, 4, 6)
    bo = np.zeros(8, np.uint64)  # never dereferenced: every call fails first
    to = np.zeros(4, np.uint64)
    out = torch.full((256,), 0xFF, dtype=torch.uint8, device="cuda")
    dig = torch.full((80,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    res = torch.full((16,), 0x77, dtype=torch.uint8, device="cuda")

    def call(sn, tn=(1,), flags=0, desc=d, results=True, offs=True, tnums=True, toffs=True):
        sn = None if sn is None else np.array(sn, np.int32)
        tn = np.array(tn, np.int32)
        return lib.sec_repair_check_batch(ctx, desc.ctypes.data, 1, None if sn is None else sn.ctypes.data,
                                          bo.ctypes.data if offs else None, None, None,
                                          tn.ctypes.data if tnums else None, to.ctypes.data if toffs else None,
                                          out.data_ptr(), dig.data_ptr(), res.data_ptr() if results else None, None,
                                          None, flags)

    def desc(**kw):
        bad = d.copy()
        for f, v in kw.items():
            bad[f] = v
        return bad

    ok = [0, 2, 3, 4, 5]
    for flags in (_lib.SEC_F_STAGED | _lib.SEC_F_HOST, _lib.SEC_F_GPU_PARITY_IDS, _lib.SEC_F_RECOVER,
                  _lib.SEC_F_HOST | _lib.SEC_F_ASYNC):
        assert call(ok, flags=flags) == _lib.SEC_EINVAL
    assert call(None) == _lib.SEC_EINVAL
    assert call(ok, offs=False) == _lib.SEC_EINVAL
    assert call(ok, results=False) == _lib.SEC_EINVAL
    assert call(ok, tnums=False) == _lib.SEC_EINVAL
    assert call(ok, toffs=False) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(ntargets=-1)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1, k=5, m=4)) == _lib.SEC_EINVAL  # before SEC_EKM
    assert call(ok, desc=desc(ntargets=-1, k=5, m=4)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(k=5, m=4)) == _lib.SEC_EKM
    assert call(ok, desc=desc(k=0)) == _lib.SEC_EKM
    assert call(ok, desc=desc(m=257)) == _lib.SEC_EKM
    assert call(ok, desc=desc(k=7, m=6, n=3)) == _lib.SEC_EKM  # before SEC_ENBLOCKS
    assert call(ok, desc=desc(n=3)) == _lib.SEC_ENBLOCKS
    assert call(ok + [1, 9], tn=(8,), desc=desc(n=7)) == _lib.SEC_ENBLOCKS  # n > m, before SEC_ESHARENUM
    assert call([0, 2, 3, 4, 6]) == _lib.SEC_ESHARENUM
    assert call([0, 2, 3, 4, -1]) == _lib.SEC_ESHARENUM
    assert call(ok, tn=(6,)) == _lib.SEC_ESHARENUM  # a target outside [0, m)
    assert call(ok, tn=(-1,)) == _lib.SEC_ESHARENUM
    assert call([0, 0, 3, 4, 5], tn=(6,)) == _lib.SEC_ESHARENUM  # before SEC_EDUPSHARE
    assert call([0, 2, 2, 4, 5]) == _lib.SEC_EDUPSHARE  # within the basis
    assert call([0, 2, 3, 4, 3]) == _lib.SEC_EDUPSHARE  # a check row that is a basis block
    assert call([0, 2, 3, 4], tn=(1, 1), desc=desc(n=4, ntargets=2)) == _lib.SEC_EDUPSHARE  # a repeated target
    assert call(ok, tn=(5,)) == _lib.SEC_EDUPSHARE  # a target held as a check row
    assert call(ok, tn=(3,)) == _lib.SEC_EDUPSHARE  # a target held in the basis
    assert call(ok, tn=(3,), desc=desc(B=1 << 31)) == _lib.SEC_EDUPSHARE  # before SEC_ESIZE
    assert call(ok, desc=desc(B=1 << 31)) == _lib.SEC_ESIZE
    assert (out.cpu() == 0xFF).all() and (dig.cpu() == UNTOUCHED).all() and (res.cpu() == 0x77).all()


# ---- host mode --------------------------------------------------------------------------
def run_host(eng, L, src=None):
    nslots = len(L.sn)
    src = L.src.copy() if src is None else src
    out = np.full(L.out.size, 0xFF, np.uint8)
    dig = np.full(L.dig.size, UNTOUCHED, np.uint8)
    res = np.zeros(len(L.specs), dtype=CHK_RESULT_DTYPE)
    rb, col = np.full(nslots, UNTOUCHED, np.uint8), np.full(nslots, UNTOUCHED, np.uint8)
    eng.repair_check_batch(L.descs, L.sn, L.bo, src, L.tn, L.to, out, res, block_avail=L.av, digests=dig, row_bad=rb,
                           column=col, host=True)
    assert np.array_equal(src, L.src), "the source buffer was written"
    assert not _diff("out", out, L.out)
    assert not _diff("digests", dig, L.dig)
    _verify(L, res, rb, col)


def test_host_numpy_buffers_are_staged(engine):
    z0, r0, s0 = engine.host_paths()
    run_host(engine, _layout(_mixed({0, 3, 5}) + _degenerate({0, 5})))
    assert engine.host_paths() == (z0, r0, s0 + 1)  # never zero-copy, never page-locked
    assert pinned_bytes()[0] == 0  # the slabs went back to the pool
    run_host(engine, _layout(_mixed({2}) + _degenerate({1})))  # the cached plan, other data


def test_host_several_slabs():
    """The staging pipeline over more slabs than it has slots: 64 KiB slabs, so every chunk of the
    mix but the small ones is a slab of its own (targets, digests and results scattered per slab)."""
    eng = Engine(0, options={"SEC_SLAB_BYTES": 1 << 16, "SEC_SLAB_BYTES_DIGEST": 1 << 16})
    try:
        run_host(eng, _layout(_mixed({0, 2, 4, 5}) + _degenerate({0, 1})))
        assert eng.host_paths() == (0, 0, 1)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_repair_check_host_from_bytes(engine):
    specs = _mixed({0, 2, 5}) + _degenerate({0, 1})
    items, want = [], []
    for s in specs:
        held, _ = _held(dict(s, short=False))
        items.append((s["k"], s["m"], [bytes(b) for b in held], s["entries"], s["targets"]))
        want.append(_expected_targets(s, held))
    out, digs, checks = engine.repair_check_host(items, digests=True)
    assert out == want
    assert digs == [[hashlib.sha1(b).digest() for b in row] for row in want]
    for (k, m, blocks, entries, _), s, (first, bad, column) in zip(items, specs, checks):
        if not s["flips"] or len(entries) == k:
            assert (first, bad, column) == (None, [], None)
            continue
        (e, p), = s["flips"]
        assert first == p and column == bytes(b[p] for b in blocks)
        assert bad == (list(range(k, len(entries))) if e < k else [e])
    out2, checks2 = engine.repair_check_host(items)
    assert out2 == want and checks2 == checks
    assert engine.repair_check_host([]) == ([], []) and engine.repair_check_host([], digests=True) == ([], [], [])
    assert pinned_bytes()[0] == 0
    with pytest.raises(Error):
        engine.repair_check_host([(4, 6, [b"ab"] * 5, [0, 2, 3, 4, 4], [1])])
    with pytest.raises(Error):
        engine.repair_check_host([(4, 6, [b"ab"] * 5, [0, 2, 3, 4, 5], [5])])


def test_repair_chunks_checked_end_to_end():
    """piece.repair_chunks_checked on 256 KiB chunks: RS(4,6) with every piece held and a byte of a
    data piece flipped (one corrupt survivor, two spares: located, and its replacement is what
    comes back); zfec(4,7) with piece 1 lost and a survivor that is repaired from corrupt (the lost
    piece is regenerated from the pieces that passed, the replacement appended); a clean RS(4,6)
    with piece 5 lost.  Expected pieces are the oracle's encode of the chunks themselves."""
    n, k = 256 << 10, 4
    B = -(-n // k)
    chunks, blocks_of = [], []
    for ci, (m, lost, bad_idx, at) in enumerate([(6, (), 2, 40000), (7, (1,), 3, B - 1), (6, (5,), None, 0)]):
        data = np.random.default_rng(500 + ci).integers(0, 256, n - ci, dtype=np.uint8).tobytes()
        blocks = cfec.easy_encode(data, k, m)
        held = [bytearray(b) for b in blocks]
        if bad_idx is not None:
            held[bad_idx][at] ^= 0x01
        pieces = [piece.Piece(chunk_idx=ci, piece_idx=i, data=bytes(b),
                              piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
                  for i, b in enumerate(held) if i not in lost]
        chunks.append(piece.EncodedChunk(pieces=pieces, chunk_idx=ci, k=k, m=m, chunk_size=B,
                                         padlen=k * B - len(data), original_chunk_size=len(data)))
        blocks_of.append(blocks)
    got, checks = piece.repair_chunks_checked(chunks, piece_ids=True)
    assert [(c.consistent, c.first_bad_offset, c.bad_piece_idx, c.located) for c in checks] == [
        (False, 40000, [2], True), (False, B - 1, [3], True), (True, None, [], False)]
    assert [[p.piece_idx for p in row] for row in got] == [[2], [1, 3], [5]]
    for row, blocks in zip(got, blocks_of):
        for p in row:
            assert p.data == blocks[p.piece_idx] and p.piece_id == hashlib.sha1(blocks[p.piece_idx]).hexdigest()
    one, ck = piece.repair_pieces_checked(chunks[2])
    assert [(p.piece_idx, p.data) for p in one] == [(5, blocks_of[2][5])] and ck.consistent
    assert pinned_bytes()[0] == 0
