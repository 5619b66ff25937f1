"""GPU: the bit-sliced repair kernel (sec_repair_bs_kernel) under sec_repair_batch and
sec_repair_check_batch, against expectations that never come from another HIP path.  Blocks =
cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c): target t must equal blocks[t] and its digest
hashlib.sha1(blocks[t]).  Corruptions are single flipped bytes put into the buffer image in numpy.  A
flip in a held parity piece flags that row only and leaves the targets alone; a flip in a data piece
flags every held check row (the code is MDS: no parity coefficient is zero) and the targets are then
the oracle's encode OF THE DATA AS HELD (cfec.easy_encode(cfec.easy_decode(the first k entries as
held))[t]): targets are written whether or not the chunk is consistent.

Layout, as tests/test_gpu_repair.py: each target sits at an offset of 1 or 33 modulo 64 between runs
of 0xA5 of at least 64 bytes, and the target buffer is compared whole; each source sits in an arena
of 0xFF at odd and even starts, block k-1 is handed over with block_avail = B - 3 (0xFF behind it), and
the source image must be byte-identical after every call.

Every case runs under SEC_CHECK_BS = 1 and = 0, as a plain repair from the chunk's first k entries
and as a repair + check of all its entries, and every run is compared with the oracle.  Under 1 the
context's bit-sliced repair counter must rise by exactly the eligible chunks (on a build without the
kernel there is no such counter: those assertions are what fails there), under 0 the direct one."""

import functools
import hashlib
import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, CHK_RESULT_DTYPE, RCHK_DTYPE, REP_DTYPE  # noqa: E402
from storb_amd.engine import Engine, check_locate, pinned_bytes, repair_method  # noqa: E402

GUARD = 0xA5
UNTOUCHED = 0xEE  # row_bad / column / digests before the call
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


def spec(k, m, B, entries, targets, flips=(), seed=None):
    """One chunk: blocks `entries` held, the first k repaired from (and the check's basis), the rest
    the check rows; blocks `targets` regenerated, in that order.  flips: (entry position, byte
    position) of bytes XORed with 0x5A.  Block k-1, wherever it is among the entries, is handed over
    with block_avail = B - PADLEN (B >= 16) and 0xFF behind it."""
    assert len(set(entries)) == len(entries) >= k and not set(entries) & set(targets)
    return dict(k=k, m=m, B=B, entries=list(entries), targets=list(targets), flips=list(flips),
                padlen=PADLEN if B > PADLEN else 0, seed=seed if seed is not None else 1000 * k + m + B)


def flipped(s, *flips):
    return dict(s, flips=list(flips))


def eligible(s):
    k, e = s["k"], s["entries"]
    return ((k, s["m"]) in SHAPES and s["B"] >= 16 and len(s["targets"]) >= 1
            and sorted(e[:k]) == list(range(k)))


def _held(s):
    """The chunk's entries as held (flips applied, block k-1 cut at its avail) and their avail."""
    k, B = s["k"], s["B"]
    blocks = _blocks(k, s["m"], B, s["padlen"], s["seed"])
    held, avail = [], []
    for b in s["entries"]:
        a = B - s["padlen"] if b == k - 1 else B
        held.append(bytearray(blocks[b][:a]))
        avail.append(a)
    for e, p in s["flips"]:
        assert p < avail[e], "a flip must land on a byte that is in memory"
        held[e][p] ^= 0x5A
    return held, avail


@functools.lru_cache(maxsize=None)
def _oracle_targets(k, m, basis_nums, targets, basis):
    """The oracle's blocks `targets` of the code word that the basis as held spans."""
    full = cfec.easy_encode(cfec.easy_decode(list(basis), list(basis_nums), 0, k, m), k, m)
    return [full[t] for t in targets]


def _expected_targets(s, held):
    k, B = s["k"], s["B"]
    basis = tuple(bytes(h) + b"\0" * (B - len(h)) for h in held[:k])
    return _oracle_targets(k, s["m"], tuple(s["entries"][:k]), tuple(s["targets"]), basis)


def _layout(specs):
    """The source image, both calls' arrays (offsets relative to the two buffers), the expected
    image of the target buffer, the expected digests and, per chunk, what the check must report."""
    rep = np.zeros(len(specs), dtype=REP_DTYPE)
    rchk = np.zeros(len(specs), dtype=RCHK_DTYPE)
    sn, bo, av, tn, to, want, parts, outs = [], [], [], [], [], [], [], []
    cur, tcur = 3, 0
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        held, avail = _held(s)
        rep[i] = (B, len(sn), len(tn), len(s["targets"]), k, s["m"], 0)
        rchk[i] = (B, len(sn), len(tn), len(s["targets"]), n, k, s["m"])
        exp = _expected_targets(s, held)
        if not any(e < k for e, _ in s["flips"]):  # the basis is clean: the chunk's own blocks
            assert exp == [_blocks(k, s["m"], B, s["padlen"], s["seed"])[t] for t in s["targets"]]
        for t, x in zip(s["targets"], exp):
            assert len(x) == B
            start = tcur + 64
            start += (1 + 32 * (len(tn) % 2) - start) % 64  # 1 or 33 modulo 64
            tn.append(t)
            to.append(start)
            outs.append((start, x))
            tcur = start + B
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
            want.append(None)  # (n == k: nothing to check, consistent whatever the bytes)
    src = np.full(cur + 64, 0xFF, np.uint8)
    for o, b in parts:
        src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    tgt = np.full(tcur + 64, GUARD, np.uint8)
    dig = np.full(20 * len(tn) + 12, UNTOUCHED, np.uint8)
    for j, (o, b) in enumerate(outs):
        tgt[o:o + len(b)] = np.frombuffer(b, np.uint8)
        dig[20 * j:20 * j + 20] = np.frombuffer(hashlib.sha1(b).digest(), np.uint8)
    with_target = [s for s in specs if s["targets"]]
    return SimpleNamespace(rep=rep, rchk=rchk, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), tn=np.array(tn, np.int32), to=np.array(to, np.uint64),
                           src=src, tgt=tgt, dig=dig, want=want, specs=specs,
                           eligible=sum(eligible(s) for s in with_target),
                           direct=sum(not eligible(s) for s in with_target))


def _verify(L, res, rb, col, what, checks):
    res = np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=CHK_RESULT_DTYPE)
    for i, (s, w) in enumerate(zip(L.specs, L.want)):
        s0, n, k = int(L.rchk[i]["slot0"]), len(s["entries"]), s["k"]
        tag = f"{what}, chunk {i}"
        if w is None or not checks:
            if checks:
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


def _diff(what, got, want):
    d = np.flatnonzero(got != want)
    assert d.size == 0, f"{what} differs at {d[:8].tolist()} ({d.size} bytes)"


def _call(engine, L, src, checks, digests, host=False):
    """One call; src: the device (or, host mode, numpy) source image.  -> (targets, digests, results,
    row_bad, column) as numpy."""
    nslots = len(L.sn)
    if host:
        new = lambda a: a.copy()  # noqa: E731
        offs, toffs, blocks = L.bo, L.to, src
    else:
        new = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        offs, toffs, blocks = L.bo + np.uint64(src.data_ptr()), L.to, 0
    tgt = new(np.full(L.tgt.size, GUARD, np.uint8))
    dig = new(np.full(L.dig.size, UNTOUCHED, np.uint8)) if digests else None
    res = new(np.zeros(16 * len(L.specs), np.uint8))
    rb = new(np.full(max(nslots, 1), UNTOUCHED, np.uint8))
    col = new(np.full(max(nslots, 1), UNTOUCHED, np.uint8))
    if checks:
        engine.repair_check_batch(L.rchk, L.sn, offs, blocks, L.tn, toffs, tgt, res, block_avail=L.av, digests=dig,
                                  row_bad=rb, column=col, host=host)
    else:
        engine.repair_batch(L.rep, L.sn, offs, blocks, L.tn, toffs, tgt, block_avail=L.av, digests=dig, host=host)
    get = (lambda a: a) if host else (lambda a: a.cpu().numpy())
    return get(tgt), None if dig is None else get(dig), get(res), get(rb), get(col)


def run_four(engine, specs, digests=False, host=False):
    """A plain repair and a repair + check under SEC_CHECK_BS = 1 and = 0, each against the oracle."""
    L = _layout(specs)
    src = L.src.copy() if host else torch.from_numpy(L.src).cuda()
    for opt in (1, 0):
        with engine.options(SEC_CHECK_BS=opt):
            for checks in (False, True):
                what = f"SEC_CHECK_BS={opt} {'repair + check' if checks else 'repair'}"
                b0, d0 = engine.repair_methods()
                c0 = engine.check_methods()
                tgt, dig, res, rb, col = _call(engine, L, src, checks, digests, host)
                b1, d1 = engine.repair_methods()
                assert (b1 - b0, d1 - d0) == ((L.eligible, L.direct) if opt else (0, L.eligible + L.direct)), what
                assert engine.check_methods() == c0, f"{what}: counted as a check"
                _diff(f"{what}: the target buffer", tgt, L.tgt)
                if digests:
                    _diff(f"{what}: digests", dig, L.dig)
                _verify(L, res, rb, col, what, checks)
    _diff("the source buffer (it was written)", src if host else src.cpu().numpy(), L.src)
    for s in specs:  # the host function agrees with what the counters were held to
        assert repair_method(s["k"], s["m"], s["entries"], s["targets"], s["B"], avail=_held(s)[1]) == (
            (s["k"], s["m"]) in SHAPES and s["B"] >= 16 and sorted(s["entries"][:s["k"]]) == list(range(s["k"]))
            and len(s["targets"]) + len(s["entries"]) - s["k"] >= 1)
    return L


def _rng(k, m, B):
    return random.Random(k * 100003 + m * 101 + B)


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("k,m", SHAPES)
def test_shapes_and_sizes(engine, k, m, B):
    """Shuffled data basis.  Targets: every parity row (nothing held); the first row with every
    other row held; the last row with a strict subset held; a random subset with a random subset of
    the rest held.  On the second: clean, one flipped byte in a held parity piece at 0, B-1, 2047 /
    2048 where B allows and in the overlap of the moved-back last piece, one in a data piece (every
    held row bad, the targets the encode of the data as held), block k-1's last byte in memory, and
    two flips in different pieces."""
    rng = _rng(k, m, B)
    basis = rng.sample(range(k), k)
    parity = list(range(k, m))
    everything = spec(k, m, B, basis, rng.sample(parity, m - k))
    first = spec(k, m, B, basis + rng.sample(parity[1:], m - k - 1), [k])
    some = rng.sample(parity[:-1], rng.randint(1, m - k - 2))
    last = spec(k, m, B, basis + some, [m - 1])
    tg = rng.sample(parity, rng.randint(2, m - k - 1))
    rest = [r for r in parity if r not in tg]
    subset = spec(k, m, B, basis + rng.sample(rest, rng.randint(1, len(rest))), tg)
    n = m - 1
    at = [0, B - 1] + [p for p in (2047, 2048) if p < B]
    if B % 16:  # the last unclamped piece's last byte: the piece moved back to end at B holds it too
        at.append(B // 16 * 16 - 1)
    cases = [everything, first, last, subset] + [flipped(first, (k + i % (n - k), p)) for i, p in enumerate(at)]
    not_last = next(j for j in range(k) if basis[j] != k - 1)
    cases.append(flipped(first, (not_last, B // 2)))
    cases.append(flipped(subset, (basis.index(k - 1), B - PADLEN - 1)))  # block k-1's last byte in memory
    cases.append(flipped(everything, (not_last, B - 1)))  # nothing held: consistent, targets of the data as held
    cases.append(flipped(first, (k, B - 2), (k + 1, 5)))
    cases.append(flipped(last, (k + len(some) - 1, B - 1), (not_last, 7)))
    L = run_four(engine, cases)
    assert L.eligible == len(cases) and L.direct == 0


def test_target_sets_and_row_groups(engine):
    """zfec(64,96): targets in group 0 only, in group 1 only and in both, with nothing held, with
    rows held in the other group only and in both.  zfec(16,24): exactly 8 targets and exactly 1.
    zfec(32,48): 16 targets in one group.  With digests."""
    B = 4096 + 21
    rng = random.Random(96)
    basis = rng.sample(range(64), 64)
    g0, g1 = list(range(64, 80)), list(range(80, 96))
    cases = []
    for tg, held in ((rng.sample(g0, 5), []), (rng.sample(g1, 7), []), (rng.sample(g0, 3) + rng.sample(g1, 3), []),
                     (g0[:8], rng.sample(g1, 4)), (g1[8:], rng.sample(g0, 4)), ([64, 95], [65, 94, 70, 88]),
                     (rng.sample(g0 + g1, 32), []), ([95], g0 + g1[:-1])):
        s = spec(64, 96, B, basis + held, tg)
        cases.append(s)
        if held:
            cases += [flipped(s, (64 + len(held) - 1, B - 1)), flipped(s, (17, 2048))]
    b16 = rng.sample(range(16), 16)
    cases += [spec(16, 24, B, b16, rng.sample(range(16, 24), 8)), spec(16, 24, B, b16, [19]),
              spec(16, 24, B, b16 + [23, 16, 20], [19]), spec(32, 48, B, rng.sample(range(32), 32), list(range(32, 48)))]
    L = run_four(engine, cases, digests=True)
    assert L.eligible == len(cases)


def test_one_mixed_call(engine):
    """Two eligible chunks ((16,24) with three check rows, (64,96) plain), one whose basis holds a
    parity row, a narrow RS(4,2) chunk, a B = 8 chunk of a bit-sliced shape and a chunk with no
    target in one call: all right, the counters split (2, 3); twice, so the second call runs from
    the cached plan; one timed launch unit."""
    B = 4096 + 21
    rng = random.Random(1624)
    a = spec(16, 24, B, rng.sample(range(16), 16) + [17, 22, 20], [23, 16])
    lost = [s for s in range(24) if s not in (2, 9, 20)]  # primaries 2 and 9 lost: rows 16, 17 stand in
    b = spec(16, 24, B, lost[:16] + lost[16:], [9, 20, 2])
    c = spec(4, 6, B, [5, 0, 3, 2, 4], [1])
    d = spec(16, 24, 8, list(range(16)) + [16], [17, 23])
    e = spec(64, 96, 2048 + 7, rng.sample(range(64), 64), [95, 64, 80])
    f = spec(16, 24, B, list(range(16)) + [18], [])  # a plain check: direct, and not counted
    for specs in ([a, b, c, d, e, f], [flipped(a, (18, 4097)), flipped(b, (17, 33)), c, flipped(d, (16, 7)), e, f],
                  [flipped(a, (5, 2047)), flipped(b, (1, 0)), flipped(c, (4, B - 1)), d, flipped(e, (63, 2048)), f]):
        for _ in range(2):
            L = run_four(engine, specs, digests=True)
        assert (L.eligible, L.direct) == (2, 3)
    L = _layout([a, b, c, d, e, f])
    dsrc = torch.from_numpy(L.src).cuda()
    engine.set_timing(True)
    try:
        with engine.options(SEC_CHECK_BS=1):
            for checks, kind in ((False, "repair"), (True, "repair_check")):
                engine.collect_timing(kind)
                b0 = engine.repair_methods()
                _call(engine, L, dsrc, checks, True)
                ms, launches = engine.collect_timing(kind)
                assert launches == 1 and ms > 0, kind
                b1 = engine.repair_methods()
                assert (b1[0] - b0[0], b1[1] - b0[1]) == (2, 3)
    finally:
        engine.set_timing(False)


def test_default_rule_takes_only_what_cleared(engine):
    """SEC_CHECK_BS = -1 (repair_bs_rule): of five eligible chunks the two in rows the profile
    cleared go bit-sliced ((32,48) with all 16 parity pieces lost, B = 32 KiB; (16,24) with one lost
    and the seven others held, B = 64 KiB), and one lost piece of a plain repair, a block size below
    the measured ones and zfec(8,12) stay direct; the bytes are the oracle's either way."""
    rng = random.Random(3248)
    b32, b16 = rng.sample(range(32), 32), rng.sample(range(16), 16)
    specs = [spec(32, 48, 32 << 10, b32, list(range(32, 48))),
             spec(16, 24, 64 << 10, b16 + list(range(17, 24)), [16]),
             spec(16, 24, 64 << 10, b16, [16]),
             spec(32, 48, 4096 + 21, b32, list(range(32, 48))),
             spec(8, 12, 4096 + 21, list(range(8)), [8, 9, 10, 11])]
    L = _layout(specs)
    assert L.eligible == 5 and engine.option("SEC_CHECK_BS") == -1
    dsrc = torch.from_numpy(L.src).cuda()
    for checks, want in ((False, (1, 4)), (True, (2, 3))):  # (the plain repair sees no held row)
        b0, d0 = engine.repair_methods()
        tgt, dig, res, rb, col = _call(engine, L, dsrc, checks, True)
        b1, d1 = engine.repair_methods()
        assert (b1 - b0, d1 - d0) == want
        _diff("the target buffer", tgt, L.tgt)
        _diff("digests", dig, L.dig)
        _verify(L, res, rb, col, "default rule", checks)


@pytest.mark.parametrize("k,m", [(16, 24), (32, 48)], ids=["register-ring", "lds-ring"])
def test_host_mode(engine, k, m):
    """SEC_F_HOST (staged: every entry B long in the slab), one shape per ring type, with digests."""
    B = 4096 + 21
    rng = _rng(k, m, B)
    basis = rng.sample(range(k), k)
    s = spec(k, m, B, basis + [m - 1, k + 1], [k, m - 2, k + 2])
    specs = [s, flipped(s, (k, B - 1)), flipped(s, (3, 2048)), spec(k, m, B, basis, list(range(k, m)))]
    z0, r0, s0 = engine.host_paths()
    L = run_four(engine, specs, digests=True, host=True)
    assert L.eligible == 4
    assert engine.host_paths() == (z0, r0, s0 + 4)  # always staged
    assert pinned_bytes()[0] == 0


def test_piece_api_end_to_end(monkeypatch):
    """piece.repair_chunks and repair_chunks_checked on a (16,24) chunk that lost three parity
    pieces, on an engine made with SEC_CHECK_BS = 1: choose_blocks picks the data pieces, so both
    calls go down the bit-sliced kernel; bytes and ids against the oracle."""
    k, m, n = 16, 24, 16 * 5000 - 11
    data = np.random.default_rng(1624).integers(0, 256, n, dtype=np.uint8).tobytes()
    blocks = cfec.easy_encode(data, k, m)
    B = len(blocks[0])
    lost = [17, 20, 23]
    pieces = [piece.Piece(chunk_idx=3, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks) if i not in lost]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=3, k=k, m=m, chunk_size=B, padlen=k * B - n,
                            original_chunk_size=n)
    eng = Engine(0, options={"SEC_CHECK_BS": 1})
    try:
        monkeypatch.setattr(piece, "get_engine", lambda *a, **kw: eng)
        assert eng.repair_methods() == (0, 0)
        got = piece.repair_chunks([ec], piece_ids=True)[0]
        assert eng.repair_methods() == (1, 0)
        fixed, checks = piece.repair_chunks_checked([ec], piece_ids=True)
        assert eng.repair_methods() == (2, 0)
        for ps in (got, fixed[0]):
            assert [p.piece_idx for p in ps] == lost
            for p in ps:
                assert p.data == blocks[p.piece_idx]
                assert p.piece_id == hashlib.sha1(blocks[p.piece_idx]).hexdigest()
        ck = checks[0]
        assert (ck.checked, ck.consistent, ck.bad_piece_idx) == (21, True, [])
        # one corrupt held parity piece: reported and located, the targets still the oracle's
        bad = bytearray(blocks[21])
        bad[4999] ^= 0x5A
        ec.pieces = [p if p.piece_idx != 21 else p.model_copy(update={"data": bytes(bad)}) for p in pieces]
        fixed, checks = piece.repair_chunks_checked([ec], [lost])
        ck = checks[0]
        assert (ck.consistent, ck.first_bad_offset, ck.bad_piece_idx, ck.located) == (False, 4999, [21], True)
        assert [p.data for p in fixed[0]][:3] == [blocks[t] for t in lost]
        assert eng.repair_methods()[0] >= 3
    finally:
        eng.close()
