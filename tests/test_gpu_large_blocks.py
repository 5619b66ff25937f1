"""GPU: zfec(64,96) with 3-4 MiB blocks (storb's 256 MiB chunks) on every path that serves it,
byte for byte against tests/gf_torch_ref.py (tied to the C oracle by tests/test_gf_torch_ref.py).

From B >= 3 MiB the pair encode and the two-kernel wide decode launch their tiles in XCD order
(bs_plan.hpp xcd_order), and only at these sizes are the position bits above 16 of a tile's t0, the
B - 16 clamp, the syndrome scratch offsets and the LDS solve exercised with large values.  The block
sizes: 3 MiB - 16 (chunk order still), 3 MiB (1536 spans, a multiple of 8), 3 MiB + 3 * 2048 + 37
(1540 spans, remainder 4, last span partial, not a multiple of 16) and 4 MiB (the policy's piece).

All data is seeded random bytes made on the device; every expected byte is gf_torch_ref's or the
source chunk itself, never another HIP path's.  Every chunk has padlen > 0 and block k-1 is read in
place with block_avail = B - padlen.  Sources sit in arenas of 0xFF and must be unchanged after
each call; outputs are 0xFF / 0xA5-filled with guard bytes and compared whole.  A difference is
reported as the first differing (row, position) and position // 2048, its span.

Flips and what a check must report follow the rule of tests/test_gpu_check_bs.py: a flip in a check
row flags that row; a flip in a data block flags every held check row; `first` is the flipped
position and `column` the entries' bytes there (0 past an entry's avail)."""

import random
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import zfec_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import piece  # noqa: E402
from storb_amd._lib import (CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, DCHK_DTYPE, DEC_DTYPE, ENC_DTYPE,  # noqa: E402
                            RCHK_DTYPE, REP_DTYPE)
from storb_amd.engine import check_locate  # noqa: E402
from tests import gf_torch_ref  # noqa: E402

MiB = 1 << 20
SPAN = 2048
DEEP = 1 << 21  # flips go past this position: bit 21 of a tile's t0 set
B_BELOW, B_FIRST, B_RAGGED, B_POLICY = 3 * MiB - 16, 3 * MiB, 3 * MiB + 3 * SPAN + 37, 4 * MiB
B_STAR = [B_BELOW, B_FIRST, B_RAGGED, B_POLICY]
B_SMALL = 70001  # a chunk in chunk order beside a large one
B_ODD = 3 * MiB + 5  # zfec(32,48) and (16,24): one row group, a 5-byte last span
PADLEN = {64: 29, 32: 13, 16: 7}
GUARD = 0xA5
UNTOUCHED = 0xEE
FORCED = dict(SEC_SYN=1, SEC_SYN_FUSED=0)  # the two syndrome kernels for every chunk with a lost block

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def test_sizes_are_what_the_names_say():
    spans = [-(-b // SPAN) for b in B_STAR]
    assert spans == [1536, 1536, 1540, 2048] and spans[2] % 8 == 4
    assert B_BELOW < 3 * MiB <= B_FIRST and B_RAGGED % 16 and B_RAGGED % SPAN == 37 and B_ODD % SPAN == 5
    assert all(0 < p < k for k, p in PADLEN.items())


def ref(k, m, B, seed=0):
    """A seeded chunk of k * B - padlen device bytes and the reference's m blocks [m, B]."""
    key = ("ref", k, m, B, seed)
    if key not in _cache:
        n = k * B - PADLEN[k]
        g = torch.Generator(device="cuda")
        g.manual_seed(1000003 * k + B + seed)
        chunk = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        blocks = gf_torch_ref.encode(chunk, k, m)
        assert tuple(blocks.shape) == (m, B) and torch.equal(blocks[:k].reshape(-1)[:n], chunk)
        assert not blocks[k - 1, B - PADLEN[k]:].any()
        _cache[key] = SimpleNamespace(k=k, m=m, B=B, n=n, padlen=PADLEN[k], chunk=chunk, blocks=blocks)
    return _cache[key]


def arena(k, m, B, seed=0):
    """The reference's m blocks in a buffer of 0xFF at odd and even starts, block k-1 cut at
    B - padlen (0xFF behind it): off / avail by block number, and an untouched copy."""
    key = ("arena", k, m, B, seed)
    if key not in _cache:
        r = ref(k, m, B, seed)
        off, avail, cur = [], [], 3
        for j in range(m):
            off.append(cur)
            avail.append(B - r.padlen if j == k - 1 else B)
            cur += B + 5 + 2 * (j % 7)
        buf = torch.full((cur + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        for j in range(m):
            buf[off[j]:off[j] + avail[j]] = r.blocks[j, :avail[j]]
        _cache[key] = SimpleNamespace(r=r, k=k, m=m, B=B, padlen=r.padlen, off=off, avail=avail, buf=buf,
                                      pristine=buf.clone())
    return _cache[key]


def same(got, want, regions, what):
    """got == want whole (guards included); else the first difference as (row, position, span).
    regions: (name, start of row 0, row stride, rows, row length) of what `want` holds."""
    if torch.equal(got, want):
        return
    diff = torch.nonzero(got != want).view(-1)
    at = int(diff[0])
    where = f"byte {at} (outside every row: a guard byte)"
    for name, start, stride, nrows, length in regions:
        if start <= at < start + (nrows - 1) * stride + length:
            row, pos = divmod(at - start, stride) if nrows > 1 else (0, at - start)
            if pos < length:
                where = f"{name}: (row {row}, position {pos}), span {pos // SPAN}"
            else:
                where = f"{name}: guard after row {row}"
            break
    raise AssertionError(f"{what}: {diff.numel()} bytes differ, the first at {where}: "
                         f"got {int(got[at]):#04x}, want {int(want[at]):#04x}")


def unchanged(A, what):
    same(A.buf, A.pristine, [("source block", o, 0, 1, a) for o, a in zip(A.off, A.avail)], f"{what}: the source was written")


# ---- a. encode -----------------------------------------------------------------------------------

def run_encode(engine, chunks, what):
    """One encode_batch over `chunks` (ref()s): sources at odd starts in 0xFF, parity rows at a
    stride of B + 37 in 0xFF."""
    ed = np.zeros(len(chunks), dtype=ENC_DTYPE)
    cur, pcur, regions = 5, 11, []
    for i, r in enumerate(chunks):
        stride = r.B + 37
        ed[i] = (cur, r.n, pcur, stride, r.k, r.m)
        regions.append((f"chunk {i} zfec({r.k},{r.m}) B={r.B} parity", pcur, stride, r.m - r.k, r.B))
        cur += r.n + 9 + 2 * i
        pcur += (r.m - r.k) * stride + 6 + i
    src = torch.full((cur + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    want = torch.full((pcur + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, r in enumerate(chunks):
        src[int(ed[i]["in_off"]):int(ed[i]["in_off"]) + r.n] = r.chunk
        _, start, stride, nrows, length = regions[i]
        want[start:start + nrows * stride].view(nrows, stride)[:, :length] = r.blocks[r.k:]
    src0 = src.clone()
    par = torch.full_like(want, 0xFF)
    engine.encode_batch(ed, src, par)
    same(par, want, regions, what)
    assert torch.equal(src, src0), f"{what}: the source was written"


@pytest.mark.parametrize("bs", [None, 0], ids=["default", "SEC_BS=0"])
@pytest.mark.parametrize("B", B_STAR)
def test_encode_one_chunk(engine, B, bs):
    with engine.options(**({} if bs is None else {"SEC_BS": bs})):
        run_encode(engine, [ref(64, 96, B)], f"encode B={B} {'default' if bs is None else 'SEC_BS=0'}")


@pytest.mark.parametrize("bs", [None, 0], ids=["default", "SEC_BS=0"])
def test_encode_mixed_batch(engine, bs):
    """A 4 MiB-block and a 70001-byte-block (64,96) chunk (two launch groups of the pair encode, one
    in XCD order) with a (32,48) and a (16,24) chunk of 3 MiB + 5 blocks in one call."""
    chunks = [ref(64, 96, B_POLICY), ref(64, 96, B_SMALL), ref(32, 48, B_ODD), ref(16, 24, B_ODD)]
    with engine.options(**({} if bs is None else {"SEC_BS": bs})):
        run_encode(engine, chunks, f"mixed encode {'default' if bs is None else 'SEC_BS=0'}")


# ---- b. decode -----------------------------------------------------------------------------------

def pattern(name, k=64, m=96, seed=0):
    """The k block numbers a decoder holds, shuffled.  Block k-1 is held in '32', '16 both' and
    '16 one' (read in place, short by padlen) and lost in '24' and '3'."""
    rng = random.Random(f"{name} {seed}")
    g0, g1 = list(range(k, k + 16)), list(range(k + 16, m))
    if name == "32":  # every parity row held
        lost, par = rng.sample(range(k - 1), 32), g0 + g1
    elif name == "24":
        lost = rng.sample(range(k - 1), 23) + [k - 1]
        par = rng.sample(g0, 11) + rng.sample(g1, 13)
    elif name == "16 both":
        lost, par = rng.sample(range(k - 1), 16), rng.sample(g0, 7) + rng.sample(g1, 9)
    elif name == "16 one":  # parity rows of one group: the fused one-wave kernel
        lost, par = rng.sample(range(k - 1), 16), g1
    else:
        assert name == "3"
        lost, par = [5, 40, k - 1], [g0[3], g1[0], g1[15]]
    keep = [j for j in range(k) if j not in lost] + par
    assert len(keep) == k == len(set(keep))
    rng.shuffle(keep)
    return keep


PATTERNS = ["32", "24", "16 both", "16 one", "3"]


def run_decode(engine, items, recover, what):
    """One decode_batch over items [(arena, keep)].  -> (decode_paths, decode_methods) deltas."""
    d = np.zeros(len(items), dtype=DEC_DTYPE)
    sn, offs, av, regions, parts = [], [], [], [], []
    ocur = 7
    for i, (A, keep) in enumerate(items):
        k, B = A.k, A.B
        lost = [j for j in range(k) if j not in keep]
        d[i] = (ocur, B, A.padlen, len(sn), k, A.m)
        if recover:  # the lost data blocks, B bytes each, in block order
            exp = A.r.blocks[torch.tensor(lost, device="cuda")].reshape(-1)
            regions.append((f"chunk {i} B={B} lost block (row = index in {lost})", ocur, B, len(lost), B))
        else:
            exp = A.r.chunk
            regions += [(f"chunk {i} B={B} data block", ocur, B, k - 1, B),
                        (f"chunk {i} B={B} data block {k - 1}", ocur + (k - 1) * B, 0, 1, B - A.padlen)]
        parts.append((ocur, exp))
        ocur += exp.numel() + 9 + (i % 2)
        for s in keep:
            sn.append(s)
            offs.append(A.buf.data_ptr() + A.off[s])
            av.append(A.avail[s])
    want = torch.full((ocur + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    for o, exp in parts:
        want[o:o + exp.numel()] = exp
    out = torch.full_like(want, 0xFF)
    p0, m0 = engine.decode_paths(), engine.decode_methods()
    engine.decode_batch(d, np.array(sn, np.int32), np.array(offs, np.uint64), 0, out,
                        block_avail=np.array(av, np.uint64), recover_only=recover)
    p1, m1 = engine.decode_paths(), engine.decode_methods()
    same(out, want, regions, what)
    for A, _ in items:
        unchanged(A, what)
    return tuple(b - a for a, b in zip(p0, p1)), tuple(b - a for a, b in zip(m0, m1))


METHODS = ("fused one-wave", "two-wave", "two kernels", "direct")


@pytest.mark.parametrize("forced", [False, True], ids=["default", "forced"])
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("B", [B_RAGGED, B_POLICY])
def test_decode(engine, B, name, forced):
    """Reassemble and recover-only of one (64,96) chunk from reference-made blocks."""
    A = arena(64, 96, B)
    keep = pattern(name)
    if name in ("24", "16 both"):
        assert {(s - 64) // 16 for s in keep if s >= 64} == {0, 1}
    with engine.options(**(FORCED if forced else {})):
        for recover in (False, True):
            what = f"decode B={B} {name} lost, {'recover-only' if recover else 'reassemble'}, " \
                   f"{'forced' if forced else 'default'}"
            paths, methods = run_decode(engine, [(A, keep)], recover, what)
            assert sum(paths) == 1 and sum(methods) == 1, (what, paths, methods)
            if forced:  # every chunk with a lost block is eligible: the two kernels
                assert paths == (1, 0) and methods == (0, 0, 1, 0), (what, paths, methods)
            else:
                print(f"PATH {what}: {METHODS[methods.index(1)]}")


@pytest.mark.parametrize("forced", [False, True], ids=["default", "forced"])
@pytest.mark.parametrize("recover", [False, True], ids=["reassemble", "recover"])
def test_decode_mixed_sizes(engine, recover, forced):
    """A 4 MiB-block and a 70001-byte-block chunk with 24 lost each in one call: they share the
    phase-1 and the phase-2 launch, whose whole tile lists go in XCD order because one chunk is
    large.  Both exact."""
    items = [(arena(64, 96, B_POLICY), pattern("24")), (arena(64, 96, B_SMALL), pattern("24", seed=1))]
    what = f"mixed decode, {'recover-only' if recover else 'reassemble'}, {'forced' if forced else 'default'}"
    with engine.options(**(FORCED if forced else {})):
        paths, methods = run_decode(engine, items, recover, what)
        run_decode(engine, items[::-1], recover, what + ", small chunk first")
    assert sum(paths) == 2
    if forced:
        assert paths == (2, 0) and methods == (0, 0, 2, 0), (paths, methods)
    else:
        print(f"PATH {what}: " + ", ".join(f"{n} x {METHODS[i]}" for i, n in enumerate(methods) if n))


# ---- c. check, decode + check, repair, repair + check -------------------------------------------------

def entries_of(k, m, B):
    """Every data block, shuffled, then every parity row, shuffled."""
    rng = random.Random(k * 100003 + m * 101 + B)
    return rng.sample(range(k), k) + rng.sample(range(k, m), m - k)


def flip_positions(B):
    last = B // SPAN * SPAN + (B % SPAN) // 2  # inside the last partial span, not its last byte
    assert B // SPAN * SPAN <= last < B - 1 and B % SPAN
    return [0, B - 1, DEEP + 2047, DEEP + 2048, last]


class Flipped:
    """One byte of an entry XORed with 0x5A in the arena for the duration of a call."""

    def __init__(self, A, block, pos):
        assert pos < A.avail[block], "a flip must land on a byte that is in memory"
        self.A, self.at = A, A.off[block] + pos

    def __enter__(self):
        self.A.buf[self.at] ^= 0x5A

    def __exit__(self, *exc):
        self.A.buf[self.at] ^= 0x5A


def check_call(engine, A, entries, decode, opt, flip, what):
    """A check or decode + check of one chunk; flip: (entry position, byte position) or None."""
    k, m, B, n = A.k, A.m, A.B, len(entries)
    sn = np.array(entries, np.int32)
    offs = np.array([A.buf.data_ptr() + A.off[s] for s in entries], np.uint64)
    av = np.array([A.avail[s] for s in entries], np.uint64)
    res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    rb = torch.full((n,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    col = torch.full((n,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    nout = k * B - A.padlen
    out = torch.full((7 + nout + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    want_out = out.clone()
    b0 = engine.check_methods()
    if decode:
        dchk = np.zeros(1, dtype=DCHK_DTYPE)
        dchk[0] = (7, B, A.padlen, 0, n, k, m, 0)
        engine.decode_check_batch(dchk, sn, offs, 0, out, res, block_avail=av, row_bad=rb, column=col)
        # nothing lost: the data blocks as held (a flipped data byte included), in block order
        want_out[7:7 + nout] = A.r.chunk
        if flip is not None and entries[flip[0]] < k:
            want_out[7 + entries[flip[0]] * B + flip[1]] ^= 0x5A
    else:
        chk = np.zeros(1, dtype=CHK_DTYPE)
        chk[0] = (B, 0, n, k, m, 0)
        engine.check_batch(chk, sn, offs, 0, res, block_avail=av, row_bad=rb, column=col)
    b1 = engine.check_methods()
    assert (b1[0] - b0[0], b1[1] - b0[1]) == ((1, 0) if opt else (0, 1)), f"{what}: kernel taken"
    same(out, want_out, [("data block", 7, B, k - 1, B), (f"data block {k - 1}", 7 + (k - 1) * B, 0, 1, B - A.padlen)], what)
    verify_check(A, entries, flip, res, rb, col, what)


def verify_check(A, entries, flip, res, rb, col, what):
    k, n = A.k, len(entries)
    res = np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)[0]
    rb, col = rb.cpu().numpy(), col.cpu().numpy()
    if flip is None or n == k:
        assert int(res["first"]) == CHK_CONSISTENT and int(res["nbad"]) == 0, f"{what}: clean"
        assert not rb.any(), f"{what}: a flag on a clean chunk"
        assert (col == UNTOUCHED).all(), f"{what}: column of a consistent chunk was written"
        return
    e, first = flip
    rows = set(range(k, n)) if e < k else {e}
    held = A.buf[torch.tensor([A.off[s] + min(first, A.avail[s] - 1) for s in entries], device="cuda")].cpu().numpy()
    column = bytes(int(held[j]) if first < A.avail[s] else 0 for j, s in enumerate(entries))
    assert int(res["first"]) == first, f"{what}: first {int(res['first'])} != {first} (span {int(res['first']) // SPAN})"
    assert int(res["nbad"]) == len(rows), f"{what}: nbad {int(res['nbad'])} != {len(rows)}"
    assert {j for j in range(n) if rb[j]} == rows and set(rb.tolist()) <= {0, 1}, f"{what}: row_bad"
    assert col.tobytes() == column, f"{what}: column"
    assert check_locate(k, A.m, entries, column) == e, f"{what}: located"


def flip_cases(A, entries):
    """None (clean), then one flip in a parity piece and one in a data piece (not block k-1) at each
    position, and one in block k-1's last byte in memory."""
    k, n, B = A.k, len(entries), A.B
    cases = [None]
    data = [j for j in range(k) if entries[j] != k - 1]
    for i, p in enumerate(flip_positions(B)):
        cases.append((k + (5 * i + 3) % (n - k), p))
        cases.append((data[(11 * i + 2) % len(data)], p))
    cases.append((entries.index(k - 1), B - A.padlen - 1))
    return cases


CHECK_SHAPES = [(64, 96, B_RAGGED), (32, 48, B_ODD)]


@pytest.mark.parametrize("opt", [1, 0], ids=["SEC_CHECK_BS=1", "SEC_CHECK_BS=0"])
@pytest.mark.parametrize("k,m,B", CHECK_SHAPES)
def test_check_and_decode_check(engine, k, m, B, opt):
    A = arena(k, m, B)
    entries = entries_of(k, m, B)
    with engine.options(SEC_CHECK_BS=opt):
        for flip in flip_cases(A, entries):
            for decode in (False, True):
                what = f"zfec({k},{m}) B={B} SEC_CHECK_BS={opt} {'decode + check' if decode else 'check'}, flip {flip}"
                if flip is None:
                    check_call(engine, A, entries, decode, opt, None, what)
                else:
                    with Flipped(A, entries[flip[0]], flip[1]):
                        check_call(engine, A, entries, decode, opt, flip, what)
                unchanged(A, what)


def repair_call(engine, A, basis, held, targets, checks, opt, flip, what):
    """A repair from the data blocks `basis` (checks: a repair + check with the rows `held` too)."""
    k, m, B = A.k, A.m, A.B
    entries = basis + (held if checks else [])
    n = len(entries)
    sn = np.array(entries, np.int32)
    offs = np.array([A.buf.data_ptr() + A.off[s] for s in entries], np.uint64)
    av = np.array([A.avail[s] for s in entries], np.uint64)
    to, tcur = [], 0
    for j in range(len(targets)):  # each target at 1 or 33 modulo 64 between runs of GUARD
        start = tcur + 64
        start += (1 + 32 * (j % 2) - start) % 64
        to.append(start)
        tcur = start + B
    want = torch.full((tcur + 64,), GUARD, dtype=torch.uint8, device="cuda")
    for o, t in zip(to, targets):
        want[o:o + B] = A.r.blocks[t]
        if flip is not None and entries[flip[0]] < k:  # the encode of the data as held: the code is linear
            want[o + flip[1]] ^= int(zfec_ref.MUL[zfec_ref.parity_rows(k, m)[t - k, entries[flip[0]]]][0x5A])
    tgt = torch.full_like(want, GUARD)
    tn, to = np.array(targets, np.int32), np.array(to, np.uint64)
    res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    rb = torch.full((n,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    col = torch.full((n,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    b0 = engine.repair_methods()
    if checks:
        d = np.zeros(1, dtype=RCHK_DTYPE)
        d[0] = (B, 0, 0, len(targets), n, k, m)
        engine.repair_check_batch(d, sn, offs, 0, tn, to, tgt, res, block_avail=av, row_bad=rb, column=col)
    else:
        d = np.zeros(1, dtype=REP_DTYPE)
        d[0] = (B, 0, 0, len(targets), k, m, 0)
        engine.repair_batch(d, sn, offs, 0, tn, to, tgt, block_avail=av)
    b1 = engine.repair_methods()
    assert (b1[0] - b0[0], b1[1] - b0[1]) == ((1, 0) if opt else (0, 1)), f"{what}: kernel taken"
    same(tgt, want, [(f"target {t}", int(o), 0, 1, B) for o, t in zip(to, targets)], what)
    if checks:
        verify_check(A, entries, flip, res, rb, col, what)


def repair_sets(k, m):
    """(targets, rows held for the check): (64,96) targets in group 0, in group 1, in both and all
    32 rows; (32,48), one row group: a few rows and all 16."""
    rng = random.Random(m)
    par = list(range(k, m))
    if m - k <= 16:
        few = rng.sample(par, 5)
        return [(few, rng.sample([r for r in par if r not in few], 6)), (rng.sample(par, len(par)), [])]
    g0, g1 = par[:16], par[16:]
    t0, t1 = rng.sample(g0, 5), rng.sample(g1, 7)
    both = rng.sample(g0, 4) + rng.sample(g1, 5)
    rng.shuffle(both)
    rest = [r for r in par if r not in both]
    return [(t0, rng.sample(g1, 6)), (t1, rng.sample(g0, 3) + rng.sample([r for r in g1 if r not in t1], 3)),
            (both, rng.sample(rest, 8)), (rng.sample(par, len(par)), [])]


@pytest.mark.parametrize("opt", [1, 0], ids=["SEC_CHECK_BS=1", "SEC_CHECK_BS=0"])
@pytest.mark.parametrize("k,m,B", CHECK_SHAPES)
def test_repair_and_repair_check(engine, k, m, B, opt):
    """Targets byte for byte the reference's rows, from the shuffled data blocks.  The repair + check:
    clean; a flip in a held parity row at each position (that row flagged, the targets untouched);
    a flip in a data block (every held row flagged, the targets those of the data as held: each
    differs from the reference's row in that one byte, by the row's coefficient times 0x5A)."""
    A = arena(k, m, B)
    basis = entries_of(k, m, B)[:k]
    pos = flip_positions(B)
    not_last = [j for j in range(k) if basis[j] != k - 1]
    with engine.options(SEC_CHECK_BS=opt):
        for i, (targets, held) in enumerate(repair_sets(k, m)):
            what = f"zfec({k},{m}) B={B} SEC_CHECK_BS={opt} targets {sorted(targets)}"
            repair_call(engine, A, basis, held, targets, False, opt, None, what + ", repair")
            repair_call(engine, A, basis, held, targets, True, opt, None, what + ", repair + check")
            unchanged(A, what)
            for j, p in enumerate(pos if held else []):
                flip = (k + (i + 2 * j) % len(held), p)
                with Flipped(A, held[flip[0] - k], p):
                    repair_call(engine, A, basis, held, targets, True, opt, flip, what + f", repair + check, flip {flip}")
                unchanged(A, what)
            flip = (not_last[7 * i + 1], pos[3])
            with Flipped(A, basis[flip[0]], flip[1]):
                repair_call(engine, A, basis, held, targets, True, opt, flip, what + f", repair + check, flip {flip}")
            unchanged(A, what)


# ---- d. the piece API on one policy-sized chunk (host memory) ------------------------------------------

POLICY_B = 2021 * SPAN + 1037  # 2022 spans, the last one partial
POLICY_N = 64 * POLICY_B - 29


@pytest.fixture(scope="module")
def policy_chunk():
    """A chunk that storb's policy cuts into zfec(64,96) with 2022 spans per block (remainder 6) and
    padlen 29; the reference's blocks computed on the device from the uploaded chunk, as bytes."""
    k, m, B, padlen = piece.chunk_shape(POLICY_N)
    assert (k, m, B, padlen) == (64, 96, POLICY_B, 29) == zfec_ref.chunk_shape(POLICY_N)
    assert -(-B // SPAN) == 2022 and 2022 % 8 == 6 and B >= 3 * MiB and padlen > 0
    host = np.random.default_rng(2022).integers(0, 256, POLICY_N, dtype=np.uint8)
    blocks = gf_torch_ref.encode(torch.from_numpy(host).cuda(), k, m).cpu().numpy()
    yield SimpleNamespace(k=k, m=m, B=B, padlen=padlen, n=POLICY_N, data=host.tobytes(),
                          blocks=[blocks[j].tobytes() for j in range(m)])


def _first_diff(got: bytes, want: bytes):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return f"length {a.size} != {b.size}"
    d = np.flatnonzero(a != b)
    return f"{d.size} bytes differ, the first at position {int(d[0])}, span {int(d[0]) // SPAN}"


def _encoded(c, held):
    pieces = [piece.Piece(chunk_idx=0, piece_idx=i, data=c.blocks[i],
                          piece_type=piece.PieceType.Data if i < c.k else piece.PieceType.Parity) for i in held]
    return piece.EncodedChunk(pieces=pieces, chunk_idx=0, k=c.k, m=c.m, chunk_size=c.B, padlen=c.padlen,
                              original_chunk_size=c.n)


def test_piece_encode_chunk(policy_chunk):
    c = policy_chunk
    ec = piece.encode_chunk(c.data, 0)
    assert (ec.k, ec.m, ec.chunk_size, ec.padlen, len(ec.pieces)) == (c.k, c.m, c.B, c.padlen, c.m)
    for i, p in enumerate(ec.pieces):
        assert p.piece_idx == i and len(p.data) == c.B
        assert p.data == c.blocks[i], f"piece {i} (row {i - c.k}): {_first_diff(p.data, c.blocks[i])}"


def test_piece_reconstruct_data(policy_chunk):
    """From 64 of the 96 pieces: 24 data pieces dropped, 24 parity pieces of both groups in their place."""
    c = policy_chunk
    rng = random.Random(64)
    lost = rng.sample(range(c.k), 24)
    held = [j for j in range(c.k) if j not in lost] + rng.sample(range(64, 80), 10) + rng.sample(range(80, 96), 14)
    ec = _encoded(c, held)
    pieces = list(ec.pieces)
    rng.shuffle(pieces)
    ec.pieces = []
    got = piece.reconstruct_data(pieces, [ec])
    assert got == c.data, _first_diff(got, c.data)


def test_piece_decode_chunks_checked(policy_chunk):
    """Every piece held, one byte of parity piece 81 flipped past 2^21: named, and the chunk returned."""
    c = policy_chunk
    ec = _encoded(c, range(c.m))
    at = DEEP + SPAN + 5
    bad = bytearray(c.blocks[81])
    bad[at] ^= 0x5A
    ec.pieces[81] = ec.pieces[81].model_copy(update={"data": bytes(bad)})
    got, checks = piece.decode_chunks_checked([ec])
    ck = checks[0]
    assert (ck.checked, ck.consistent, ck.first_bad_offset, ck.bad_piece_idx, ck.located) == (96, False, at, [81], True)
    assert got == c.data, _first_diff(got, c.data)
