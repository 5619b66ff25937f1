"""GPU: sec_repair_correct_batch against expectations that never come from the code under test.
Blocks = cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c); damage is bytes XORed into the buffer
image in numpy at places the test chose.  So a target's expected bytes are the ORACLE'S block
wherever a position carries at most one damaged entry (and the chunk has two check rows or more),
whether the target was lost or is a held entry being healed; the expected hits are the flips the
test put into each entry; and the expected open positions are those where it put two (in shapes
with n - k >= 3) or any (n - k == 1).  There, and everywhere in a chunk with n == k, every target is
cfec.easy_encode(cfec.easy_decode(basis as held))[target] at that position.  A second witness:
engine.check_locate (host arithmetic) on the damaged columns must name the entry the call counted.

Layout of every case as in tests/test_gpu_repair_check.py and tests/test_gpu_decode_correct.py:
each entry sits in a buffer of 0xFF at odd and even starts, so a short entry (block_avail < B) is
followed by 0xFF bytes and a read past its avail shows up as a difference; the buffer must be
byte-identical after every call.  The target buffer is 0xFF-filled too, every target at an odd or
even start with guard bytes around it, and is compared whole.  Every case also asks for the targets'
digests, which must equal hashlib's of the expected bytes."""

import functools
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import CHK_CONSISTENT, COR_RESULT_DTYPE, RCHK_DTYPE  # noqa: E402
from storb_amd.engine import Engine, Error, check_locate, get_engine, pinned_bytes  # noqa: E402

UNTOUCHED = 0xEEEEEEEE  # entry_hits before the call
WITNESSED = 48  # damaged columns per chunk put before check_locate


@functools.lru_cache(maxsize=None)
def _chunk(k, m, B, padlen, seed):
    """The oracle's m blocks (block k-1 with its zero padding) of a seeded chunk of k*B - padlen bytes."""
    data = np.random.default_rng(seed).integers(0, 256, k * B - padlen, dtype=np.uint8).tobytes()
    blocks = cfec.easy_encode(data + b"\0" * padlen, k, m)
    assert len(blocks) == m and all(len(b) == B for b in blocks)
    return blocks


def spec(k, m, B, entries, targets, flips=(), padlen=0, short=False, seed=None):
    """One chunk: blocks `entries` held, the first k the basis, the rest the check rows; blocks
    `targets` asked for, held or not.  flips: (entry position, byte position[, xor value, default
    0x5A]).  short: block k-1, wherever it is among the entries, is handed over with block_avail =
    B - padlen."""
    assert len(set(entries)) == len(entries) >= k and len(set(targets)) == len(targets)
    flips = [(f[0], f[1], f[2] if len(f) > 2 else 0x5A) for f in flips]
    assert len({(e, p) for e, p, _ in flips}) == len(flips) and all(v for _, _, v in flips)
    return dict(k=k, m=m, B=B, entries=list(entries), targets=list(targets), flips=flips, padlen=padlen, short=short,
                seed=seed if seed is not None else 1000 * k + m + B)


def flipped(s, *flips):
    return spec(s["k"], s["m"], s["B"], s["entries"], s["targets"], flips, s["padlen"], s["short"], s["seed"])


def _held(s):
    k, B = s["k"], s["B"]
    blocks = _chunk(k, s["m"], B, s["padlen"], s["seed"])
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
    """(target blocks, first, first_open, corrected, open, hits per entry, {position: entry or -2})."""
    k, m, B, n = s["k"], s["m"], s["B"], len(s["entries"])
    blocks = _chunk(k, m, B, s["padlen"], s["seed"])
    nr = n - k
    at = {}
    for e, p, _ in s["flips"]:
        at.setdefault(p, []).append(e)
    basis = [bytes(h) + b"\0" * (B - len(h)) for h in held[:k]]
    as_held = cfec.easy_encode(cfec.easy_decode(basis, s["entries"][:k], 0, k, m), k, m)
    if nr == 0:  # nothing to check: a plain repair, consistent whatever the bytes
        return [as_held[t] for t in s["targets"]], None, None, 0, 0, [0] * n, {}
    exp = [bytearray(blocks[t]) for t in s["targets"]]
    hits, verdict, opened = [0] * n, {}, []
    for p, es in sorted(at.items()):
        if nr >= 2 and len(es) == 1:
            hits[es[0]] += 1
            verdict[p] = es[0]
            continue
        assert nr == 1 or nr >= 3, "two flips at one position of a distance-3 code prove nothing"
        opened.append(p)
        verdict[p] = -2
        for x, t in zip(exp, s["targets"]):
            x[p] = as_held[t][p]
    return ([bytes(x) for x in exp], min(at) if at else None, min(opened) if opened else None, sum(hits), len(opened),
            hits, verdict)


def _layout(specs):
    descs = np.zeros(len(specs), dtype=RCHK_DTYPE)
    sn, bo, av, tn, to, want, parts, outs = [], [], [], [], [], [], [], []
    cur, ocur = 3, 7
    for i, s in enumerate(specs):
        k, B, n = s["k"], s["B"], len(s["entries"])
        held, avail = _held(s)
        descs[i] = (B, len(sn), len(tn), len(s["targets"]), n, k, s["m"])
        w = _expect(s, held)
        columns = {p: bytes(held[j][p] if p < avail[j] else 0 for j in range(n)) for p in w[6]}
        want.append(w[1:] + (columns,))
        for j, t in enumerate(s["targets"]):
            tn.append(t)
            to.append(ocur)
            outs.append((ocur, w[0][j]))
            ocur += B + 9 + (j % 2)  # guard bytes between the targets, odd and even starts
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
    dig = np.frombuffer(b"".join(hashlib.sha1(b).digest() for _, b in outs), np.uint8)
    return SimpleNamespace(descs=descs, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), tn=np.array(tn + [0], np.int32)[:len(tn)],
                           to=np.array(to + [0], np.uint64)[:len(to)], src=src, out=out, dig=dig, want=want, specs=specs)


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
    return f"targets differ at {d[:8].tolist()} ({d.size} bytes)" if d.size else ""


def run_device(engine, L, dsrc=None, asynchronous=False, use_avail=True, with_hits=True, with_digests=True):
    if dsrc is None:
        dsrc = torch.from_numpy(L.src).cuda()
    dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
    res = torch.zeros(24 * len(L.specs), dtype=torch.uint8, device="cuda")
    hits = torch.from_numpy(np.full(len(L.sn), UNTOUCHED, np.uint32).view(np.int32)).cuda() if with_hits else None
    dig = torch.zeros(max(L.dig.size, 1), dtype=torch.uint8, device="cuda") if with_digests else None
    engine.repair_correct_batch(L.descs, L.sn, L.bo + np.uint64(dsrc.data_ptr()), 0, L.tn, L.to, dout, res,
                                block_avail=L.av if use_avail else None, digests=dig, entry_hits=hits,
                                asynchronous=asynchronous)
    if asynchronous:
        engine.sync()
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    assert not _out_diff(dout.cpu().numpy(), L.out)
    if with_digests:
        assert dig.cpu().numpy()[:L.dig.size].tobytes() == L.dig.tobytes()
    _verify(L, res.cpu().numpy(), hits.cpu().numpy().view(np.uint32) if with_hits else None)
    return dsrc


def run_host(eng, L):
    src = L.src.copy()
    out = np.full(L.out.size, 0xFF, np.uint8)
    res = np.zeros(len(L.specs), dtype=COR_RESULT_DTYPE)
    hits = np.full(len(L.sn), UNTOUCHED, np.uint32)
    dig = np.zeros(max(L.dig.size, 1), np.uint8)
    eng.repair_correct_batch(L.descs, L.sn, L.bo, src, L.tn, L.to, out, res, block_avail=L.av, digests=dig,
                             entry_hits=hits, host=True)
    assert np.array_equal(src, L.src), "the source buffer was written"
    assert not _out_diff(out, L.out)
    assert dig[:L.dig.size].tobytes() == L.dig.tobytes()
    _verify(L, res, hits)


def run_both(engine, specs, **kw):
    L = _layout(specs)
    run_device(engine, L, **kw)
    run_host(engine, L)


# zfec(4,7) from blocks {5, 0, 3, 2}: block 6 is lost, primary 1 is a check row, the basis holds parity 5
E47 = [5, 0, 3, 2, 4, 1]
T47 = [6, 1, 5, 0]  # a lost block, a check-row heal, a basis-parity heal, a basis-primary heal


def _edges(B):
    """Position 0, B - 1, and both sides of every boundary the kernel has: its 16-position lanes,
    its 4096-position tiles, and the last whole lane's end (where the byte-wise lane takes over)."""
    whole = B // 16 * 16
    return sorted({p for p in (0, B - 1, 15, 16, 31, 32, 4095, 4096, whole - 1, whole) if 0 <= p < B})


@pytest.mark.parametrize("B", [1, 5, 15, 16, 17, 63, 257, 4099])
def test_block_sizes(engine, B):
    """The tail kernel only (B < 16), exactly one lane, a straddling lane, several lanes, a second
    tile.  Clean; flips in a check row only; in a present-primary basis entry; in the basis entry
    that is a parity block; in two different entries at different positions."""
    s = spec(4, 7, B, E47, T47)
    ps = _edges(B)
    two = [(q % 2 * 5, p, 1 + (p % 255)) for q, p in enumerate(ps)]  # entries 0 and 5 in turn
    run_both(engine, [s, flipped(s, *[(4, p) for p in ps]), flipped(s, *[(2, p, 0xFF) for p in ps]),
                      flipped(s, *[(0, p, 0x01) for p in ps]), flipped(s, *two)], use_avail=False)


# 12 of zfec(10,14) held (blocks 1 and 7 lost), nr = 2; block 9 is short and a heal target
Z1014_SHORT = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 9, 8, 4, 12, 10], [9, 1, 7], padlen=4, short=True)
Z1014_LOST9 = spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 1, 8, 4, 12, 10], [7, 9], padlen=4, short=True)
Z1014_ALL = spec(10, 14, 6554, [3, 0, 9, 1, 7, 5, 6, 2, 8, 4, 12, 10, 13, 11], [3, 12, 9, 13], padlen=4,
                 short=True)  # nr = 4


def test_short_block(engine):
    """zfec(10,14), B = 6554, padlen 4.  Block 9 held with avail = B - 4 (0xFF behind it) and also a
    heal target: it comes back whole, with its zero padding.  Then block 9 lost and a target.  A
    flip at avail - 1 of the short entry, and flips of full entries in the ragged end behind it."""
    short_at = Z1014_SHORT["entries"].index(9)
    run_both(engine, [Z1014_SHORT, flipped(Z1014_SHORT, (short_at, 6549)),
                      flipped(Z1014_SHORT, (1, 6553), (11, 6551), (short_at, 0), (0, 6550, 0x80)),
                      Z1014_LOST9, flipped(Z1014_LOST9, (7, 6553), (10, 6549), (0, 6552, 0x80))])
    blocks = _chunk(10, 14, 6554, 4, Z1014_SHORT["seed"])
    assert blocks[9][-4:] == b"\0" * 4 and any(blocks[9][-8:-4])  # what "whole" means above


_P16 = [s for s in range(16) if s not in (0, 5)]
# 18 of zfec(16,24) held, data pieces 0 and 5 among the six lost; ten targets: two groups of rows
Z1624 = spec(16, 24, 259, _P16[::-1] + [19, 16] + [23, 20], [0, 5, 17, 18, 21, 22, 19, 3, 23, 16])


def test_more_than_eight_targets(engine):
    """zfec(16,24), B = 259: the six lost blocks and four held ones.  Flips in a basis parity row, in
    a present primary and in a check row."""
    run_both(engine, [Z1624, flipped(Z1624, (14, 7), (14, 258), (Z1624["entries"].index(3), 100),
                                     (Z1624["entries"].index(3), 255), (15, 256, 0x11), (16, 8), (17, 31, 0x80))])


_B32 = [40, 33] + [s for s in range(32) if s not in (0, 13)][::-1]
# every block of zfec(32,48) held (nr = 16), and the same with blocks 47 and 35 lost (nr = 14)
Z3248 = spec(32, 48, 130, _B32 + [0, 13] + [s for s in range(32, 48) if s not in (40, 33)], [44, 40, 1, 13, 0])
Z3248_LOST = spec(32, 48, 130, _B32 + [0, 13] + [s for s in range(32, 47) if s not in (40, 33, 35)],
                  [47, 35, 40, 1, 13, 44])
_B64 = list(range(1, 64)) + [64]
Z6496 = spec(64, 96, 33, _B64 + list(range(65, 81)), [0, 81, 95, 63, 64, 80, 6, 41])  # 80 held, nr = 16


def test_row_groups(engine):
    """More than one group of check rows, over k = 32 and over k = 64: flips in a check row of the
    second group, in basis entries, in the ragged end.  Targets are lost blocks and the damaged
    entries.  (All 48 of zfec(32,48) held is nr = 16; with two lost it is nr = 14: both run.)"""
    e44 = Z3248["entries"].index(44)
    assert e44 - 32 >= 8 and Z3248_LOST["entries"].index(44) - 32 >= 8  # a check row of the second group
    f32 = [(0, 64), (31, 129), (Z3248["entries"].index(13), 128, 0xC3)]
    run_both(engine, [Z3248, flipped(Z3248, (e44, 5), *f32),
                      Z3248_LOST, flipped(Z3248_LOST, (Z3248_LOST["entries"].index(44), 5), *f32),
                      Z6496, flipped(Z6496, (63, 0), (64 + 15, 31), (5, 32, 0x02), (40, 16))])


def test_two_errors_at_one_position_are_open(engine):
    """zfec(10,14) with all 14 held (distance 5): two flips at one position are reported open and
    every target there is what the basis as held predicts; another position with one flip is
    corrected.  The same in the ragged end."""
    s = flipped(Z1014_ALL, (2, 3000), (12, 3000, 0x21), (7, 41))
    L = _layout([s])
    assert L.want[0][:4] == (41, 3000, 1, 1)
    blocks = _chunk(10, 14, 6554, 4, s["seed"])
    t13 = int(L.to[3])
    assert L.out[t13 + 3000] != blocks[13][3000]  # the as-held prediction is not the oracle's byte there
    run_device(engine, L)
    run_host(engine, L)
    run_both(engine, [flipped(Z1014_ALL, (0, 6553), (1, 6553, 0x03), (13, 6552))])


def test_one_check_row_corrects_nothing(engine):
    """n - k = 1 (zfec(4,7) with five held): every damaged position is open and corrected == 0."""
    s = spec(4, 7, 257, [5, 0, 3, 2, 1], [6, 1, 0, 4])
    L = _layout([s, flipped(s, (4, 0), (1, 100), (0, 256))])
    assert L.want[1][:4] == (0, 0, 0, 3)
    run_device(engine, L)
    run_host(engine, L)


def test_plain_repair(engine):
    """n == k: reported consistent, a plain repair from the blocks as held; a heal target of a basis
    entry is a copy, damage included."""
    run_both(engine, [spec(4, 7, 4099, [5, 0, 3, 2], [1, 5, 6, 2]),
                      spec(4, 7, 17, [0, 1, 2, 3], [1, 4], flips=[(1, 3)]),
                      spec(4, 7, 4101, [0, 1, 2, 3], [3, 6], padlen=7, short=True)])
    L = _layout([spec(4, 7, 17, [0, 1, 2, 3], [1], flips=[(1, 3)])])
    assert L.out[int(L.to[0]) + 3] == _chunk(4, 7, 17, 0, 4024)[1][3] ^ 0x5A


def test_no_targets_counts_only(engine):
    """ntargets == 0: counts and hits, no block written; `out` may be NULL."""
    s = spec(4, 7, 257, E47, [])
    L = _layout([flipped(s, (4, 0), (1, 100), (0, 256)), s])
    assert L.want[0][:4] == (0, None, 3, 0) and L.tn.size == 0
    run_device(engine, L, with_digests=False)
    dsrc = torch.from_numpy(L.src).cuda()
    res = torch.zeros(24 * 2, dtype=torch.uint8, device="cuda")
    hits = torch.from_numpy(np.full(len(L.sn), UNTOUCHED, np.uint32).view(np.int32)).cuda()
    engine.repair_correct_batch(L.descs, L.sn, L.bo + np.uint64(dsrc.data_ptr()), 0, L.tn, L.to, None, res,
                                entry_hits=hits)
    _verify(L, res.cpu().numpy(), hits.cpu().numpy().view(np.uint32))
    res = np.zeros(2, dtype=COR_RESULT_DTYPE)
    hits = np.full(len(L.sn), UNTOUCHED, np.uint32)
    engine.repair_correct_batch(L.descs, L.sn, L.bo, L.src.copy(), L.tn, L.to, None, res, entry_hits=hits, host=True)
    _verify(L, res, hits)


def _junk(s, entry, seed):
    """`s` with one whole entry replaced by random bytes."""
    blocks = _chunk(s["k"], s["m"], s["B"], s["padlen"], s["seed"])
    true = np.frombuffer(blocks[s["entries"][entry]], np.uint8)
    junk = np.random.default_rng(seed).integers(0, 256, true.size, dtype=np.uint8)
    diff = true ^ junk
    return flipped(s, *[(entry, int(p), int(diff[p])) for p in np.flatnonzero(diff)]), int(np.count_nonzero(diff))


@pytest.mark.parametrize("entry", [2, 5])
def test_whole_piece_junk_is_healed(engine, entry):
    """One whole piece replaced by random bytes, zfec(4,7) B = 4099, and asked for as a target: the
    target is the oracle's block, corrected equals the positions where the random byte differs from
    the true one, and the hits fall on that entry only."""
    s, ndiff = _junk(spec(4, 7, 4099, E47, [E47[entry], 6]), entry, 77 + entry)
    L = _layout([s])
    assert 4000 < ndiff <= 4099 and L.want[0][2] == ndiff and L.want[0][4][entry] == ndiff
    assert sum(L.want[0][4]) == ndiff
    blocks = _chunk(4, 7, 4099, 0, s["seed"])
    assert L.out[int(L.to[0]):int(L.to[0]) + 4099].tobytes() == blocks[E47[entry]]
    run_device(engine, L)
    run_host(engine, L)


def _mixed():
    s47 = spec(4, 7, 4099, E47, T47)
    s5 = spec(4, 7, 5, E47, T47)
    return [Z1014_SHORT, flipped(s47, (4, 4095), (0, 4096), (3, 4098)), s47,
            flipped(Z1624, (14, 7), (Z1624["entries"].index(3), 255)), s5, flipped(s5, (1, 4)),
            flipped(Z3248, (Z3248["entries"].index(44), 5), (31, 129)), Z1624,
            flipped(Z1014_ALL, (2, 3000), (12, 3000, 0x21), (7, 41)),
            spec(4, 7, 17, [0, 1, 2, 3], [1, 4], flips=[(1, 3)]),
            flipped(spec(4, 7, 257, [5, 0, 3, 2, 1], [6, 1, 0, 4]), (1, 100)),
            flipped(spec(4, 7, 257, E47, []), (4, 0), (1, 100)),
            _junk(spec(4, 7, 63, E47, [1, 6]), 5, 5)[0], Z6496, flipped(Z6496, (63, 0), (64 + 15, 31)),
            flipped(Z1014_LOST9, (7, 6549)), Z3248_LOST]


def test_mixed_batch_twice_from_the_cached_plan(engine):
    """Every shape of this file in one call with clean chunks between, digests included; then the
    same plan on data changed in place (all clean): no count is left over from the first call; then
    SEC_F_ASYNC without hits."""
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
        assert eng.check_methods() == (0, 0) and eng.repair_methods() == (0, 0)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_timing_kind_is_the_correcting_calls(engine):
    engine.set_timing(True)
    try:
        for kind in ("decode_correct", "repair_check", "repair", "check"):
            engine.collect_timing(kind)
        run_device(engine, _layout([flipped(Z1624, (Z1624["entries"].index(3), 100))]))
        ms, launches = engine.collect_timing("decode_correct")
        assert launches == 1 and ms > 0
        for kind in ("repair_check", "repair", "check"):
            assert engine.collect_timing(kind) == (0.0, 0)
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    """Each error code in sec_repair_check_batch's order; no buffer is touched (the addresses handed
    over do not exist, and the results stay as they were)."""
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=RCHK_DTYPE)
    d[0] = (64, 0, 0, 2, 6, 4, 7)
    bo = np.zeros(8, np.uint64)  # never dereferenced: every call fails first
    to = np.zeros(4, np.uint64)
    res = np.full(24, 0x77, dtype=np.uint8).view(COR_RESULT_DTYPE)
    before = res.tobytes()
    OUT = 0x1000  # never dereferenced either

    def call(sn, tg=(6, 1), flags=0, desc=d, results=True, offs=True, tnums=True, toffs=True):
        sn = None if sn is None else np.array(sn, np.int32)
        tn = np.array(list(tg) + [0], np.int32)
        return lib.sec_repair_correct_batch(ctx, desc.ctypes.data, 1, None if sn is None else sn.ctypes.data,
                                            bo.ctypes.data if offs else None, None, None,
                                            tn.ctypes.data if tnums else None, to.ctypes.data if toffs else None, OUT,
                                            None, res.ctypes.data if results else None, None, flags)

    def desc(**kw):
        bad = d.copy()
        for f, v in kw.items():
            bad[f] = v
        return bad

    ok = [0, 2, 3, 4, 1, 5]
    assert call(ok, flags=_lib.SEC_F_STAGED | _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_STAGED) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_GPU_PARITY_IDS) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call(None) == _lib.SEC_EINVAL
    assert call(ok, offs=False) == _lib.SEC_EINVAL
    assert call(ok, results=False) == _lib.SEC_EINVAL
    assert call(ok, tnums=False) == _lib.SEC_EINVAL  # targets without their arrays
    assert call(ok, toffs=False) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(ntargets=-1)) == _lib.SEC_EINVAL
    assert call(ok, desc=desc(n=-1, k=5, m=4)) == _lib.SEC_EINVAL  # before SEC_EKM
    assert call(ok, desc=desc(k=5, m=4)) == _lib.SEC_EKM
    assert call(ok, desc=desc(k=8, m=7, n=3)) == _lib.SEC_EKM  # before SEC_ENBLOCKS
    assert call(ok, desc=desc(n=3)) == _lib.SEC_ENBLOCKS
    assert call(ok + [6, 9], desc=desc(n=8)) == _lib.SEC_ENBLOCKS  # n > m, before SEC_ESHARENUM
    assert call([0, 2, 3, 7, 1, 5]) == _lib.SEC_ESHARENUM
    assert call(ok, tg=(6, 7)) == _lib.SEC_ESHARENUM  # a target >= m
    assert call(ok, tg=(-1, 6)) == _lib.SEC_ESHARENUM
    assert call([0, 0, 3, 4, 1, 7]) == _lib.SEC_ESHARENUM  # before SEC_EDUPSHARE
    assert call([0, 2, 3, 4, 1, 3], tg=(6, 7)) == _lib.SEC_ESHARENUM
    assert call([0, 2, 3, 4, 1, 3]) == _lib.SEC_EDUPSHARE
    assert call(ok, tg=(6, 6)) == _lib.SEC_EDUPSHARE  # a repeated target
    assert call(ok, tg=(1, 1)) == _lib.SEC_EDUPSHARE  # ... also when it is a held one
    assert call([0, 2, 3, 4, 1, 3], desc=desc(B=1 << 31)) == _lib.SEC_EDUPSHARE  # before SEC_ESIZE
    assert call(ok, desc=desc(B=1 << 31)) == _lib.SEC_ESIZE
    assert call(ok, tg=(1, 0), desc=desc(B=1 << 31)) == _lib.SEC_ESIZE  # held targets: no error of their own
    assert res.tobytes() == before


def test_repair_correct_host_from_bytes(engine):
    specs = _mixed()
    items, want = [], []
    for s in specs:
        held, _ = _held(dict(s, short=False))
        items.append((s["k"], s["m"], [bytes(b) for b in held], s["entries"], s["targets"]))
        want.append(_expect(s, held))
    out, digs, results = engine.repair_correct_host(items, digests=True)
    for w, blocks, dg, got in zip(want, out, digs, results):
        assert blocks == w[0] and [bytes(x) for x in dg] == [hashlib.sha1(b).digest() for b in w[0]]
        assert got == w[1:6]
    out2, results2 = engine.repair_correct_host(items)
    assert out2 == out and results2 == results
    assert engine.repair_correct_host([]) == ([], []) and engine.repair_correct_host([], digests=True) == ([], [], [])
    assert pinned_bytes()[0] == 0
    with pytest.raises(Error):
        engine.repair_correct_host([(4, 7, [b"ab"] * 5, [0, 2, 3, 4, 5], [1, 1])])


def _encoded(ci, data, k, m, damage, lost=()):
    """An EncodedChunk of `data` and the oracle's blocks; damage: (piece_idx, offset) bytes flipped."""
    B = -(-len(data) // k)
    blocks = cfec.easy_encode(data + b"\0" * (k * B - len(data)), k, m)
    held = [bytearray(b) for b in blocks]
    for idx, at in damage:
        held[idx][at] ^= 0x01
    pieces = [piece.Piece(chunk_idx=ci, piece_idx=i, data=bytes(b),
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(held) if i not in lost]
    return piece.EncodedChunk(pieces=pieces, chunk_idx=ci, k=k, m=m, chunk_size=B, padlen=k * B - len(data),
                              original_chunk_size=len(data)), blocks


def _datas(n, count, seed):
    return [np.random.default_rng(seed + ci).integers(0, 256, n - ci, dtype=np.uint8).tobytes() for ci in range(count)]


def _ids(pieces):
    return [(p.piece_idx, p.data, p.piece_id) for p in pieces]


def _oracle_ids(blocks, idx):
    return [(i, blocks[i], hashlib.sha1(blocks[i]).hexdigest()) for i in idx]


def test_clean_repair_launches_nothing_new():
    """Clean input through piece.repair_chunks_corrected: no launch of the correcting kernels, and
    pieces and verdicts equal repair_chunks_checked's."""
    chunks = [_encoded(ci, d, 10, 14, [], lost={3, 12})[0] for ci, d in enumerate(_datas(256 << 10, 3, 500))]
    eng = get_engine()
    eng.set_timing(True)
    try:
        eng.collect_timing("decode_correct")
        eng.collect_timing("repair_check")
        got, cors = piece.repair_chunks_corrected(chunks, piece_ids=True)
        assert eng.collect_timing("decode_correct") == (0.0, 0)
        assert eng.collect_timing("repair_check")[1] >= 1  # round one, the call repair_chunks_checked makes
    finally:
        eng.set_timing(False)
    want, checks = piece.repair_chunks_checked(chunks, piece_ids=True)
    assert [_ids(row) for row in got] == [_ids(row) for row in want]
    assert [[p.piece_idx for p in row] for row in got] == [[3, 12]] * 3
    assert [(c.chunk_idx, c.checked, c.consistent, c.first_bad_offset) for c in cors] == [
        (c.chunk_idx, c.checked, c.consistent, c.first_bad_offset) for c in checks]
    assert all(c.damaged == {} and c.corrected_positions == 0 and c.open_positions == 0 for c in cors)


def test_damaged_pieces_are_healed_end_to_end():
    """RS(4,2), 256 KiB chunk, all six held, piece 1 bad at offset 100 and piece 4 bad at 9000:
    repair_chunks_checked ends located=False; the corrected repair returns both pieces equal to the
    oracle's, ids included.  The same with three pieces damaged at three offsets, where fewer than k
    undamaged pieces remain.  RS(10,4) with piece 3 lost and pieces 0 and 12 damaged: [3], then
    [0, 12]."""
    datas = _datas(256 << 10, 4, 600)
    (a, ba), (b, bb), (c, bc), (d, bd) = (
        _encoded(0, datas[0], 4, 6, []), _encoded(1, datas[1], 4, 6, [(1, 100), (4, 9000)]),
        _encoded(2, datas[2], 4, 6, [(0, 7), (3, 65000), (5, 30000)]),
        _encoded(3, datas[3], 10, 14, [(0, 5), (12, 26000)], lost={3}))
    _, checks = piece.repair_chunks_checked([a, b, c, d])
    assert not checks[1].consistent and not checks[1].located
    got, cors = piece.repair_chunks_corrected([a, b, c, d], piece_ids=True)
    assert _ids(got[0]) == []
    assert _ids(got[1]) == _oracle_ids(bb, [1, 4])
    assert _ids(got[2]) == _oracle_ids(bc, [0, 3, 5])
    assert _ids(got[3]) == _oracle_ids(bd, [3, 0, 12])
    assert [(x.consistent, x.first_bad_offset, x.corrected_positions, x.open_positions, x.damaged) for x in cors] == [
        (True, None, 0, 0, {}), (False, 100, 2, 0, {1: 1, 4: 1}), (False, 7, 3, 0, {0: 1, 3: 1, 5: 1}),
        (False, 5, 2, 0, {0: 1, 12: 1})]
    one, cor = piece.repair_pieces_corrected(b)
    assert [(p.piece_idx, p.data) for p in one] == [(1, bb[1]), (4, bb[4])] and cor == cors[1]
    assert pinned_bytes()[0] == 0
