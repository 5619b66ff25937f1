"""GPU: sec_decode_correct_ex_batch and sec_repair_correct_ex_batch (several errors per byte position)
against expectations that never come from the code under test.  Blocks = cfec.easy_encode(chunk, k,
m); damage is XORed into the buffer image in numpy at places the test chose.  With r = n - k and
t = min(max_errors or r // 2, r // 2, 16): the expected output is the ORIGINAL chunk (the oracle's
blocks, for a repair) wherever a position carries at most t flips, the expected hits are the flips
put in, the expected open positions are those carrying t + 1 .. r - t flips, and there the outputs
are what the basis as held gives (cfec.easy_decode / easy_encode of it).

Chunk specs and the layout discipline are tests/test_gpu_decode_correct.py's and
tests/test_gpu_repair_correct.py's: every entry in a buffer of 0xFF at odd and even starts, short
block k-1 followed by 0xFF, the source byte-identical after every call, `out` 0xFF-filled and
compared whole, guard bytes included.  Device mode and host mode run for every layout."""

import functools
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import COR_RESULT_DTYPE, DCHK_DTYPE, RCHK_DTYPE  # noqa: E402
from storb_amd.engine import Engine, check_correct, get_engine, pinned_bytes  # noqa: E402
from tests.test_gpu_decode_correct import (UNTOUCHED, _chunk, _edges, _held, _mixed, _opt, _out_diff,  # noqa: E402
                                           flipped, spec)


def bound(nr, T):
    t = min(nr // 2, 16)
    return t if T == 0 else min(t, T)


@functools.lru_cache(maxsize=None)
def _as_held_blocks(k, m, entries, basis):
    """The m blocks of the code word the basis as held spans."""
    whole = cfec.easy_decode(list(basis), list(entries), 0, k, m)
    return cfec.easy_encode(whole, k, m)


def _expect(s, held, T, targets=None, unspecified=False):
    """(outputs, first, first_open, corrected, open, hits per entry).  outputs: the decoded bytes, or
    with targets the list of target blocks."""
    k, m, B, n = s["k"], s["m"], s["B"], len(s["entries"])
    data, blocks = _chunk(k, m, B, s["padlen"], s["seed"])
    nr = n - k
    t = bound(nr, T)
    at = {}
    for e, p, _ in s["flips"]:
        at.setdefault(p, []).append(e)
    basis = tuple(bytes(h) + b"\0" * (B - len(h)) for h in held[:k])
    pred = _as_held_blocks(k, m, tuple(s["entries"][:k]), basis)
    if targets is None:
        exp = [bytearray(data if nr else b"".join(pred[:k])[:len(data)])]
    else:
        exp = [bytearray(blocks[g] if nr else pred[g]) for g in targets]
    hits, opened, ncor = [0] * n, [], 0
    for p, es in sorted(at.items() if nr else ()):
        if len(es) <= t:
            ncor += 1
            for e in es:
                hits[e] += 1
            continue
        assert unspecified or len(es) <= nr - t, "beyond r - t flips the verdict is unspecified"
        opened.append(p)
        if targets is None:
            for row in range(k):
                if row * B + p < len(exp[0]):
                    exp[0][row * B + p] = pred[row][p]
        else:
            for q, g in enumerate(targets):
                exp[q][p] = pred[g][p]
    out = bytes(exp[0]) if targets is None else [bytes(x) for x in exp]
    first = min(at) if at and nr else None
    return out, first, min(opened) if opened else None, ncor, len(opened), hits


def _layout(cases, T, form, unspecified=False):
    """cases: specs (decode) or (spec, targets) pairs (repair)."""
    repair = form == "repair"
    descs = np.zeros(len(cases), dtype=RCHK_DTYPE if repair else DCHK_DTYPE)
    sn, bo, av, tn, to, want, parts, outs, specs = [], [], [], [], [], [], [], [], []
    cur, ocur = 3, 7
    for i, case in enumerate(cases):
        s, targets = case if repair else (case, None)
        specs.append(s)
        k, B, n = s["k"], s["B"], len(s["entries"])
        held, avail = _held(s)
        w = _expect(s, held, T, targets, unspecified)
        want.append(w[1:])
        if repair:
            descs[i] = (B, len(sn), len(tn), len(targets), n, k, s["m"])
            for q, g in enumerate(targets):
                tn.append(g)
                to.append(ocur)
                outs.append((ocur, w[0][q]))
                ocur += B + 9 + (q % 2)
        else:
            descs[i] = (ocur, B, s["padlen"], len(sn), n, k, s["m"], 0)
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
    dig = np.frombuffer(b"".join(hashlib.sha1(b).digest() for _, b in outs), np.uint8) if repair else None
    return SimpleNamespace(descs=descs, sn=np.array(sn, np.int32), bo=np.array(bo, np.uint64),
                           av=np.array(av, np.uint64), tn=np.array(tn + [0], np.int32)[:len(tn)],
                           to=np.array(to + [0], np.uint64)[:len(to)], src=src, out=out, dig=dig, want=want,
                           specs=specs, T=T, repair=repair)


def _verify(L, res, hits):
    res = np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=COR_RESULT_DTYPE)
    for i, (s, w) in enumerate(zip(L.specs, L.want)):
        first, first_open, corrected, opened, want_hits = w
        s0, n = int(L.descs[i]["slot0"]), len(s["entries"])
        got = (_opt(res[i]["first"]), _opt(res[i]["first_open"]), int(res[i]["corrected"]), int(res[i]["open"]))
        assert got == (first, first_open, corrected, opened), f"chunk {i}: {got}"
        if hits is not None:
            assert hits[s0:s0 + n].tolist() == want_hits, f"chunk {i}: hits"


def _call(engine, L, blocks, bo, out, res, hits, dig, T=None, **kw):
    T = L.T if T is None else T
    if L.repair:
        engine.repair_correct_batch(L.descs, L.sn, bo, blocks, L.tn, L.to, out, res, block_avail=L.av, digests=dig,
                                    entry_hits=hits, max_errors=T, **kw)
    else:
        engine.decode_correct_batch(L.descs, L.sn, bo, blocks, out, res, block_avail=L.av, entry_hits=hits,
                                    max_errors=T, **kw)


def device_call(engine, L, dsrc, T=None, asynchronous=False, with_hits=True):
    """-> (out, results, hits, digests) as numpy, after checking the source is untouched"""
    dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
    res = torch.zeros(24 * len(L.specs), dtype=torch.uint8, device="cuda")
    hits = torch.from_numpy(np.full(len(L.sn), UNTOUCHED, np.uint32).view(np.int32)).cuda() if with_hits else None
    dig = torch.zeros(max(L.dig.size, 1), dtype=torch.uint8, device="cuda") if L.repair else None
    _call(engine, L, 0, L.bo + np.uint64(dsrc.data_ptr()), dout, res, hits, dig, T, asynchronous=asynchronous)
    if asynchronous:
        engine.sync()
    assert np.array_equal(dsrc.cpu().numpy(), L.src), "the source buffer was written"
    return (dout.cpu().numpy(), res.cpu().numpy(), hits.cpu().numpy().view(np.uint32) if with_hits else None,
            dig.cpu().numpy()[:L.dig.size] if L.repair else None)


def run_device(engine, L, dsrc=None, **kw):
    if dsrc is None:
        dsrc = torch.from_numpy(L.src).cuda()
    out, res, hits, dig = device_call(engine, L, dsrc, **kw)
    assert not _out_diff(out, L.out)
    if L.repair:
        assert dig.tobytes() == L.dig.tobytes()
    _verify(L, res, hits)
    return dsrc


def run_host(eng, L):
    src = L.src.copy()
    out = np.full(L.out.size, 0xFF, np.uint8)
    res = np.zeros(len(L.specs), dtype=COR_RESULT_DTYPE)
    hits = np.full(len(L.sn), UNTOUCHED, np.uint32)
    dig = np.zeros(max(L.dig.size, 1), np.uint8) if L.repair else None
    _call(eng, L, src, L.bo, out, res, hits, dig, host=True)
    assert np.array_equal(src, L.src), "the source buffer was written"
    assert not _out_diff(out, L.out)
    if L.repair:
        assert dig[:L.dig.size].tobytes() == L.dig.tobytes()
    _verify(L, res, hits)


def run_both(engine, cases, T=0, form="decode"):
    L = _layout(cases, T, form)
    run_device(engine, L)
    run_host(engine, L)


FORMS = ["decode", "repair"]


def _cases(form, specs, targets):
    """The specs as they are (decode), or each with targets of `targets` (repair): lost blocks where
    the chunk lacks some, held ones (heal targets) too."""
    if form == "decode":
        return specs
    return [(s, [g for g in targets if g < s["m"]]) for s in specs]


# zfec(10,14), all 14 held (r = 4, t = 2), B = 6554, padlen 4, block 9 short.  A: piece 0 and the short
# block in the basis; C: both among the check rows.
Z_A = spec(10, 14, 6554, [3, 0, 9, 1, 7, 5, 6, 2, 8, 4, 12, 10, 13, 11], padlen=4, short=True)
Z_C = spec(10, 14, 6554, [3, 13, 12, 1, 7, 5, 6, 2, 8, 4, 0, 10, 9, 11], padlen=4, short=True)


def _pairs_1014(s):
    """One flip at every edge position + 1 and two at every edge position: basis + basis, basis +
    check and check + check in turn, each once with piece 0 and once with the short entry (another
    entry stands in for the short one behind its avail)."""
    ent = s["entries"]
    zero, short = ent.index(0), ent.index(9)
    avail = s["B"] - s["padlen"]
    basis = [j for j in range(10) if j not in (zero, short)]
    check = [j for j in range(10, 14) if j not in (zero, short)]
    # the partner's kind changes every second position, so piece 0 and the short entry meet both kinds:
    # basis + basis and basis + check (A), check + check and check + basis (C)
    partners = [basis[0], check[0]] if zero < 10 else [check[0], basis[1]]
    flips, q = [], 0
    for p in _edges(s["B"]):
        a = (zero, short)[q % 2]
        if a == short and p >= avail:
            a = basis[5]
        flips += [(a, p, 1 + p % 255), (partners[q // 2 % 2], p, 0x80 | (q + 1))]
        if p + 1 < s["B"] and p + 1 not in _edges(s["B"]):
            one = (zero, short, basis[2], check[-1])[q % 4]
            flips.append((one if not (one == short and p + 1 >= avail) else check[-1], p + 1, 0x33))
        q += 1
    return flipped(s, *flips)


@pytest.mark.parametrize("form", FORMS)
def test_1014_one_and_two_flips_at_every_edge(engine, form):
    specs = [_pairs_1014(Z_A), _pairs_1014(Z_C)]
    L = _layout(_cases(form, specs, [5, 0, 13, 9]), 0, form)
    assert all(w[3] == 0 and w[2] > 10 and max(w[4]) >= 2 for w in L.want)
    run_device(engine, L)
    run_host(engine, L)


@pytest.mark.parametrize("form", FORMS)
def test_1014_max_errors_1_equals_the_one_error_call(engine, form):
    """The same layout with max_errors = 1: every two-flip position is open, and results, hits, digests
    and every output byte equal the existing call's on the same buffers."""
    L = _layout(_cases(form, [_pairs_1014(Z_A), _pairs_1014(Z_C)], [5, 0, 13, 9]), 1, form)
    assert all(w[3] >= 10 for w in L.want)
    dsrc = run_device(engine, L)
    run_host(engine, L)
    # T = 1 through the Python layer is the existing call; the _ex entry itself with max_errors = 1:
    lib = engine.lib
    ex = lib.sec_repair_correct_ex_batch if L.repair else lib.sec_decode_correct_ex_batch
    old = lib.sec_repair_correct_batch if L.repair else lib.sec_decode_correct_batch
    got = []
    for fn, extra in ((old, ()), (ex, (1,))):
        dout = torch.full((L.out.size,), 0xFF, dtype=torch.uint8, device="cuda")
        res = torch.zeros(24 * len(L.specs), dtype=torch.uint8, device="cuda")
        hits = torch.zeros(len(L.sn), dtype=torch.int32, device="cuda")
        dig = torch.zeros(max(20 * len(L.tn), 1), dtype=torch.uint8, device="cuda")
        bo = L.bo + np.uint64(dsrc.data_ptr())
        args = [L.sn.ctypes.data, bo.ctypes.data, L.av.ctypes.data, None]
        if L.repair:
            args += [L.tn.ctypes.data, L.to.ctypes.data, dout.data_ptr(), dig.data_ptr()]
        else:
            args += [dout.data_ptr()]
        assert fn(engine._ctx, L.descs.ctypes.data, len(L.descs), *args, res.data_ptr(), hits.data_ptr(), *extra,
                  0) == _lib.SEC_OK
        got.append((dout.cpu().numpy(), np.frombuffer(res.cpu().numpy().tobytes(), COR_RESULT_DTYPE),
                    hits.cpu().numpy(), dig.cpu().numpy()))
    for f in COR_RESULT_DTYPE.names:
        assert np.array_equal(got[0][1][f], got[1][1][f]), f
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], L.out)
    assert np.array_equal(got[0][2], got[1][2]) and np.array_equal(got[0][3], got[1][3])


Z_13 = spec(10, 14, 6554, [3, 0, 9, 1, 7, 5, 6, 2, 8, 4, 12, 10, 13], padlen=4, short=True)  # r = 3, t = 1


@pytest.mark.parametrize("form", FORMS)
def test_1014_thirteen_held_two_flips_are_open(engine, form):
    s = flipped(Z_13, (1, 17), (12, 17, 0x21), (4, 6552), (5, 6552, 0x04), (11, 300), (0, 6549))
    L = _layout(_cases(form, [s], [11, 9, 3]), 0, form)
    assert L.want[0][:4] == (17, 17, 2, 2)
    run_device(engine, L)
    run_host(engine, L)


_P16 = [s for s in range(16) if s not in (0, 5)]
Z1624_22 = spec(16, 24, 259, _P16[::-1] + [19, 16] + [23, 17, 20, 18, 22, 21])  # pieces 0, 5 absent; r = 6, t = 3
Z1624_23 = spec(16, 24, 259, _P16[::-1] + [19, 16] + [23, 17, 20, 18, 22, 21, 0])  # r = 7, t = 3


@pytest.mark.parametrize("form", FORMS)
def test_1624_three_flips_corrected_four_open(engine, form):
    three = flipped(Z1624_22, (14, 7), (3, 7, 0x11), (20, 7, 0xF0), (15, 258), (2, 258, 0x02), (16, 258, 0x9),
                    (0, 100), (1, 100, 0x40), (21, 31), (17, 31, 0x7), (18, 31, 0x77))
    four = flipped(Z1624_23, (14, 7), (3, 7, 0x11), (20, 7, 0xF0), (22, 7, 0x3), (5, 200), (6, 200, 0x6),
                   (7, 200, 0x7), (22, 16), (0, 16, 0x2))
    L = _layout(_cases(form, [three, four, Z1624_22], [0, 5, 3, 19, 23]), 0, form)
    assert L.want[0][:4] == (7, None, 4, 0) and L.want[1][:4] == (7, 7, 2, 1)
    run_device(engine, L)
    run_host(engine, L)


_B32 = [40, 33] + [s for s in range(32) if s not in (0, 13)][::-1]
Z3248 = spec(32, 48, 130, _B32 + [0, 13] + [s for s in range(32, 48) if s not in (40, 33)], padlen=3, short=True)
Z6496_ALL = spec(64, 96, 33, list(range(95, 31, -1)) + list(range(32)))
Z6496_80 = spec(64, 96, 33, list(range(1, 64)) + [64] + list(range(65, 81)))  # data piece 0 absent: r = 16, t = 8


@pytest.mark.parametrize("form", FORMS)
def test_3248_eight_flips(engine, form):
    """All 48 held (t = 8 = r - t: no flip count is always open): eight flips at one position, check
    rows of the second 8-row group among them, at a lane position and in the ragged end."""
    ent = [0, 5, 31, 32, 33, 32 + 9, 32 + 12, 47]  # piece 0 is entry 32, a check row; entry 2 is the short one
    s = flipped(Z3248, *[(e, 64, 1 + e) for e in ent], *[(e, 129, 0x80 | e) for e in ent], (46, 128), (1, 128, 0x3))
    L = _layout(_cases(form, [s], [0, 13, 40, 47]), 0, form)
    assert L.want[0][:4] == (64, None, 3, 0)
    run_device(engine, L)
    run_host(engine, L)


@pytest.mark.parametrize("form", FORMS)
def test_6496_sixteen_and_eight_flips(engine, form):
    sixteen = list(range(0, 96, 6))
    a = flipped(Z6496_ALL, *[(e, 32, 1 + e) for e in sixteen], *[(e, 3, 0xFF - e) for e in sixteen[1:]], (95, 3, 0x1),
                (40, 15), (70, 16, 0x2))
    eight = [0, 7, 62, 63, 64, 70, 78, 79]
    b = flipped(Z6496_80, *[(e, 0, 1 + e) for e in eight], *[(e, 17, 0x40 | e) for e in eight], (5, 32, 0x02))
    L = _layout(_cases(form, [a, b], [0, 63, 64, 95]), 0, form)
    assert L.want[0][:4] == (3, None, 4, 0) and L.want[1][:4] == (0, None, 3, 0)
    run_device(engine, L)
    run_host(engine, L)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [1, 5, 15, 16, 17, 63, 257, 4099])
def test_812_block_sizes(engine, B, form):
    """zfec(8,12), all held (t = 2): the tail kernel only, one lane, the straddling lane, several
    lanes, a second tile; two flips at each edge position."""
    s = spec(8, 12, B, [7, 0, 2, 10, 4, 5, 6, 1, 8, 9, 3, 11])
    ps = _edges(B)
    two = [f for q, p in enumerate(ps) for f in ((q % 8, p, 1 + p % 255), (8 + q % 4 if q % 2 else (q + 3) % 8, p, 0x81))]
    run_both(engine, _cases(form, [s, flipped(s, *two)], [3, 7, 11]), 0, form)


def test_rs46_mixed_batch_with_the_codes_limit(engine):
    """Every case of the existing mixed batch with max_errors = 0: wherever r = 2 the bound is 1 and
    the expectations are today's."""
    L = _layout(_mixed(), 0, "decode")
    run_device(engine, L)
    run_host(engine, L)


def _junk2(s, entries, seed):
    """`s` with whole entries replaced by random bytes -> (spec, positions where any differs)"""
    _, blocks = _chunk(s["k"], s["m"], s["B"], s["padlen"], s["seed"])
    flips, bad = [], np.zeros(s["B"], bool)
    for q, e in enumerate(entries):
        true = np.frombuffer(blocks[s["entries"][e]], np.uint8)
        diff = true ^ np.random.default_rng(seed + q).integers(0, 256, true.size, dtype=np.uint8)
        flips += [(e, int(p), int(diff[p])) for p in np.flatnonzero(diff)]
        bad |= diff != 0
    return flipped(s, *flips), int(bad.sum())


Z_JUNK = spec(10, 14, 4099, [3, 0, 9, 1, 7, 5, 6, 2, 8, 4, 12, 10, 13, 11])


@pytest.mark.parametrize("form", FORMS)
def test_two_whole_pieces_of_junk(engine, form):
    s, nbad = _junk2(Z_JUNK, (4, 12), 99)
    L = _layout(_cases(form, [s], [7, 13]), 0, form)
    first, first_open, corrected, opened, hits = L.want[0]
    assert 4090 < nbad <= 4099 and corrected == nbad and opened == 0
    assert [j for j, h in enumerate(hits) if h] == [4, 12] and min(hits[4], hits[12]) > 4000
    run_device(engine, L)
    run_host(engine, L)


@pytest.mark.parametrize("form", FORMS)
def test_beyond_r_minus_t_the_verdict_is_unspecified(engine, form):
    """zfec(10,14), three flips at one position (r - t + 1): corrected to another code word or open.
    The source is untouched, every byte of `out` away from that position is as expected, and
    corrected + open counts the damaged positions."""
    s = flipped(Z_JUNK, (0, 1000), (5, 1000, 0x3), (11, 1000, 0x70), (2, 77))
    L = _layout(_cases(form, [s], [7, 13, 5]), 0, form, unspecified=True)
    dsrc = torch.from_numpy(L.src).cuda()
    out, res, hits, _ = device_call(engine, L, dsrc)
    res = np.frombuffer(res.tobytes(), COR_RESULT_DTYPE)
    assert int(res[0]["corrected"]) + int(res[0]["open"]) == 2 and int(res[0]["first"]) == 77
    assert hits[2] >= 1 and 1 <= int(hits.sum()) <= 3
    B = s["B"]
    starts = [int(x) for x in L.to] if L.repair else [int(L.descs[0]["out_off"]) + r * B for r in range(10)]
    differs = set(np.flatnonzero(out != L.out).tolist())
    assert differs <= {o + 1000 for o in starts}
    # host mode: the same verdict, the same bytes
    src = L.src.copy()
    hout = np.full(L.out.size, 0xFF, np.uint8)
    hres = np.zeros(1, dtype=COR_RESULT_DTYPE)
    hhits = np.full(len(L.sn), UNTOUCHED, np.uint32)
    dig = np.zeros(max(L.dig.size, 1), np.uint8) if L.repair else None
    _call(engine, L, src, L.bo, hout, hres, hhits, dig, host=True)
    assert np.array_equal(src, L.src), "the source buffer was written"
    assert int(hres[0]["corrected"]) + int(hres[0]["open"]) == 2 and int(hres[0]["first"]) == 77
    assert np.array_equal(hout, out) and np.array_equal(hhits, hits) and hres.tobytes() == res.tobytes()


def test_rs47_mixed_repair_batch_with_the_codes_limit(engine):
    """Every case of the corrected repair's mixed batch with max_errors = 0, by this file's rule."""
    from tests.test_gpu_repair_correct import _mixed as repair_mixed
    L = _layout([(s, s["targets"]) for s in repair_mixed()], 0, "repair")
    run_device(engine, L)
    run_host(engine, L)


# Chunks whose tables have the same rows (targets, then check rows) over the same basis but another
# split between the two: their held entries differ, and so do the points and weights behind the rows.
_SPLIT_A = (flipped(spec(4, 10, 257, [0, 1, 2, 3, 6, 7, 8]), (5, 100), (2, 256, 0x3)), [5])        # rows 5 | 6 7 8
_SPLIT_B = (flipped(spec(4, 10, 257, [0, 1, 2, 3, 7, 8]), (4, 100), (1, 17, 0x9)), [5, 6])         # rows 5 6 | 7 8
_SPLIT_C = (flipped(spec(10, 14, 130, list(range(10)) + [11, 12, 13]), (11, 5), (3, 129)), [10])  # 10 | 11 12 13
_SPLIT_D = (flipped(spec(10, 14, 130, list(range(10)) + [12, 13]), (10, 5), (0, 64, 0x7)), [10, 11])


@pytest.mark.parametrize("order", [0, 1])
def test_same_rows_another_split_in_one_batch(engine, order):
    cases = [_SPLIT_A, _SPLIT_B, _SPLIT_C, _SPLIT_D]
    L = _layout(cases[::-1] if order else cases, 0, "repair")
    assert all(w[2:4] == (2, 0) for w in L.want)
    run_device(engine, L)
    run_host(engine, L)


def test_same_rows_another_split_call_after_call():
    """One engine, so one table cache: a repair, then a repair and a decode whose rows are the same
    with the split elsewhere, then the first again."""
    dec = flipped(spec(4, 10, 257, [0, 1, 2, 7, 5, 6, 8, 9]), (6, 100), (3, 200, 0x11), (0, 200, 0x2))  # rows 3 | 5 6 8 9
    rep = (flipped(spec(4, 10, 257, [0, 1, 2, 7, 6, 8, 9]), (5, 100), (3, 200, 0x11)), [3, 5])          # rows 3 5 | 6 8 9
    eng = Engine(0)
    try:
        for _ in range(2):
            run_device(eng, _layout([_SPLIT_A], 0, "repair"))
            run_device(eng, _layout([_SPLIT_B], 0, "repair"))
            run_device(eng, _layout([dec], 0, "decode"))
            run_device(eng, _layout([rep], 0, "repair"))
            run_device(eng, _layout([(dec, [3])], 0, "repair"))  # the decode's rows and split, as a repair
    finally:
        eng.close()


def test_same_rows_another_split_through_the_piece_layer():
    """zfec(10,14), heal=False: one chunk lost piece 10, the other pieces 10 and 11; both ask for rows
    10 11 12 13, and each has one wrong byte, which is always put right."""
    datas = _datas(10 * 300, 2, 40)
    a = _encoded(0, datas[0], 10, 14, [(12, 7, 0x1)])
    b = _encoded(1, datas[1], 10, 14, [(3, 250, 0x80)])
    want = [{p.piece_idx: p.data for p in _encoded(ci, d, 10, 14, []).pieces} for ci, d in enumerate(datas)]
    a.pieces = [p for p in a.pieces if p.piece_idx != 10]
    b.pieces = [p for p in b.pieces if p.piece_idx not in (10, 11)]
    for chunks in ([a, b], [b, a]):
        pieces, cks = piece.repair_chunks_corrected(chunks, heal=False, max_errors=None)
        for ch, ps, ck in zip(chunks, pieces, cks):
            assert (ck.corrected_positions, ck.open_positions) == (1, 0)
            assert [p.piece_idx for p in ps] == ([10] if ch is a else [10, 11])
            assert all(p.data == want[ch.chunk_idx][p.piece_idx] for p in ps)


def _all_cases(form):
    specs = [_pairs_1014(Z_A), Z_A, flipped(Z_13, (1, 17), (12, 17, 0x21), (11, 300)),
             flipped(Z1624_22, (14, 7), (3, 7, 0x11), (20, 7, 0xF0)),
             flipped(Z1624_23, (14, 7), (3, 7, 0x11), (20, 7, 0xF0), (22, 7, 0x3)),
             flipped(Z3248, *[(e, 129, 0x80 | e) for e in (0, 5, 31, 32, 33, 41, 44, 47)]),
             flipped(Z6496_ALL, *[(e, 32, 1 + e) for e in range(0, 96, 6)]), Z6496_80,
             flipped(spec(8, 12, 5, list(range(12))), (1, 4), (9, 4, 0x2)),
             flipped(spec(8, 12, 17, list(range(12))), (0, 16), (11, 16, 0x2), (3, 0)),
             _junk2(spec(10, 14, 63, Z_JUNK["entries"]), (4, 12), 5)[0],
             flipped(spec(4, 6, 257, [5, 0, 3, 2, 4, 1]), (4, 100), (0, 256)), spec(4, 6, 17, [0, 1, 2, 3])]
    return _cases(form, specs, [0, 5, 9, 13, 47, 95])


@pytest.mark.parametrize("form", FORMS)
def test_mixed_batch_twice_from_the_cached_plan(engine, form):
    """Every shape of this file in one call; then the same plan on data changed in place to be all
    clean: no count is left over; then SEC_F_ASYNC without hits; then host mode."""
    cases = _all_cases(form)
    clean = [flipped(c) if form == "decode" else (flipped(c[0]), c[1]) for c in cases]
    L1, L2 = _layout(cases, 0, form), _layout(clean, 0, form)
    assert L1.descs.tobytes() == L2.descs.tobytes() and np.array_equal(L1.bo, L2.bo)
    assert all(w[:4] == (None, None, 0, 0) for w in L2.want)
    dsrc = run_device(engine, L1)
    dsrc.copy_(torch.from_numpy(L2.src))
    run_device(engine, L2, dsrc)
    run_device(engine, L1, asynchronous=True, with_hits=False)
    run_host(engine, L1)


@pytest.mark.parametrize("form", FORMS)
def test_host_mode_is_staged_over_several_slabs(form):
    eng = Engine(0, options={"SEC_SLAB_BYTES": 1 << 16})
    try:
        run_host(eng, _layout(_all_cases(form), 0, form))
        assert eng.host_paths() == (0, 0, 1)
        assert eng.check_methods() == (0, 0) and eng.repair_methods() == (0, 0)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_repair_with_fewer_than_k_undamaged_pieces(engine):
    """zfec(10,14), all held, five pieces damaged at five different offsets: nine undamaged pieces
    are left, and every target, the five damaged pieces healed, comes back as the oracle's block."""
    s = flipped(Z_JUNK, (0, 5), (3, 600, 0x7), (9, 601, 0x1), (11, 4000, 0xFE), (13, 4098, 0x80))
    targets = [s["entries"][e] for e in (0, 3, 9, 11, 13)] + [6]
    L = _layout([(s, targets)], 0, "repair")
    assert L.want[0][:4] == (5, None, 5, 0)
    run_device(engine, L)
    run_host(engine, L)
    run_both(engine, [(s, targets)], 1, "repair")  # one wrong piece per position: the existing call does it too


def test_the_host_model_agrees_on_damaged_columns(engine):
    """A second witness for the counts above: engine.check_correct on the damaged columns of the
    (16,24) case names the entries the test damaged."""
    s = flipped(Z1624_22, (14, 7), (3, 7, 0x11), (20, 7, 0xF0))
    held, _ = _held(s)
    col = bytes(h[7] for h in held)
    fixed, changed = check_correct(16, 24, s["entries"], col, 0)
    assert changed == 3 and [j for j in range(22) if fixed[j] != col[j]] == [3, 14, 20]
    assert check_correct(16, 24, s["entries"], col, 2)[1] == -2


def test_timing_kind_and_methods(engine):
    engine.set_timing(True)
    try:
        for kind in ("decode_correct", "decode_check", "repair_check", "decode", "check"):
            engine.collect_timing(kind)
        before = (engine.check_methods(), engine.repair_methods())
        run_device(engine, _layout([flipped(Z1624_22, (3, 100), (4, 100, 0x2))], 0, "decode"))
        run_device(engine, _layout([(flipped(Z1624_22, (3, 100), (4, 100, 0x2)), [0, 3])], 0, "repair"))
        ms, launches = engine.collect_timing("decode_correct")
        assert launches == 2 and ms > 0
        for kind in ("decode_check", "repair_check", "decode", "check"):
            assert engine.collect_timing(kind) == (0.0, 0)
        assert (engine.check_methods(), engine.repair_methods()) == before
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    """max_errors < 0 is SEC_EINVAL, with the other SEC_EINVALs and before SEC_EKM; the flags refused
    are the existing calls'; the rest of the order is theirs."""
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=DCHK_DTYPE)
    d[0] = (0, 64, 3, 0, 6, 4, 6, 0)
    r = np.zeros(1, dtype=RCHK_DTYPE)
    r[0] = (64, 0, 0, 1, 5, 4, 6)
    bo = np.zeros(8, np.uint64)  # never dereferenced: every call fails first
    res = np.full(24, 0x77, dtype=np.uint8).view(COR_RESULT_DTYPE)
    before = res.tobytes()
    tn, to = np.array([5], np.int32), np.zeros(1, np.uint64)
    OUT = 0x1000  # never dereferenced either

    def dec(sn, T=0, flags=0, desc=d):
        sn = np.array(sn, np.int32)
        return lib.sec_decode_correct_ex_batch(ctx, desc.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                               OUT, res.ctypes.data, None, T, flags)

    def rep(sn, T=0, flags=0, desc=r):
        sn = np.array(sn, np.int32)
        return lib.sec_repair_correct_ex_batch(ctx, desc.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                               tn.ctypes.data, to.ctypes.data, OUT, None, res.ctypes.data, None, T,
                                               flags)

    def bad(desc, **kw):
        desc = desc.copy()
        for f, v in kw.items():
            desc[f] = v
        return desc

    ok = [0, 2, 3, 4, 1, 5]
    for call, desc in ((dec, d), (rep, r)):
        assert call(ok[:int(desc[0]["n"])], T=-1) == _lib.SEC_EINVAL
        assert call(ok, T=-1, desc=bad(desc, k=5, m=4)) == _lib.SEC_EINVAL  # before SEC_EKM
        assert call(ok, desc=bad(desc, k=5, m=4)) == _lib.SEC_EKM
        assert call(ok, flags=_lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
        assert call(ok, flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC) == _lib.SEC_EINVAL
        assert call(ok, desc=bad(desc, n=-1, k=5, m=4)) == _lib.SEC_EINVAL
        assert call(ok, desc=bad(desc, n=3)) == _lib.SEC_ENBLOCKS
        assert call([0, 2, 3, 6, 1, 5][:int(desc[0]["n"])]) == _lib.SEC_ESHARENUM
        assert call([0, 2, 3, 3, 1, 5][:int(desc[0]["n"])]) == _lib.SEC_EDUPSHARE
        assert call(ok, desc=bad(desc, B=1 << 31)) == _lib.SEC_ESIZE
    assert dec(ok, desc=bad(d, padlen=4 * 64 + 1)) == _lib.SEC_EPADLEN
    assert res.tobytes() == before


def _encoded(ci, data, k, m, damage):
    """An EncodedChunk of `data` with every piece held; damage: (piece_idx, offset, xor) bytes flipped."""
    B = -(-len(data) // k)
    held = [bytearray(b) for b in cfec.easy_encode(data + b"\0" * (k * B - len(data)), k, m)]
    for idx, at, v in damage:
        held[idx][at] ^= v
    pieces = [piece.Piece(chunk_idx=ci, piece_idx=i, data=bytes(b),
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(held)]
    return piece.EncodedChunk(pieces=pieces, chunk_idx=ci, k=k, m=m, chunk_size=B, padlen=k * B - len(data),
                              original_chunk_size=len(data))


def _datas(n, count, seed):
    return [np.random.default_rng(seed + ci).integers(0, 256, n - ci, dtype=np.uint8).tobytes() for ci in range(count)]


def test_two_pieces_damaged_at_the_same_offsets_end_to_end():
    """zfec(16,24), pieces 2 and 19 damaged at the same offsets: the default still raises, and
    max_errors=None returns the data, heals both pieces, and streams the same bytes."""
    datas = _datas(64 << 10, 3, 800)
    damage = [(2, 10, 0x1), (19, 10, 0x2), (2, 4000, 0xFF), (19, 4000, 0x80)]
    chunks = [_encoded(0, datas[0], 16, 24, []), _encoded(1, datas[1], 16, 24, damage),
              _encoded(2, datas[2], 16, 24, [(23, 0, 0x1)])]
    pieces = [p for ch in chunks for p in ch.pieces]
    with pytest.raises(piece.PieceCorrectionError):
        piece.reconstruct_data_corrected(pieces, chunks)
    data, cors = piece.reconstruct_data_corrected(pieces, chunks, max_errors=None)
    assert data == b"".join(datas)
    assert [(c.consistent, c.first_bad_offset, c.corrected_positions, c.open_positions, c.damaged) for c in cors] == [
        (True, None, 0, 0, {}), (False, 10, 2, 0, {2: 2, 19: 2}), (False, 0, 1, 0, {23: 1})]
    assert b"".join(d for d, _ in piece.reconstruct_data_stream_corrected(pieces, chunks, max_errors=None)) == data
    clean = _encoded(1, datas[1], 16, 24, [])
    healed, ck = piece.repair_pieces_corrected(chunks[1], max_errors=None)
    assert [p.piece_idx for p in healed] == [2, 19] and ck.damaged == {2: 2, 19: 2} and ck.open_positions == 0
    assert all(p.data == clean.pieces[p.piece_idx].data for p in healed)
    _, ck = piece.repair_pieces_corrected(chunks[1])  # the default: one piece per offset, so both offsets are open
    assert ck.open_positions == 2 and ck.corrected_positions == 0
    assert pinned_bytes()[0] == 0


def test_clean_download_through_the_new_keyword_launches_nothing_new():
    datas = _datas(64 << 10, 2, 900)
    chunks = [_encoded(ci, d, 16, 24, []) for ci, d in enumerate(datas)]
    eng = get_engine()
    eng.set_timing(True)
    try:
        eng.collect_timing("decode_correct")
        got, cors = piece.decode_chunks_corrected(chunks, max_errors=None)
        assert eng.collect_timing("decode_correct") == (0.0, 0)
    finally:
        eng.set_timing(False)
    assert got == b"".join(datas)
    assert all(c.damaged == {} and c.corrected_positions == 0 and c.open_positions == 0 for c in cors)
