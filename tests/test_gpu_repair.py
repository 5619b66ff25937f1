"""GPU: sec_repair_batch against the oracle.  Expected bytes never come from another HIP path:
blocks = cfec.easy_encode(chunk, k, m) (oracle/fec_oracle.c), the sources are blocks[s], target t
must equal blocks[t] and its digest hashlib.sha1(blocks[t]).

Layout of every device case: each target sits in a larger buffer at an odd offset (1 or 33
modulo 64) between runs of 0xA5 of at least 64 bytes, and everything outside the targets must
still be 0xA5 afterwards; each source sits in a buffer of 0xFF, so a short source (block_avail <
B) is followed by 0xFF bytes and a read past its avail shows up as wrong output."""

import functools
import hashlib
import random

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd import _lib, piece  # noqa: E402
from storb_amd._lib import REP_DTYPE  # noqa: E402
from storb_amd.engine import Error, pinned_bytes  # noqa: E402

GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def _blocks(k, m, B, padlen, seed):
    """The oracle's m blocks of a seeded chunk of k*B - padlen bytes (block k-1 zero-padded)."""
    n = k * B - padlen
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes() + b"\0" * padlen
    blocks = cfec.easy_encode(data, k, m)
    assert len(blocks) == m and all(len(b) == B for b in blocks)
    assert blocks[k - 1][B - padlen:] == b"\0" * padlen
    return blocks


def spec(k, m, B, src, tg, padlen=0, short=False, seed=None):
    """One chunk: sources `src` (in that order), targets `tg`; short: source k-1 is handed over
    with block_avail = B - padlen (zfec's padded block read in place)."""
    assert len(src) == k and not set(src) & set(tg)
    return dict(k=k, m=m, B=B, src=list(src), tg=list(tg), padlen=padlen, short=short,
                seed=seed if seed is not None else 1000 * k + m + B)


def _layout(specs):
    """Host images of the source and target buffers, the call's arrays with offsets relative to
    the two buffers, and the expected bytes."""
    descs = np.zeros(len(specs), dtype=REP_DTYPE)
    sn, bo, av, tn, to, want = [], [], [], [], [], []
    scur, tcur = 3, 0
    src_parts, tgt_ranges = [], []
    for i, s in enumerate(specs):
        blocks = _blocks(s["k"], s["m"], s["B"], s["padlen"], s["seed"])
        B = s["B"]
        descs[i] = (B, len(sn), len(tn), len(s["tg"]), s["k"], s["m"], 0)
        for j, b in enumerate(s["src"]):
            a = B - s["padlen"] if s["short"] and b == s["k"] - 1 else B
            sn.append(b)
            bo.append(scur)
            av.append(a)
            src_parts.append((scur, blocks[b][:a]))
            scur += B + 5 + 2 * j  # odd and even starts; what lies between stays 0xFF
        for j, t in enumerate(s["tg"]):
            start = tcur + 64
            start += (1 + 32 * (len(tn) % 2) - start) % 64  # 1 or 33 modulo 64
            tn.append(t)
            to.append(start)
            want.append(blocks[t])
            tgt_ranges.append((start, B))
            tcur = start + B
    src = np.full(scur + 64, 0xFF, np.uint8)
    for o, b in src_parts:
        src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    tgt = np.full(tcur + 64, GUARD, np.uint8)
    return (descs, np.array(sn, np.int32), np.array(bo, np.uint64), np.array(av, np.uint64), np.array(tn, np.int32),
            np.array(to, np.uint64), src, tgt, want, tgt_ranges)


def _check(tgt_h, want, ranges, dig_h=None):
    mask = np.ones(tgt_h.size, bool)
    for j, ((o, B), w) in enumerate(zip(ranges, want)):
        assert tgt_h[o:o + B].tobytes() == w, f"target {j} differs from the oracle's block"
        mask[o:o + B] = False
        if dig_h is not None:
            assert dig_h[20 * j:20 * j + 20].tobytes() == hashlib.sha1(w).digest(), f"digest {j}"
    assert (tgt_h[mask] == GUARD).all(), "a byte outside the targets was written"


def run_device(engine, specs, digests=False, asynchronous=False, use_avail=True, repeat=1):
    descs, sn, bo, av, tn, to, src, tgt, want, ranges = _layout(specs)
    dsrc = torch.from_numpy(src).cuda()
    for _ in range(repeat):  # the second call reuses the cached plan
        dtgt = torch.from_numpy(tgt).cuda()
        ddig = torch.zeros(max(20 * len(tn), 1), dtype=torch.uint8, device="cuda") if digests else None
        engine.repair_batch(descs, sn, bo + np.uint64(dsrc.data_ptr()), 0, tn, to + np.uint64(dtgt.data_ptr()), 0,
                            block_avail=av if use_avail else None, digests=ddig, asynchronous=asynchronous)
        if asynchronous:
            engine.sync()
        _check(dtgt.cpu().numpy(), want, ranges, ddig.cpu().numpy() if digests else None)


# ---- device mode ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 4096 + 5, 33001])
def test_block_sizes(engine, B):
    """RS(4,6) from sources {5,0,3,2} in that order, targets [4,1]: the tail kernel only (B < 16),
    exactly one lane, one clamped lane, a ragged last tile, several tiles."""
    run_device(engine, [spec(4, 6, B, [5, 0, 3, 2], [4, 1])], digests=True, use_avail=False)


@pytest.mark.parametrize("B,padlen", [(4096 + 5, 1), (4096 + 5, 3), (20, 3), (33001, 1), (4096 + 5, 4096 + 5)],
                         ids=["pad1", "padk-1", "B20pad3", "B33001pad1", "avail0"])
def test_short_last_data_block(engine, B, padlen):
    """Source k-1 read in place with block_avail = B - padlen (0xFF behind it); the last case
    has avail = 0 (the whole chunk through the tail kernel).  Both targets are whole pieces."""
    run_device(engine, [spec(4, 6, B, [3, 0, 5, 2], [1, 4], padlen=padlen, short=True)], digests=True)


def test_repaired_last_data_block_keeps_its_zero_padding(engine):
    """Target k-1 itself: all B bytes are written, zfec's padding as computed zeros."""
    run_device(engine, [spec(4, 6, 4096 + 5, [0, 1, 2, 5], [3, 4], padlen=3)], digests=True)


def _lost(k, m, src):
    return [t for t in range(m) if t not in src]


_SRC96 = random.Random(6496).sample(range(96), 64)
ROW_GROUPS = {
    "10,14-1": spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 12, 8, 9], [7]),
    "10,14-3": spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 12, 8, 9], [10, 1, 7]),
    "10,14-4": spec(10, 14, 6554, [13, 0, 2, 3, 11, 5, 6, 12, 8, 9], [4, 10, 1, 7]),
    "16,24-8": spec(16, 24, 4096 + 9, [s for s in range(24) if s not in (1, 4, 9, 14, 16, 19, 21, 23)][::-1],
                    [19, 1, 23, 9, 16, 4, 21, 14]),
    "3,12-9": spec(3, 12, 5000 + 3, [10, 1, 6], [11, 0, 9, 2, 8, 3, 7, 4, 5]),
    # every lost piece, shuffled: 32 targets = four row groups over the wide-k loop
    "64,96-32": spec(64, 96, 2048 + 7, _SRC96, random.Random(1).sample(_lost(64, 96, _SRC96), 32), seed=6496),
    "1,3": spec(1, 3, 4096 + 1, [2], [1, 0]),
}


@pytest.mark.parametrize("name", list(ROW_GROUPS))
def test_row_groups(engine, name):
    run_device(engine, [ROW_GROUPS[name]], digests=True)


def _mixed():
    return [ROW_GROUPS["10,14-3"], spec(4, 6, 17, [5, 0, 3, 2], [4, 1]),
            spec(4, 6, 4096 + 5, [0, 1, 2, 3], []),  # nothing to repair
            ROW_GROUPS["3,12-9"], spec(4, 6, 7, [3, 0, 5, 2], [1, 4], padlen=2, short=True),
            ROW_GROUPS["64,96-32"], ROW_GROUPS["1,3"]]


@pytest.mark.parametrize("digests", [False, True], ids=["nodigests", "digests"])
def test_mixed_batch(engine, digests):
    """One call over four of the shapes above, a tail-only chunk and a chunk with ntargets = 0;
    twice, so the second call runs from the cached plan."""
    run_device(engine, _mixed(), digests=digests, repeat=2)


def test_async_then_sync(engine):
    run_device(engine, _mixed(), digests=True, asynchronous=True)


def test_timing_kind_repair(engine):
    engine.set_timing(True)
    try:
        engine.collect_timing("repair")
        run_device(engine, [ROW_GROUPS["10,14-4"]])
        ms, launches = engine.collect_timing("repair")
        assert launches == 1 and ms > 0
    finally:
        engine.set_timing(False)


def test_errors_before_any_device_work(engine):
    lib, ctx = engine.lib, engine._ctx
    d = np.zeros(1, dtype=REP_DTYPE)
    d[0] = (64, 0, 0, 2, 4, 6, 0)
    bo, to = np.zeros(4, np.uint64), np.zeros(2, np.uint64)  # never dereferenced: every call fails first

    def call(sn, tn, flags=0, desc=d):
        sn, tn = np.array(sn, np.int32), np.array(tn, np.int32)
        return lib.sec_repair_batch(ctx, desc.ctypes.data, 1, sn.ctypes.data, bo.ctypes.data, None, None,
                                    tn.ctypes.data, to.ctypes.data, None, None, flags)

    assert call([0, 2, 3, 4], [1, 5], flags=_lib.SEC_F_RECOVER) == _lib.SEC_EINVAL
    assert call([0, 2, 3, 4], [1, 5], flags=_lib.SEC_F_STAGED | _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert call([0, 2, 3, 4], [1, 5], flags=_lib.SEC_F_HOST | _lib.SEC_F_ASYNC) == _lib.SEC_EINVAL
    assert call([0, 2, 3, 6], [1, 5]) == _lib.SEC_ESHARENUM
    assert call([0, 2, 3, 4], [1, 6]) == _lib.SEC_ESHARENUM
    assert call([0, 2, 2, 4], [1, 5]) == _lib.SEC_EDUPSHARE
    assert call([0, 2, 3, 4], [1, 1]) == _lib.SEC_EDUPSHARE
    assert call([0, 2, 3, 4], [1, 3]) == _lib.SEC_EDUPSHARE
    bad = d.copy()
    bad["k"], bad["m"] = 5, 4
    assert call([0, 1, 2, 3, 4], [1, 5], desc=bad) == _lib.SEC_EKM
    bad = d.copy()
    bad["ntargets"] = -1
    assert call([0, 2, 3, 4], [1, 5], desc=bad) == _lib.SEC_EINVAL
    bad = d.copy()
    bad["B"] = 1 << 31
    assert call([0, 2, 3, 4], [1, 5], desc=bad) == _lib.SEC_ESIZE


# ---- host mode --------------------------------------------------------------------------
def _host_specs():
    return [ROW_GROUPS["10,14-3"], spec(4, 6, 17, [5, 0, 3, 2], [4, 1]), spec(4, 6, 4096 + 5, [0, 1, 2, 3], []),
            ROW_GROUPS["3,12-9"], spec(4, 6, 4096 + 5, [3, 0, 5, 2], [1, 4], padlen=3, short=True), ROW_GROUPS["1,3"]]


@pytest.mark.parametrize("digests", [False, True], ids=["nodigests", "digests"])
def test_host_numpy_buffers_are_staged(engine, digests):
    descs, sn, bo, av, tn, to, src, tgt, want, ranges = _layout(_host_specs())
    dig = np.zeros(20 * len(tn), np.uint8) if digests else None
    z0, r0, s0 = engine.host_paths()
    engine.repair_batch(descs, sn, bo, src, tn, to, tgt, block_avail=av, digests=dig, host=True)
    _check(tgt, want, ranges, dig)
    z1, r1, s1 = engine.host_paths()
    assert (z1, r1) == (z0, r0) and s1 == s0 + 1  # never zero-copy, never page-locked
    assert pinned_bytes()[0] == 0  # the slabs went back to the pool


@pytest.mark.parametrize("digests", [False, True], ids=["nodigests", "digests"])
def test_host_several_slabs(digests):
    """The staging pipeline over more slabs than it has slots: 64 KiB slabs, so every chunk of
    the mix but the small ones is a slab of its own (targets and digests scattered per slab)."""
    from storb_amd.engine import Engine

    eng = Engine(0, options={"SEC_SLAB_BYTES": 1 << 16, "SEC_SLAB_BYTES_DIGEST": 1 << 16})
    try:
        specs = _host_specs() + [ROW_GROUPS["16,24-8"], spec(4, 6, 33001, [5, 0, 3, 2], [4, 1])]
        descs, sn, bo, av, tn, to, src, tgt, want, ranges = _layout(specs)
        dig = np.zeros(20 * len(tn), np.uint8) if digests else None
        eng.repair_batch(descs, sn, bo, src, tn, to, tgt, block_avail=av, digests=dig, host=True)
        _check(tgt, want, ranges, dig)
        assert eng.host_paths() == (0, 0, 1)
        assert pinned_bytes()[0] == 0
    finally:
        eng.close()


def test_host_pinned_buffers_are_staged_too(engine):
    """Even buffers the encode / decode host paths would use in place are staged."""
    descs, sn, bo, av, tn, to, src, tgt, want, ranges = _layout(_host_specs()[:2])
    psrc, ptgt = engine.host_empty(src.size), engine.host_empty(tgt.size)
    psrc[:], ptgt[:] = src, tgt
    z0, r0, s0 = engine.host_paths()
    engine.repair_batch(descs, sn, bo, psrc, tn, to, ptgt, block_avail=av, host=True)
    _check(ptgt, want, ranges)
    assert engine.host_paths() == (z0, r0, s0 + 1)
    assert pinned_bytes()[0] == 0


def test_repair_host_from_bytes(engine):
    specs = _host_specs()
    items = []
    for s in specs:
        blocks = _blocks(s["k"], s["m"], s["B"], s["padlen"], s["seed"])
        items.append((s["k"], s["m"], [blocks[b] for b in s["src"]], s["src"], s["tg"]))
    out, digs = engine.repair_host(items, digests=True)
    for s, row, drow in zip(specs, out, digs):
        blocks = _blocks(s["k"], s["m"], s["B"], s["padlen"], s["seed"])
        assert all(type(b) is bytes for b in row)
        assert row == [blocks[t] for t in s["tg"]]
        assert drow == [hashlib.sha1(blocks[t]).digest() for t in s["tg"]]
    assert engine.repair_host(items) == out
    assert pinned_bytes()[0] == 0
    with pytest.raises(Error):
        engine.repair_host([(4, 6, [b"ab"] * 4, [0, 2, 3, 4], [3])])


def test_repair_host_targets_as_arrays(engine):
    """targets given as numpy arrays, whose truth value is not their length: a lone target 0, and
    two targets."""
    s = _host_specs()[0]
    k, m = s["k"], s["m"]
    blocks = _blocks(k, m, s["B"], s["padlen"], s["seed"])
    src = list(range(1, k + 1))  # block 0 lost
    held = [blocks[b] for b in src]
    out, digs = engine.repair_host([(k, m, held, src, np.array([0]))], digests=True)
    assert out == [[blocks[0]]] and digs == [[hashlib.sha1(blocks[0]).digest()]]
    two = np.array([0, m - 1]) if m - 1 > k else np.array([0])
    assert engine.repair_host([(k, m, held, src, two)]) == [[blocks[t] for t in two]]


def test_repair_pieces_end_to_end():
    """piece.repair_pieces on a 256 KiB chunk whose pieces come from the oracle: one data and
    one parity piece dropped, their bytes and ids regenerated on the GPU.  RS(4,2), the shape
    of the 256 KiB benchmark chunks (encode_chunk's own shape for this size, zfec(2,3), cannot
    lose two pieces)."""
    n = 256 << 10
    data = np.random.default_rng(256).integers(0, 256, n, dtype=np.uint8).tobytes()
    k, m = 4, 6
    B, padlen = -(-n // k), -(-n // k) * k - n
    blocks = cfec.easy_encode(data, k, m)
    lost = {k - 1, m - 1}
    pieces = [piece.Piece(chunk_idx=5, piece_idx=i, data=b,
                          piece_type=piece.PieceType.Data if i < k else piece.PieceType.Parity)
              for i, b in enumerate(blocks) if i not in lost]
    ec = piece.EncodedChunk(pieces=pieces, chunk_idx=5, k=k, m=m, chunk_size=B, padlen=padlen, original_chunk_size=n)
    got = piece.repair_pieces(ec, piece_ids=True)
    assert [p.piece_idx for p in got] == sorted(lost)
    for p in got:
        assert p.data == blocks[p.piece_idx]
        assert p.piece_id == hashlib.sha1(blocks[p.piece_idx]).hexdigest()
        assert p.chunk_idx == 5
        assert p.piece_type == (piece.PieceType.Data if p.piece_idx < k else piece.PieceType.Parity)
    plain = piece.repair_pieces(ec, targets=[m - 1])
    assert [(type(p), p.data) for p in plain] == [(piece.Piece, blocks[m - 1])]
