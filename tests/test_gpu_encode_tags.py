"""GPU: the tagged encode (sec_encode_tag_batch, sec_encode_pieces_tags and the piece API above
them): parity, piece ids and APDP tags from one pass over each chunk.

Expected values never come from the library: parity from the cfec oracle (oracle/fec_oracle.c),
ids from hashlib.sha1, tags from oracle.apdp_ref.tag_value over the oracle's block bytes (the
last data block's padding zeros included).  The composition is asserted as well: the fused
call's outputs equal sec_encode_digest_batch + sec_apdp_tag_batch on the same buffers.

The shapes are the smallest at which the plan or the segmented reduce can go wrong: one 8 KiB
segment per piece, a second segment of one byte, three segments, a padded last data block whose
`avail` ends inside a segment, m == k (no parity, tags only), k == 1 (both pieces equal), the
bit-sliced encode route with unaligned blocks, and an empty chunk.

On "zfec(4,6) with n = 3 B + 1": a chunk's block size is B = ceil(n / k), so n = 3 B + 1 with
k = 4 holds only up to B = 4 (n = 13; the padding of any chunk is below k bytes).  That chunk is
here (its last block is one byte and three zeros), beside a zfec(4,6) chunk with the most padding
a large block can have (n = 4 B - 3, B = 8200)."""

import ctypes
import hashlib
import random

import numpy as np
import pytest

from oracle import apdp_ref, cfec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from storb_amd import _lib, apdp, bn, piece  # noqa: E402
from storb_amd._lib import ENC_DTYPE, MSG_DTYPE  # noqa: E402
from storb_amd.engine import Engine, device_count  # noqa: E402

PRF_KEY = b"prf-key-for-tests-0123456789abcdef0123456789="

# (k, m, n) by the issue's groups
SEGMENTS = [(2, 3, 2 * 8192), (2, 3, 2 * 8193), (2, 3, 2 * 16385)]
PADDING = [(3, 5, 3 * 8200 - 5), (4, 6, 13), (4, 6, 4 * 8200 - 3)]
EQUAL_AND_NO_PARITY = [(1, 2, 9001), (4, 4, 4 * 5001 - 1)]
BIT_SLICED = [(10, 14, 65536), (16, 24, 16 * 4099)]
EVERY = SEGMENTS + PADDING + EQUAL_AND_NO_PARITY + BIT_SLICED


@pytest.fixture(scope="module")
def key():
    n, e, d, p, q = apdp_ref.test_key(11)
    return {"n": n, "e": e, "d": d, "p": p, "q": q, "g": pow(31337, 2, n)}


def _modkey(key, engine, crt):
    mk = bn.ModKey(key["n"], engine)
    if crt:
        mk.set_crt(key["p"], key["q"])
    mk.set_tag(key["g"], apdp_ref.full_domain_hash(key["n"], apdp_ref.prf(PRF_KEY, 0)), key["d"])
    return mk


@pytest.fixture(scope="module", params=[True, False], ids=["crt", "nocrt"])
def mk(request, key, engine):
    return _modkey(key, engine, request.param)


@pytest.fixture(scope="module")
def mk_crt(key, engine):
    return _modkey(key, engine, True)


_chunk_memo, _tag_memo = {}, {}


def _chunk(k, m, n):
    """(data, the oracle's m blocks) of the test chunk of this shape: computed once, never changed."""
    if (k, m, n) not in _chunk_memo:
        data = random.Random(k * 1000003 + m * 1009 + n).randbytes(n)
        _chunk_memo[(k, m, n)] = (data, cfec.easy_encode(data, k, m) if n else [b""] * m)
    return _chunk_memo[(k, m, n)]


def _want_tag(key, block: bytes) -> int:
    if block not in _tag_memo:
        _tag_memo[block] = apdp_ref.tag_value(key["n"], key["g"], key["d"], PRF_KEY, block)
    return _tag_memo[block]


def _layout(shapes, stride_pad):
    """Descriptors of the chunks back to back, parity blocks parity_stride = B + stride_pad apart."""
    descs = np.zeros(len(shapes), dtype=ENC_DTYPE)
    ioff = poff = 0
    for i, (k, m, n) in enumerate(shapes):
        B = -(-n // k)
        descs[i] = (ioff, n, poff, max(B + stride_pad, 1), k, m)
        ioff += n
        poff += (m - k) * (B + stride_pad)
    return descs, ioff, poff


def _expect(key, shapes, descs, par, dig, tags, what):
    """Parity (and the guard bytes between blocks), ids and tags against the oracles."""
    slot = 0
    for (k, m, n), d in zip(shapes, descs):
        B = -(-n // k)
        _, blocks = _chunk(k, m, n)
        po, st = int(d["parity_off"]), int(d["parity_stride"])
        for r in range(m - k):
            assert par[po + r * st:po + r * st + B].tobytes() == blocks[k + r], (what, k, m, n, r)
            if B:
                assert (par[po + r * st + B:po + (r + 1) * st] == 0xA5).all(), (what, "guard", k, m, n, r)
        for j in range(m):
            if dig is not None:
                assert dig[20 * slot:20 * (slot + 1)].tobytes() == hashlib.sha1(blocks[j]).digest(), (what, k, m, n, j)
            got = int.from_bytes(tags[256 * slot:256 * (slot + 1)].tobytes(), "big")
            assert got == _want_tag(key, blocks[j]), (what, k, m, n, j)
            slot += 1


def _block_msgs(shapes, descs, src_addr, par_addr):
    """The chunks' m blocks as sec_apdp_tag_batch messages (the contract's len and avail)."""
    msgs = []
    for (k, m, n), d in zip(shapes, descs):
        B = -(-n // k)
        for j in range(k):
            msgs.append((src_addr + int(d["in_off"]) + j * B, B, max(0, min(B, n - j * B))))
        for r in range(m - k):
            msgs.append((par_addr + int(d["parity_off"]) + r * int(d["parity_stride"]), B, B))
    return np.array(msgs, dtype=MSG_DTYPE)


def _device(engine, mk, key, shapes, *, digests=True, stride_pad=0, asynchronous=False, compose=True):
    descs, nin, npar = _layout(shapes, stride_pad)
    nslots = sum(m for _, m, _ in shapes)
    host = np.frombuffer(b"".join(_chunk(*s)[0] for s in shapes), np.uint8)
    src = torch.from_numpy(host.copy()).cuda() if nin else torch.zeros(1, dtype=torch.uint8, device="cuda")
    par = torch.full((max(npar, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    dig = torch.zeros(20 * nslots, dtype=torch.uint8, device="cuda") if digests else None
    tags = torch.zeros(256 * nslots, dtype=torch.uint8, device="cuda")
    engine.encode_tag_batch(descs, src, par, tags, mk, digests=dig, asynchronous=asynchronous)
    if asynchronous:
        engine.sync()
    ph, th = par.cpu().numpy(), tags.cpu().numpy()
    dh = dig.cpu().numpy() if digests else None
    _expect(key, shapes, descs, ph, dh, th, "device")
    if compose:  # the calls it replaces, on the same input
        par2 = torch.full_like(par, 0xA5)
        dig2 = torch.zeros(20 * nslots, dtype=torch.uint8, device="cuda")
        tags2 = torch.zeros_like(tags)
        engine.encode_digest_batch(descs, src, par2, dig2)
        mk.tag_batch(_block_msgs(shapes, descs, src.data_ptr(), par2.data_ptr()), tags2)
        assert torch.equal(par, par2) and torch.equal(tags, tags2)
        if digests:
            assert torch.equal(dig, dig2)


def _host(engine, mk, key, shapes, *, digests=True, stride_pad=0, compose=True, what="host"):
    descs, nin, npar = _layout(shapes, stride_pad)
    nslots = sum(m for _, m, _ in shapes)
    src = np.frombuffer(b"".join(_chunk(*s)[0] for s in shapes), np.uint8).copy()
    if not nin:
        src = np.zeros(1, np.uint8)
    par = np.full(max(npar, 1), 0xA5, np.uint8)
    dig = np.zeros(20 * nslots, np.uint8) if digests else None
    tags = np.zeros(256 * nslots, np.uint8)
    staged = engine.host_paths()[2]
    engine.encode_tag_batch(descs, src, par, tags, mk, digests=dig, host=True)
    assert engine.host_paths()[2] == staged + 1  # always staged, as digest mode
    _expect(key, shapes, descs, par, dig, tags, what)
    if compose:
        par2, dig2, tags2 = np.full_like(par, 0xA5), np.zeros(20 * nslots, np.uint8), np.zeros_like(tags)
        engine.encode_digest_batch(descs, src, par2, dig2, host=True)
        mk.tag_batch(_block_msgs(shapes, descs, src.ctypes.data, par2.ctypes.data), tags2, host=True)
        assert (par == par2).all() and (tags == tags2).all()
        if digests:
            assert (dig == dig2).all()


@pytest.mark.parametrize("shapes", [SEGMENTS, PADDING, EQUAL_AND_NO_PARITY, BIT_SLICED],
                         ids=["segments", "padding", "k1_and_m_eq_k", "bit_sliced"])
def test_shapes_device_and_host(engine, mk, key, shapes):
    """Cases 1-4, each chunk alone and the group as one batch, device and host mode, with and
    without CRT."""
    for s in shapes:
        _device(engine, mk, key, [s])
    _device(engine, mk, key, shapes, compose=False)
    _host(engine, mk, key, shapes)


def test_equal_pieces_equal_tags(engine, mk_crt, key):
    """zfec(1,2): the parity piece is the data piece, so the two tags are one value."""
    _, blocks = _chunk(1, 2, 9001)
    assert blocks[0] == blocks[1]
    descs, _, npar = _layout([(1, 2, 9001)], 0)
    src = torch.from_numpy(np.frombuffer(blocks[0], np.uint8).copy()).cuda()
    par = torch.empty(npar, dtype=torch.uint8, device="cuda")
    tags = torch.zeros(512, dtype=torch.uint8, device="cuda")
    engine.encode_tag_batch(descs, src, par, tags, mk_crt)
    t = tags.cpu().numpy()
    assert t[:256].tobytes() == t[256:].tobytes() == _want_tag(key, blocks[0]).to_bytes(256, "big")


def test_heterogeneous_batch(engine, mk, key):
    """Case 5: every shape and an empty chunk in one batch; device mode with parity_stride > B and
    guard bytes between the parity blocks, then the same batch in host mode."""
    shapes = EVERY[:4] + [(2, 3, 0)] + EVERY[4:]
    _device(engine, mk, key, shapes, stride_pad=7)
    _host(engine, mk, key, shapes, stride_pad=7)


def test_empty_chunk_gets_the_empty_message_tag(engine, mk_crt, key):
    """n == 0: each of the m slots holds sec_apdp_tag_batch's tag of a message of length 0."""
    _device(engine, mk_crt, key, [(2, 3, 0)], compose=False)
    want = np.zeros(256, np.uint8)
    mk_crt.tag_batch(np.array([(0, 0, 0)], dtype=MSG_DTYPE), want, host=True)
    assert int.from_bytes(want.tobytes(), "big") == _want_tag(key, b"")


def test_small_slabs_pipeline_reuse(key):
    """Case 6: SEC_SLAB_BYTES_DIGEST = 65536 over 8 chunks of about 40 KiB: one sub-plan per chunk,
    so both pipeline slots' staging and partials are reused; twice on one context (plan reuse),
    then with one chunk's k changed (plan rebuild)."""
    eng = Engine(0, options={"SEC_SLAB_BYTES_DIGEST": 65536})
    try:
        mk = _modkey(key, eng, True)
        shapes = [(4, 6, 40000 + 13 * i) for i in range(6)] + [(2, 3, 2 * 16385 + 1), (3, 5, 40961)]
        _host(eng, mk, key, shapes, what="first")
        _host(eng, mk, key, shapes, compose=False, what="plan reused")
        shapes[2] = (5, 8, shapes[2][2])
        _host(eng, mk, key, shapes, compose=False, what="plan rebuilt")
        _host(eng, mk, key, shapes[:3], digests=False, compose=False, what="fewer chunks, no ids")
        mk.close()
    finally:
        eng.close()


def test_no_digests_and_async(engine, mk, key):
    """Case 7: digests = NULL, and SEC_F_ASYNC followed by sec_sync."""
    shapes = [SEGMENTS[1], PADDING[0], EQUAL_AND_NO_PARITY[1]]
    _device(engine, mk, key, shapes, digests=False)
    _device(engine, mk, key, shapes, asynchronous=True, compose=False)
    _device(engine, mk, key, shapes, digests=False, asynchronous=True, compose=False)
    _host(engine, mk, key, shapes, digests=False)


def test_errors(engine, mk_crt, key):
    """Case 8: SEC_EINVAL, then SEC_ENOTAG, then the chunks' own errors, before any device work."""
    lib, ctx = engine.lib, engine._ctx
    bare = bn.ModKey(key["n"], engine)  # no set_tag
    bad = np.zeros(1, dtype=ENC_DTYPE)
    bad[0] = (0, 100, 0, 100, 0, 3)  # k = 0: SEC_EKM
    one = ctypes.c_void_p(1)  # never dereferenced
    p = bad.ctypes.data
    assert lib.sec_encode_tag_batch(ctx, bare.handle, p, 1, one, one, one, one, 0) == _lib.SEC_ENOTAG
    assert lib.sec_encode_tag_batch(ctx, mk_crt.handle, p, 1, one, one, one, one, 0) == _lib.SEC_EKM
    hostasync = _lib.SEC_F_HOST | _lib.SEC_F_ASYNC
    assert lib.sec_encode_tag_batch(ctx, bare.handle, p, 1, one, one, one, one, hostasync) == _lib.SEC_EINVAL
    assert lib.sec_encode_tag_batch(ctx, mk_crt.handle, p, 1, one, one, one, one, hostasync) == _lib.SEC_EINVAL
    assert lib.sec_encode_tag_batch(ctx, mk_crt.handle, p, 1, one, one, one, one, _lib.SEC_F_STAGED) == _lib.SEC_EINVAL
    assert lib.sec_encode_tag_batch(ctx, None, p, 1, one, one, one, one, 0) == _lib.SEC_EINVAL
    assert lib.sec_encode_tag_batch(ctx, bare.handle, p, 1, one, one, one, None, 0) == _lib.SEC_EINVAL
    # sec_encode_pieces_tags: the same order; key and tags go together
    assert lib.sec_encode_pieces_tags(ctx, bare.handle, p, 1, None, one, None, one, _lib.SEC_F_HOST) == _lib.SEC_ENOTAG
    assert lib.sec_encode_pieces_tags(ctx, mk_crt.handle, p, 1, None, one, None, one, _lib.SEC_F_HOST) == _lib.SEC_EKM
    assert lib.sec_encode_pieces_tags(ctx, mk_crt.handle, p, 1, None, one, None, None, _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert lib.sec_encode_pieces_tags(ctx, None, p, 1, None, one, None, one, _lib.SEC_F_HOST) == _lib.SEC_EINVAL
    assert lib.sec_encode_pieces_tags(ctx, bare.handle, p, 1, None, one, None, one, 0) == _lib.SEC_EINVAL
    bare.close()


def test_key_of_another_device(engine, key):
    if device_count() < 2:
        pytest.skip("a key created on another device needs two devices")
    other = Engine(1)
    try:
        far = _modkey(key, other, False)
        bad = np.zeros(1, dtype=ENC_DTYPE)
        bad[0] = (0, 100, 0, 100, 0, 3)
        one = ctypes.c_void_p(1)
        assert engine.lib.sec_encode_tag_batch(engine._ctx, far.handle, bad.ctypes.data, 1, one, one, one, one,
                                               0) == _lib.SEC_EINVAL
        assert engine.lib.sec_encode_pieces_tags(engine._ctx, far.handle, bad.ctypes.data, 1, None, one, None, one,
                                                 _lib.SEC_F_HOST) == _lib.SEC_EINVAL
        far.close()
    finally:
        other.close()


PIECE_SHAPES = PADDING + EQUAL_AND_NO_PARITY + BIT_SLICED + [(4, 6, 1 << 20)]


def _odd_buffers(shapes):
    """One buffer per piece, each at an odd address."""
    rows, addrs = [], []
    for (k, m, n) in shapes:
        B = -(-n // k)
        row = [np.empty(B + 1, np.uint8)[1:] for _ in range(m)]
        assert all(r.ctypes.data & 1 for r in row)
        rows.append(row)
        addrs += [r.ctypes.data for r in row]
    return rows, addrs


@pytest.mark.parametrize("gpu_parity_ids", [False, True], ids=["host_ids", "gpu_parity_ids"])
def test_pieces_tags(engine, mk, key, gpu_parity_ids):
    """Case 9: sec_encode_pieces_tags into separate odd-aligned buffers, with ids and tags."""
    shapes = PIECE_SHAPES
    rows, addrs = _odd_buffers(shapes)
    dig = np.zeros(20 * len(addrs), np.uint8)
    tags = np.zeros(256 * len(addrs), np.uint8)
    engine.encode_pieces_into([_chunk(*s)[0] for s in shapes], [(k, m) for k, m, _ in shapes], addrs, dig,
                              gpu_parity_ids=gpu_parity_ids, tags=tags, tag_key=mk)
    slot = 0
    for s, row in zip(shapes, rows):
        blocks = _chunk(*s)[1]
        assert [r.tobytes() for r in row] == blocks, s
        for b in blocks:
            assert dig[20 * slot:20 * (slot + 1)].tobytes() == hashlib.sha1(b).digest(), (s, slot)
            assert int.from_bytes(tags[256 * slot:256 * (slot + 1)].tobytes(), "big") == _want_tag(key, b), (s, slot)
            slot += 1


def test_pieces_tags_sub_batches_and_no_ids(key):
    """The sub-batches of sec_encode_pieces_tags are bounded by their staged bytes too (twice
    SEC_SLAB_BYTES): with 65536 no two chunks here share one, and the m == k ones, which have no
    parity, take their GPU call all the same."""
    eng = Engine(0, options={"SEC_SLAB_BYTES": 65536, "SEC_SLAB_BYTES_DIGEST": 65536})
    try:
        mk = _modkey(key, eng, True)
        shapes = [(4, 4, 4 * 20001 - 1), (4, 6, 80013), (4, 4, 4 * 20001 - 1), (10, 14, 2 * 65536), (3, 5, 9 * 8200 - 5)]
        rows, addrs = _odd_buffers(shapes)
        tags = np.zeros(256 * len(addrs), np.uint8)
        eng.encode_pieces_into([_chunk(*s)[0] for s in shapes], [(k, m) for k, m, _ in shapes], addrs, None,
                               tags=tags, tag_key=mk)
        slot = 0
        for s, row in zip(shapes, rows):
            blocks = _chunk(*s)[1]
            assert [r.tobytes() for r in row] == blocks, s
            for b in blocks:
                assert int.from_bytes(tags[256 * slot:256 * (slot + 1)].tobytes(), "big") == _want_tag(key, b), (s, slot)
                slot += 1
        mk.close()
    finally:
        eng.close()


def test_pieces_tags_without_key_is_encode_pieces(engine):
    """No key and no tags: sec_encode_pieces byte for byte (pieces and ids)."""
    shapes = PIECE_SHAPES
    descs = np.zeros(len(shapes), dtype=ENC_DTYPE)
    keep = []
    for i, (k, m, n) in enumerate(shapes):
        c = np.frombuffer(_chunk(k, m, n)[0], np.uint8)
        keep.append(c)
        descs[i] = (c.ctypes.data, n, 0, -(-n // k), k, m)
    out = []
    for fn, extra in ((engine.lib.sec_encode_pieces, False), (engine.lib.sec_encode_pieces_tags, True)):
        for flags in (_lib.SEC_F_HOST, _lib.SEC_F_HOST | _lib.SEC_F_GPU_PARITY_IDS):
            rows, addrs = _odd_buffers(shapes)
            pa = np.array(addrs, dtype=np.uint64)
            dig = np.zeros(20 * len(addrs), np.uint8)
            if extra:
                rc = fn(engine._ctx, None, descs.ctypes.data, len(shapes), None, pa.ctypes.data, dig.ctypes.data, None,
                        flags)
            else:
                rc = fn(engine._ctx, descs.ctypes.data, len(shapes), None, pa.ctypes.data, dig.ctypes.data, flags)
            assert rc == 0
            out.append((b"".join(r.tobytes() for row in rows for r in row), dig.tobytes()))
    assert out[0] == out[1] == out[2] == out[3]
    assert out[0][0] == b"".join(b for s in shapes for b in _chunk(*s)[1])


def _system(key):
    cs = apdp.ChallengeSystem()
    cs.key.rsa = apdp.RSAPrivateKey(key["p"], key["q"], key["e"])
    cs.key.g = key["g"]
    cs.key.prf_key = PRF_KEY
    return cs


def test_piece_api_against_generate_tags(key):
    """Case 10: piece.encode_chunks_with_tags and the stream form against
    ChallengeSystem.generate_tags, and verify_proofs accepting a proof made for a returned tag."""
    cs = _system(key)
    with pytest.raises(apdp.APDPError):
        piece.encode_chunks_with_tags([b"abc"], apdp.ChallengeSystem())  # generate_tags' uninitialised-key error
    rng = random.Random(10)
    chunks = [rng.randbytes(n) for n in (1000, 40_001, 200_001, (1 << 20) + 3)]
    out, ids, tags = piece.encode_chunks_with_tags(chunks, cs, 3)
    out2, ids2 = piece.encode_chunks_with_ids(chunks, 3)
    assert ids == ids2 and [ec.model_dump() for ec in out] == [ec.model_dump() for ec in out2]
    flat = [p.data for ec in out for p in ec.pieces]
    want = cs.generate_tags(flat)
    assert [t for ts in tags for t in ts] == want
    assert want[0].tag_value == _want_tag(key, flat[0])  # generate_tags itself against the oracle, once
    assert cs.tag_key() is cs.tag_key() and cs.tag_key().has_tag
    streamed = list(piece.encode_chunks_stream(iter(chunks), 3, piece_ids=True, window_bytes=300_000, tags=cs))
    assert [s[1] for s in streamed] == ids
    assert [s[2] for s in streamed] == tags
    assert [s[0].model_dump() for s in streamed] == [ec.model_dump() for ec in out]
    _, none, tags3 = piece.encode_chunks_with_tags(chunks[:2], cs, piece_ids=False)
    assert none is None and tags3 == tags[:2]
    # a returned tag proves possession of its piece
    data, tag = out[2].pieces[1].data, tags[2][1]
    ch = cs.issue_challenges([tag])[0]
    pr = cs.generate_proofs([(data, tag, ch)], key["n"])[0]
    assert cs.verify_proofs([(pr, ch, tag)], key["n"], key["e"]) == [True]
    assert cs.verify_proofs([(pr.model_copy(update={"tag_value": pr.tag_value + 1}), ch, tag)], key["n"],
                            key["e"]) == [False]


def test_engine_host_forms(engine, mk_crt, key):
    """Engine.encode_host / encode_host_raw with tag_key=: the tags as Python ints per chunk."""
    shapes = [PADDING[0], EQUAL_AND_NO_PARITY[1], SEGMENTS[1]]
    chunks = [_chunk(*s)[0] for s in shapes]
    km = [(k, m) for k, m, _ in shapes]
    par, digs, tags = engine.encode_host(chunks, km, digests=True, tag_key=mk_crt)
    par2, tags2 = engine.encode_host(chunks, km, tag_key=mk_crt)
    buf, layout, dig, tags3 = engine.encode_host_raw(chunks, km, digests=True, tag_key=mk_crt)
    assert tags == tags2 == tags3 and par == par2
    for s, p, dg, tg, (o, B, np_) in zip(shapes, par, digs, tags, layout):
        blocks = _chunk(*s)[1]
        assert p == blocks[s[0]:]
        assert buf[o:o + np_ * B].tobytes() == b"".join(blocks[s[0]:])
        assert dg == [hashlib.sha1(b).digest() for b in blocks]
        assert tg == [_want_tag(key, b) for b in blocks]


def test_bignum_calls_keep_their_values(engine, mk_crt, key):
    """Case 11: sec_apdp_tag_batch and sec_bn_reduce_batch over a device buffer still give the
    oracle's values (their launchers gained the second base pointer)."""
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, 40000, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    spans = [(3, 8192, 8192), (1, 8193, 8193), (17, 20001, 12345), (0, 0, 0), (5, 300, 7)]
    msgs = np.array([(buf.data_ptr() + o, ln, av) for o, ln, av in spans], dtype=MSG_DTYPE)
    datas = [host[o:o + av].tobytes() + b"\0" * (ln - av) for o, ln, av in spans]
    out = torch.zeros(256 * len(spans), dtype=torch.uint8, device="cuda")
    mk_crt.reduce_batch(msgs, out)
    assert bn.from_be(out.cpu().numpy()) == [int.from_bytes(d, "big") % key["n"] for d in datas]
    mk_crt.tag_batch(msgs, out)
    assert bn.from_be(out.cpu().numpy()) == [_want_tag(key, d) for d in datas]
    # ... and the fused call reads the same bytes through both bases: the buffer as one zfec(2,3)
    # chunk, its data blocks' tags against sec_apdp_tag_batch over the same spans
    descs = np.zeros(1, dtype=ENC_DTYPE)
    descs[0] = (0, 40000, 0, 20000, 2, 3)
    par = torch.empty(20000, dtype=torch.uint8, device="cuda")
    fused = torch.zeros(256 * 3, dtype=torch.uint8, device="cuda")
    engine.encode_tag_batch(descs, buf, par, fused, mk_crt)
    blocks = np.array([(buf.data_ptr(), 20000, 20000), (buf.data_ptr() + 20000, 20000, 20000),
                       (par.data_ptr(), 20000, 20000)], dtype=MSG_DTYPE)
    mk_crt.tag_batch(blocks, out)
    assert torch.equal(fused, out[:256 * 3])
