"""GPU: one batch whose coefficient tables outgrow the table cache's first buffer (api.cpp
resolve_tables: the cache is reset once, to a buffer sized by every table of the batch).

A fresh context's cache starts empty and grows to at least 1 MiB (encode) or about 2.2 MiB (decode,
repair) at its first reset, so a first call that needs more than that in distinct tables must
still succeed.  Expected bytes come from the oracle (oracle/fec_oracle.c) only.  Every test makes
its own Engine: the session's shared one has a grown cache."""

import functools

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd._lib import DEC_DTYPE, ENC_DTYPE, REP_DTYPE  # noqa: E402
from storb_amd.engine import Engine  # noqa: E402

K, M, B, PADLEN, NCH = 64, 96, 80, 3, 96
N = K * B - PADLEN
GUARD, POISON = 0xA5, 0xFF


def survivors(i):
    """Chunk i keeps shares i .. i + 63 (mod 96), in that order: 96 distinct patterns."""
    return [(i + j) % M for j in range(K)]


@functools.lru_cache(maxsize=None)
def chunks():
    """Per chunk: its N data bytes and the oracle's 96 blocks of B bytes (block 63 ends in PADLEN
    zeros).  Computed once, shared by the repair and the decode test, never modified."""
    rng = np.random.default_rng(6496)
    out = []
    for _ in range(NCH):
        data = rng.integers(0, 256, N, dtype=np.uint8).tobytes()
        blocks = cfec.easy_encode(data, K, M)
        assert len(blocks) == M and all(len(b) == B for b in blocks)
        out.append((data, blocks))
    return out


def block_image():
    """Every block of every chunk, block b of chunk i at (i * M + b) * B."""
    return np.frombuffer(b"".join(b"".join(blocks) for _, blocks in chunks()), np.uint8).copy()


def test_repair_batch_larger_than_the_cache_floor():
    """96 zfec(64,96) repairs of 32 targets each: 96 tables of 64 * 32 coefficients, 3.75 MiB.
    Block 63, where it survives, is handed over B - PADLEN bytes long with 0xFF behind, so tiles
    ([0, 77), clamped lanes) and the ragged end ([77, 80)) both run; where it is lost it is
    repaired whole, padding included.  Targets lie one guard byte apart, at every alignment.
    Then the same call again (plan reuse) and an RS(4,6) repair (the cache after its reset)."""
    eng = Engine(0)
    img = block_image()
    descs = np.zeros(NCH, dtype=REP_DTYPE)
    sn, bo, av, tn, to, want = [], [], [], [], [], []
    for i, (_, blocks) in enumerate(chunks()):
        src = survivors(i)
        tg = [t for t in range(M) if t not in src]
        assert len(tg) == M - K
        descs[i] = (B, len(sn), len(tn), len(tg), K, M, 0)
        for s in src:
            sn.append(s)
            bo.append((i * M + s) * B)
            av.append(B - PADLEN if s == K - 1 else B)
            if s == K - 1:
                img[bo[-1] + B - PADLEN:bo[-1] + B] = POISON
        for t in tg:
            to.append(1 + len(tn) * (B + 1))
            tn.append(t)
            want.append(blocks[t])
    dsrc = torch.from_numpy(img).cuda()
    tgt = np.full(1 + len(tn) * (B + 1) + 64, GUARD, np.uint8)
    dtgt = torch.empty(tgt.size, dtype=torch.uint8, device="cuda")
    args = (descs, np.array(sn, np.int32), np.array(bo, np.uint64) + np.uint64(dsrc.data_ptr()), 0,
            np.array(tn, np.int32), np.array(to, np.uint64) + np.uint64(dtgt.data_ptr()), 0)
    # the second call is the first one again, target addresses included (the plan key covers
    # them), so it reuses the plan that was stamped after the cache's reset
    for call in range(2):
        dtgt.copy_(torch.from_numpy(tgt))
        eng.repair_batch(*args, block_avail=np.array(av, np.uint64))
        got = dtgt.cpu().numpy()
        mask = np.ones(got.size, bool)
        for j, (o, w) in enumerate(zip(to, want)):
            assert got[o:o + B].tobytes() == w, f"call {call}: target {j} (chunk {j // 32}, block {tn[j]})"
            mask[o:o + B] = False
        assert (got[mask] == GUARD).all(), "a byte outside the targets was written"

    # a small repair on the same context, its table placed in the cache that was just reset
    k, m, b2 = 4, 6, 4096 + 5
    data = np.random.default_rng(46).integers(0, 256, k * b2, dtype=np.uint8).tobytes()
    blocks = cfec.easy_encode(data, k, m)
    src, tg = [5, 0, 3, 2], [4, 1]
    d2 = np.zeros(1, dtype=REP_DTYPE)
    d2[0] = (b2, 0, 0, len(tg), k, m, 0)
    dsrc2 = torch.from_numpy(np.frombuffer(b"".join(blocks), np.uint8).copy()).cuda()
    dtgt2 = torch.full((2 * b2,), GUARD, dtype=torch.uint8, device="cuda")
    eng.repair_batch(d2, np.array(src, np.int32), np.array(src, np.uint64) * np.uint64(b2), dsrc2,
                     np.array(tg, np.int32), np.array([0, b2], np.uint64), dtgt2)
    got = dtgt2.cpu().numpy()
    for j, t in enumerate(tg):
        assert got[j * b2:(j + 1) * b2].tobytes() == blocks[t], f"RS(4,6) target {t}"
    eng.close()


def test_direct_decode_batch_larger_than_the_cache_floor():
    """The same 96 patterns decoded.  One present data block other than block 63 of each chunk
    has block_avail = B - 1 (0xFF in that byte's place), so no chunk can take the syndrome path
    and each chunk with a lost primary needs its own table of 64 * e coefficients (e = 1 .. 32,
    2.5 MiB in all).  Expected: the oracle's decode with the missing byte zero."""
    eng = Engine(0)
    img = block_image()
    descs = np.zeros(NCH, dtype=DEC_DTYPE)
    sn, bo, av, want = [], [], [], []
    for i, (_, blocks) in enumerate(chunks()):
        src = survivors(i)
        short = i if i < K - 1 else 0  # a surviving data block that is not the last one
        assert short in src and short < K - 1
        descs[i] = (i * N, B, PADLEN, len(sn), K, M)
        for s in src:
            sn.append(s)
            bo.append((i * M + s) * B)
            av.append(B - 1 if s == short else B)
        img[(i * M + short) * B + B - 1] = POISON
        given = [blocks[s][:B - 1] + b"\0" if s == short else blocks[s] for s in src]
        want.append(cfec.easy_decode(given, src, PADLEN, K, M))
        assert len(want[-1]) == N
    dsrc = torch.from_numpy(img).cuda()
    out = torch.full((NCH * N + 64,), GUARD, dtype=torch.uint8, device="cuda")
    eng.decode_batch(descs, np.array(sn, np.int32), np.array(bo, np.uint64), dsrc, out,
                     block_avail=np.array(av, np.uint64))
    syndrome, direct = eng.decode_paths()
    assert (syndrome, direct) == (0, NCH - 1)  # chunk 0 keeps every primary: copies only
    got = out.cpu().numpy()
    for i in range(NCH):
        assert got[i * N:(i + 1) * N].tobytes() == want[i], f"chunk {i}"
    assert (got[NCH * N:] == GUARD).all()
    eng.close()


def test_encode_batch_larger_than_the_cache_floor():
    """One batch of 40 shapes (k, k + 32), k = 60 .. 99: 2 MiB of tables over the encode cache's
    1 MiB floor.  n = 33 * k - 3, so B = 33 and the last data block holds 30 bytes: one clamped
    tile and a ragged end of 3 bytes per chunk."""
    eng = Engine(0)
    ks = list(range(60, 100))
    rng = np.random.default_rng(6099)
    descs = np.zeros(len(ks), dtype=ENC_DTYPE)
    datas, in_off, par_off = [], 0, 0
    for i, k in enumerate(ks):
        n = 33 * k - 3
        descs[i] = (in_off, n, par_off, 33, k, k + 32)
        datas.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        in_off += n
        par_off += 32 * 33
    src = torch.from_numpy(np.frombuffer(b"".join(datas), np.uint8).copy()).cuda()
    par = torch.full((par_off + 64,), GUARD, dtype=torch.uint8, device="cuda")
    eng.encode_batch(descs, src, par)
    got = par.cpu().numpy()
    for i, k in enumerate(ks):
        want = b"".join(cfec.easy_encode(datas[i], k, k + 32)[k:])
        assert got[i * 32 * 33:(i + 1) * 32 * 33].tobytes() == want, f"parity of ({k},{k + 32})"
    assert (got[par_off:] == GUARD).all()
    eng.close()
