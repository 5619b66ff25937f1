"""GPU: repair, check, decode + check and repair + check on ONE context.  The four share one plan
builder, launch unit and entry skeleton, and keep their plan, plan key, table cache and flag words
side by side in the context; this test is about that state staying apart.  One Engine runs the
sequence repair, check, decode + check, repair + check twice over the same buffers, in device mode
and with host=True, one byte of a check row flipped in place between the rounds, so that round two
reuses every cached plan on changed data.  Every call's outputs (targets, digests, decoded bytes,
results, row_bad, column) must equal, byte for byte, those of the same call made on a fresh Engine;
round one must be clean (targets and decoded bytes the oracle's), round two must name the flipped
row.

Shapes: B = 4096 + 3 (one full tile plus ragged bytes), one missing primary (block 1; the first
parity block stands in for it in the basis), one target (block 1), all chunks in one batch:
  k = 4,  m = 7:  n = k + 2 held, the small-batch tile kernels (k <= 4)
  k = 4,  m = 6:  n = k + 1 held (with m = 6, k + 2 held blocks would leave no block to repair)
  k = 10, m = 14: n = k + 2, the default batch
  k = 20, m = 24: n = k + 2, the wide kernels (k > 16)"""

import hashlib

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, DCHK_DTYPE, RCHK_DTYPE, REP_DTYPE  # noqa: E402
from storb_amd.engine import Engine  # noqa: E402

B = 4096 + 3
PADLEN = 5
SHAPES = [(4, 7, 6), (4, 6, 5), (10, 14, 12), (20, 24, 22)]  # (k, m, n held)
FLIPS = [4097, 17, 4095, 2048]  # per chunk: the byte of its LAST check row flipped before round two
OPS = ["repair", "check", "decode_check", "repair_check"]
FILL = 0xEE


def _case():
    """The batch: the blocks' image (entries at odd and even starts), the index arrays all four
    calls share (a repair reads a chunk's first k entries), and the oracle's data and targets."""
    sn, bo, parts, data, chunks = [], [], [], [], []
    cur = 3
    for i, (k, m, n) in enumerate(SHAPES):
        d = np.random.default_rng(100 + i).integers(0, 256, k * B - PADLEN, dtype=np.uint8).tobytes()
        blocks = cfec.easy_encode(d + b"\0" * PADLEN, k, m)
        entries = [0, k] + list(range(2, k)) + list(range(k + 1, k + 1 + n - k))
        assert len(entries) == n and 1 not in entries and max(entries) < m
        chunks.append((k, m, n, len(sn), blocks[1]))
        data.append(d)
        for j, e in enumerate(entries):
            sn.append(e)
            bo.append(cur)
            parts.append((cur, blocks[e]))
            cur += B + 5 + 2 * j
    img = np.full(cur + 64, 0xFF, np.uint8)
    for o, b in parts:
        img[o:o + B] = np.frombuffer(b, np.uint8)
    return img, np.array(sn, np.int32), np.array(bo, np.uint64), chunks, data


def _descs(chunks):
    nch = len(chunks)
    rep, chk = np.zeros(nch, REP_DTYPE), np.zeros(nch, CHK_DTYPE)
    dchk, rchk = np.zeros(nch, DCHK_DTYPE), np.zeros(nch, RCHK_DTYPE)
    for i, (k, m, n, slot0, _t) in enumerate(chunks):
        rep[i] = (B, slot0, i, 1, k, m, 0)
        chk[i] = (B, slot0, n, k, m, 0)
        dchk[i] = (i * 24 * B, B, PADLEN, slot0, n, k, m, 0)
        rchk[i] = (B, slot0, i, 1, n, k, m)
    return dict(repair=rep, check=chk, decode_check=dchk, repair_check=rchk)


def _run(eng, op, descs, src, sn, bo, host):
    """One call; its outputs as host bytes, by name."""
    nch, nslots = len(descs[op]), len(sn)

    def buf(nbytes):
        a = np.full(nbytes, FILL, np.uint8)
        return a if host else torch.from_numpy(a).to("cuda:0")

    tn = np.ones(nch, np.int32)  # block 1 of every chunk
    to = np.arange(nch, dtype=np.uint64) * (B + 9) + 7
    tgt, dig, dec = buf(nch * (B + 9) + 16), buf(20 * nch), buf(nch * 24 * B)
    res, rb, col = buf(nch * CHK_RESULT_DTYPE.itemsize), buf(nslots), buf(nslots)
    if op == "repair":
        eng.repair_batch(descs[op], sn, bo, src, tn, to, tgt, digests=dig, host=host)
        outs = dict(targets=tgt, digests=dig)
    elif op == "check":
        eng.check_batch(descs[op], sn, bo, src, res, row_bad=rb, column=col, host=host)
        outs = dict(results=res, row_bad=rb, column=col)
    elif op == "decode_check":
        eng.decode_check_batch(descs[op], sn, bo, src, dec, res, row_bad=rb, column=col, host=host)
        outs = dict(decoded=dec, results=res, row_bad=rb, column=col)
    else:
        eng.repair_check_batch(descs[op], sn, bo, src, tn, to, tgt, res, digests=dig, row_bad=rb, column=col, host=host)
        outs = dict(targets=tgt, digests=dig, results=res, row_bad=rb, column=col)
    return {name: (v if host else v.cpu().numpy()).tobytes() for name, v in outs.items()}


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_four_operations_share_one_context(host):
    img, sn, bo, chunks, data = _case()
    descs = _descs(chunks)
    src = img.copy() if host else torch.from_numpy(img).to("cuda:0")
    shared = Engine(0)
    try:
        for rnd in (1, 2):
            if rnd == 2:  # one byte of every chunk's last check row, in place
                for (k, m, n, slot0, _t), p in zip(chunks, FLIPS):
                    src[int(bo[slot0 + n - 1]) + p] ^= 0x5A
            for op in OPS:
                got = _run(shared, op, descs, src, sn, bo, host)
                fresh = Engine(0)
                try:
                    want = _run(fresh, op, descs, src, sn, bo, host)
                finally:
                    fresh.close()
                assert got.keys() == want.keys()
                for name in got:
                    assert got[name] == want[name], f"round {rnd} {op}: {name} differs from a fresh Engine's"
                # a flipped check row never reaches a stored row: the oracle's bytes in both rounds
                for i, (k, m, n, slot0, target) in enumerate(chunks):
                    if "targets" in got:
                        o = 7 + i * (B + 9)
                        assert got["targets"][o:o + B] == target, f"round {rnd} {op}: chunk {i} target"
                        assert got["digests"][20 * i:20 * i + 20] == hashlib.sha1(target).digest()
                    if "decoded" in got:
                        o = i * 24 * B
                        assert got["decoded"][o:o + len(data[i])] == data[i], f"round {rnd} {op}: chunk {i} data"
                if "results" not in got:
                    continue
                res = np.frombuffer(got["results"], CHK_RESULT_DTYPE)
                rb = np.frombuffer(got["row_bad"], np.uint8)
                for i, ((k, m, n, slot0, _t), p) in enumerate(zip(chunks, FLIPS)):
                    if rnd == 1:
                        assert int(res[i]["first"]) == CHK_CONSISTENT and int(res[i]["nbad"]) == 0, (op, i)
                        assert not rb[slot0:slot0 + n].any(), (op, i)
                    else:
                        assert int(res[i]["first"]) == p and int(res[i]["nbad"]) == 1, (op, i)
                        assert [j for j in range(n) if rb[slot0 + j]] == [n - 1], (op, i)
    finally:
        shared.close()
