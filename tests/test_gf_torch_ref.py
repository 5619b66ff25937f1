"""CPU: tests/gf_torch_ref.py (the torch reference the large-block GPU tests use) against the C oracle
(oracle/fec_oracle.c via cfec), byte for byte, on torch CPU tensors.  This is the only link between
the two references: the GPU tests of 3-4 MiB blocks take every expected byte from gf_torch_ref.

Encode: zfec(4,6), (10,14), (32,48), (64,96) at B = 16, 17, 2049, 4099 with padlen 0 and k-1.  zfec
splits a chunk into equal blocks and refuses a chunk whose padding does not fit in block k-1
(padlen > B: "Input blocks are required to be all the same length"), so padlen = k-1 does not exist
for (32,48) and (64,96) at B = 16 and 17: there both references must refuse the chunk, and the
largest padding that does exist (B) is compared instead.
Decode: rows(decode_matrix(k, m, idx), kept) of zfec(64,96) with 24 random and all 32 lost blocks."""

import random

import numpy as np
import pytest

from oracle import cfec, zfec_ref

torch = pytest.importorskip("torch")

from tests import gf_torch_ref  # noqa: E402

SHAPES = [(4, 6), (10, 14), (32, 48), (64, 96)]
SIZES = [16, 17, 2049, 4099]


def _chunk(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _same(got: torch.Tensor, blocks):
    want = np.frombuffer(b"".join(blocks), np.uint8).reshape(len(blocks), -1)
    assert tuple(got.shape) == want.shape
    d = np.argwhere(got.numpy() != want)
    assert d.size == 0, f"first difference at (row, position) {d[0].tolist()} of {len(d)}"


@pytest.mark.parametrize("pad", ["0", "k-1"])
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("k,m", SHAPES)
def test_encode_equals_oracle(k, m, B, pad):
    padlen = 0 if pad == "0" else k - 1
    if padlen > B:  # no such chunk in zfec: both refuse it; then the largest padding there is
        n = k * B - padlen
        with pytest.raises(ValueError):
            cfec.easy_encode(bytes(n), k, m)
        with pytest.raises(ValueError):
            gf_torch_ref.encode(torch.zeros(n, dtype=torch.uint8), k, m)
        padlen = B
    n = k * B - padlen
    data = _chunk(n, 1000 * k + B + padlen)
    want = cfec.easy_encode(data.tobytes(), k, m)
    assert len(want) == m and len(want[0]) == B
    got = gf_torch_ref.encode(torch.from_numpy(data), k, m)
    _same(got, want)


def test_rows_is_the_table_gather():
    """rows against its definition, element by element, on a small random product; zero coefficients
    and zero bytes included."""
    rng = np.random.default_rng(5)
    coef = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    coef[1, 2] = coef[4, 0] = 0
    blocks = rng.integers(0, 256, (7, 33), dtype=np.uint8)
    blocks[3, :5] = 0
    got = gf_torch_ref.rows(coef, torch.from_numpy(blocks)).numpy()
    for i in range(5):
        for t in range(33):
            v = 0
            for j in range(7):
                v ^= int(zfec_ref.MUL[coef[i, j]][blocks[j, t]])
            assert got[i, t] == v, (i, t)


@pytest.mark.parametrize("pattern", ["24 random", "32 all parity"])
@pytest.mark.parametrize("B", [17, 2049])
def test_decode_equals_oracle(pattern, B):
    k, m, padlen = 64, 96, 11
    n = k * B - padlen
    data = _chunk(n, B)
    blocks = cfec.easy_encode(data.tobytes(), k, m)
    rng = random.Random(B)
    if pattern == "24 random":
        lost = rng.sample(range(k), 24)
        keep = [j for j in range(k) if j not in lost] + rng.sample(range(k, m), 24)
    else:
        lost = rng.sample(range(k), 32)
        keep = [j for j in range(k) if j not in lost] + list(range(k, m))
    rng.shuffle(keep)
    want = cfec.easy_decode([blocks[s] for s in keep], keep, padlen, k, m)
    assert want == data.tobytes()
    slots, idx = zfec_ref.normalise([blocks[s] for s in keep], keep, k, m)
    kept = torch.from_numpy(np.frombuffer(b"".join(slots), np.uint8).reshape(k, B).copy())
    got = gf_torch_ref.rows(zfec_ref.decode_matrix(k, m, idx), kept)
    assert got.numpy().tobytes()[:n] == want
    # and from the reference's own blocks, as the GPU tests use it
    mine = gf_torch_ref.encode(torch.from_numpy(data), k, m)
    _same(mine, blocks)
    got = gf_torch_ref.rows(zfec_ref.decode_matrix(k, m, idx), mine[torch.tensor(idx)])
    assert got.numpy().tobytes()[:n] == want
