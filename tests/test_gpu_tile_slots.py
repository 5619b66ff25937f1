"""GPU: the tile maps' XCD-major placement (kernels.hpp tile_slot): workgroup b of a launch of nt
tiles reads entry tile_slot(b, nt) of the launch's own sub-array, where the planner put its tile.

The smallest shapes at which a misplaced entry shows, against the CPU oracle (oracle/fec_oracle.c)
byte for byte: tile counts of every residue modulo 8 on both sides of the 16-tile threshold below
which the map keeps its order, ragged chunks (the ragged end rides on the chunk's last tile), the
one-wave encode tiles, several launches in one plan (each sub-array is placed on its own) and the
bit-sliced kernels.  Every decode reads the surviving blocks in place from the encode's buffers and
must return the source; a recover-only decode returns the lost data blocks, zero padding included."""

import numpy as np
import pytest

from oracle import cfec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from storb_amd._lib import DEC_DTYPE, ENC_DTYPE  # noqa: E402

FILL = 0xEE


def _starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)


def roundtrip(engine, shapes, sizes, erased_of, seed, recover=True):
    """One encode_batch of chunks (k, m) = shapes[i] of sizes[i] bytes packed back to back, the parity
    against the oracle; then one decode_batch with the blocks erased_of(k, m) lost and the others read
    in place (block k-1, when held, short by padlen), the output against the source; then, with
    `recover`, the same as a recover-only decode against the oracle's blocks."""
    nch = len(sizes)
    sizes = np.asarray(sizes, dtype=np.uint64)
    ks = np.array([s[0] for s in shapes], dtype=np.uint64)
    ms = np.array([s[1] for s in shapes], dtype=np.uint64)
    Bs = (sizes + ks - 1) // ks
    in_off, par_off = _starts(sizes), _starts(Bs * (ms - ks))
    host = np.random.default_rng(seed).integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    ed = np.zeros(nch, dtype=ENC_DTYPE)
    ed["in_off"], ed["n"], ed["parity_off"], ed["parity_stride"], ed["k"], ed["m"] = in_off, sizes, par_off, Bs, ks, ms
    par = torch.full((int((Bs * (ms - ks)).sum()),), FILL, dtype=torch.uint8, device="cuda")
    engine.encode_batch(ed, src, par)
    par_h = par.cpu().numpy()
    blocks = []
    for i in range(nch):
        k, m, B, n = int(ks[i]), int(ms[i]), int(Bs[i]), int(sizes[i])
        blocks.append(cfec.easy_encode(host[int(in_off[i]):int(in_off[i]) + n].tobytes(), k, m))
        got = par_h[int(par_off[i]):int(par_off[i]) + (m - k) * B].tobytes()
        assert got == b"".join(blocks[i][k:]), f"parity of chunk {i}: zfec({k},{m}) n={n} B={B}"

    dd = np.zeros(nch, dtype=DEC_DTYPE)
    sn, offs, av, lost_blocks = [], [], [], []
    for i in range(nch):
        k, m, B, n = int(ks[i]), int(ms[i]), int(Bs[i]), int(sizes[i])
        erased = erased_of(k, m)
        keep = [s for s in range(m) if s not in erased][:k]
        assert len(keep) == k
        dd[i]["B"], dd[i]["padlen"], dd[i]["slot0"], dd[i]["k"], dd[i]["m"] = B, B * k - n, len(sn), k, m
        for s in keep:
            sn.append(s)
            offs.append(src.data_ptr() + int(in_off[i]) + s * B if s < k
                        else par.data_ptr() + int(par_off[i]) + (s - k) * B)
            av.append(n - (k - 1) * B if s == k - 1 else B)
        lost_blocks.append(b"".join(blocks[i][s] for s in range(k) if s not in keep))
    sn, offs, av = np.array(sn, np.int32), np.array(offs, np.uint64), np.array(av, np.uint64)

    dd["out_off"] = in_off
    out = torch.full_like(src, FILL)
    engine.decode_batch(dd, sn, offs, 0, out, block_avail=av)
    bad = torch.nonzero(out != src).view(-1)
    assert bad.numel() == 0, f"decode: {bad.numel()} bytes differ, the first at {int(bad[0])} " \
                             f"(chunk {int(np.searchsorted(in_off, int(bad[0]), 'right')) - 1})"
    if recover:
        want = b"".join(lost_blocks)
        dd["out_off"] = _starts([len(b) for b in lost_blocks])
        rec = torch.full((len(want),), FILL, dtype=torch.uint8, device="cuda")
        engine.decode_batch(dd, sn, offs, 0, rec, block_avail=av, recover_only=True)
        assert rec.cpu().numpy().tobytes() == want, "recover-only decode"
    assert torch.equal(src, torch.from_numpy(host).cuda()), "the source was written"


def erase(*lost):
    return lambda k, m: set(lost)


@pytest.mark.parametrize("ragged", [0, 3], ids=["n=4B", "n=4B-3"])
def test_rs42_every_tile_count_to_17(engine, ragged):
    """RS(4,2), one chunk per call, B = 4096 j: j 256-lane tiles, j = 1 .. 17 (every residue modulo
    8, and 16 and 17 where the placement starts); n = 4B - 3: the last tile's ragged end."""
    for j in range(1, 18):
        B = 4096 * j
        roundtrip(engine, [(4, 6)], [4 * B - ragged], erase(1, 3), seed=100 * ragged + j)


def test_rs42_one_wave_encode_tiles(engine):
    """Blocks of at least 64 KiB encode in 64-lane tiles: B = 65536 + 1024 j is 64 + j tiles."""
    for j in range(9):
        B = 65536 + 1024 * j
        roundtrip(engine, [(4, 6)], [4 * B - (j % 4)], erase(1, 3), seed=200 + j)


def test_rs83_mixed_sizes_one_plan(engine):
    """41 seeded chunks of 4 KiB to 300 KiB, RS(8,3): decode with {1,3,5} erased, block 7 read in place."""
    rng = np.random.default_rng(41)
    sizes = rng.integers(4 << 10, 300 << 10, 41).tolist()
    roundtrip(engine, [(8, 11)] * 41, sizes, erase(1, 3, 5), seed=41)


def test_mixed_shapes_several_launches(engine):
    """Shapes of other row counts and row groups in one call, so that one plan holds several launches,
    each more than 16 tiles with its own remainder modulo 8: an offset error between sub-arrays shows."""
    rng = np.random.default_rng(7)
    shapes = [(4, 6), (8, 11), (3, 12), (2, 3)] * 6
    sizes = rng.integers(20 << 10, 120 << 10, len(shapes)).tolist()
    roundtrip(engine, shapes, sizes, lambda k, m: {0, k - 1} if m - k > 1 else {k - 1}, seed=7)


@pytest.mark.parametrize("syn", [None, 1], ids=["default", "SEC_SYN=1"])
def test_bit_sliced_c4_kernel(engine, syn):
    """zfec(10,14), 19 chunks of 64 KiB (one tile each: 19 tiles); decode with {0,2,5,9} erased."""
    with engine.options(**({} if syn is None else {"SEC_SYN": syn})):
        roundtrip(engine, [(10, 14)] * 19, [65536] * 19, erase(0, 2, 5, 9), seed=1014)


def test_bit_sliced_zfec_16_24(engine):
    """zfec(16,24), 3 chunks of 256 KiB: 6 tiles, below the threshold."""
    roundtrip(engine, [(16, 24)] * 3, [(256 << 10) - 5] * 3, lambda k, m: {2, 15, 7}, seed=1624)
