#!/usr/bin/env python3
"""The bit-sliced check kernel (sec_check_bs_kernel) against the direct (v_perm) check kernels, on
the same device-resident buffers in one process: every piece of every chunk held (n = m), the data
pieces the basis (choose_blocks' pick when all are held), block k-1 read in place with its avail.

  check          sec_check_batch: reads n * B per chunk, writes nothing but the results
  decode_check   sec_decode_check_batch, nothing lost: the same, plus the chunk's k * B - padlen
                 bytes copied to `out`

each with SEC_CHECK_BS = 0 (direct) and = 1 (bit-sliced), on two contexts of the same process so
neither re-plans when the other runs.  Kernel times are the library's per-launch HIP events
(sec_ctx_set_timing).  Every schedule is warmed up, then `--reps` steps per round, `--rounds`
rounds interleaved over the four schedules, median of the rounds.  Bytes are the algorithm's, from
the shapes.  Before anything is timed both paths must report a clean batch clean, find one flipped
parity byte, and reproduce the data.

    python tools/bench_check_bs.py [--rounds 5] [--reps 10] [--only NAMES] [--extra]
                                   [--out profiles/check_bs_rate.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0  # MI355X HBM3E

MIXED = [(64 << 10) + 13, (256 << 10) + 5, 1 << 20, (4 << 20) + 7]
CASES = [
    dict(name="c4_rs10_4", sizes=[64 << 10] * 8192, k=10, m=14),
    dict(name="zfec16_24_8MiB", sizes=[8 << 20] * 128, k=16, m=24),
    dict(name="zfec32_48_1MiB", sizes=[1 << 20] * 1024, k=32, m=48),
    dict(name="zfec32_48_64MiB", sizes=[64 << 20] * 16, k=32, m=48),
    dict(name="zfec64_96_1MiB", sizes=[1 << 20] * 1024, k=64, m=96),
    dict(name="zfec64_96_256MiB", sizes=[256 << 20] * 4, k=64, m=96),
    dict(name="c5_rs8_3_mixed", sizes=[MIXED[i % 4] for i in range(512)], k=8, m=11),
]
# --extra: other block sizes of the shapes above and the shape they leave out, to see whether the
# default rule needs a block-size term
EXTRA = [
    dict(name="rs10_4_1MiB", sizes=[1 << 20] * 1024, k=10, m=14),
    dict(name="rs10_4_8MiB", sizes=[8 << 20] * 128, k=10, m=14),
    dict(name="zfec16_24_64KiB", sizes=[64 << 10] * 8192, k=16, m=24),
    dict(name="zfec16_24_1MiB", sizes=[1 << 20] * 1024, k=16, m=24),
    dict(name="zfec8_12_64KiB", sizes=[64 << 10] * 8192, k=8, m=12),
    dict(name="zfec8_12_4MiB", sizes=[4 << 20] * 256, k=8, m=12),
    dict(name="zfec32_48_128KiB", sizes=[128 << 10] * 8192, k=32, m=48),
    dict(name="zfec64_96_256KiB", sizes=[256 << 10] * 4096, k=64, m=96),
]


def run_case(engs, torch, c, rounds, reps):
    from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, DCHK_DTYPE, ENC_DTYPE

    sizes, k, m = np.array(c["sizes"], np.uint64), c["k"], c["m"]
    nch, p = len(sizes), m - k
    Bs = (sizes + np.uint64(k - 1)) // np.uint64(k)
    pad = Bs * np.uint64(k) - sizes
    in_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    par_off = np.concatenate([[0], np.cumsum(Bs * np.uint64(p))[:-1]]).astype(np.uint64)
    total, ptotal = int(sizes.sum()), int((Bs * np.uint64(p)).sum())
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2024)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda:0", generator=g)
    par = torch.empty(ptotal, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    ed = np.zeros(nch, dtype=ENC_DTYPE)
    ed["in_off"], ed["n"], ed["parity_off"], ed["parity_stride"], ed["k"], ed["m"] = in_off, sizes, par_off, Bs, k, m
    engs[0].encode_batch(ed, src, par)

    s = np.arange(m, dtype=np.uint64)[None, :]
    data_addr = np.uint64(src.data_ptr()) + in_off[:, None] + s * Bs[:, None]
    par_addr = np.uint64(par.data_ptr()) + par_off[:, None] + (s - np.uint64(k)) * Bs[:, None]
    bo = np.where(s < k, data_addr, par_addr).astype(np.uint64).ravel()
    av = np.where(s == k - 1, (Bs - pad)[:, None], Bs[:, None]).astype(np.uint64).ravel()
    sn = np.tile(np.arange(m, dtype=np.int32), nch)
    cd = np.zeros(nch, dtype=CHK_DTYPE)
    cd["B"], cd["n"], cd["k"], cd["m"] = Bs, m, k, m
    cd["slot0"] = np.arange(nch, dtype=np.uint64) * m
    dd = np.zeros(nch, dtype=DCHK_DTYPE)
    dd["out_off"], dd["B"], dd["padlen"], dd["n"], dd["k"], dd["m"] = in_off, Bs, pad, m, k, m
    dd["slot0"] = cd["slot0"]
    res = torch.zeros(16 * nch, dtype=torch.uint8, device="cuda:0")
    rb = torch.zeros(nch * m, dtype=torch.uint8, device="cuda:0")
    col = torch.zeros(nch * m, dtype=torch.uint8, device="cuda:0")

    def check(eng):
        eng.check_batch(cd, sn, bo, 0, res, block_avail=av, row_bad=rb, column=col, asynchronous=True)

    def decode_check(eng):
        eng.decode_check_batch(dd, sn, bo, 0, out, res, block_avail=av, row_bad=rb, column=col, asynchronous=True)

    def results(eng):
        eng.sync()
        return np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)

    # both kernels agree with the placement before anything is timed: clean, then one flipped byte
    ci, r = nch // 3, p - 1
    at = int(Bs[ci]) - 2
    spot = int(par_off[ci]) + r * int(Bs[ci]) + at
    for bs, eng in enumerate(engs):
        for fn in (check, decode_check):
            b0, d0 = eng.check_methods()
            out.zero_()
            fn(eng)
            assert (results(eng)["first"] == CHK_CONSISTENT).all(), "clean data"
            assert eng.check_methods() == ((b0 + nch, d0) if bs else (b0, d0 + nch)), "the path under test"
            assert fn is check or torch.equal(out, src), "decode + check output"
            par[spot] ^= 0x10
            fn(eng)
            got = results(eng)
            par[spot] ^= 0x10
            assert int(got[ci]["first"]) == at and int(got[ci]["nbad"]) == 1 and int(rb[ci * m + k + r]) == 1
            assert int((got["first"] != CHK_CONSISTENT).sum()) == 1

    def timed(fn, eng, kind):
        for _ in range(2):  # untimed lead-in: plan cached, steady state
            fn(eng)
        eng.sync()
        eng.set_timing(True)
        for _ in range(reps):
            fn(eng)
        eng.sync()
        eng.set_timing(False)
        return eng.collect_timing(kind)[0] / reps

    sched = [("check", check, 0), ("check", check, 1), ("decode_check", decode_check, 0),
             ("decode_check", decode_check, 1)]
    samples = {(kind, bs): [] for kind, _, bs in sched}
    for _ in range(rounds):
        for kind, fn, bs in sched:
            samples[(kind, bs)].append(timed(fn, engs[bs], kind))
    read = int((Bs * np.uint64(m)).sum())
    moved = {"check": read, "decode_check": read + total}
    o = {"case": f"{nch} chunks of {sorted(set(int(x) for x in sizes))} B zfec({k},{m}), all {m} pieces held, "
                 "data pieces the basis", "B": sorted(set(int(x) for x in Bs))}
    for kind in ("check", "decode_check"):
        o[kind] = {"bytes_moved": moved[kind]}
        for bs in (0, 1):
            ms = float(np.median(samples[(kind, bs)]))
            tbs = moved[kind] / (ms / 1e3) / 1e12
            o[kind]["bitsliced" if bs else "direct"] = {
                "ms": round(ms, 4), "ms_rounds": [round(x, 4) for x in samples[(kind, bs)]], "TBs": round(tbs, 3),
                "fraction_of_8TBs": round(tbs / PEAK_TBS, 3)}
        o[kind]["bitsliced_over_direct"] = round(o[kind]["direct"]["ms"] / o[kind]["bitsliced"]["ms"], 3)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--extra", action="store_true", help="the EXTRA cases as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_bs_rate.json"))
    a = ap.parse_args()

    import torch

    import bench
    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_check_bs needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    engs = [Engine(0, options={"SEC_CHECK_BS": 0}), Engine(0, options={"SEC_CHECK_BS": 1})]
    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing); median of {a.rounds} rounds "
                     f"of {a.reps} steps, the four schedules (check / decode + check x SEC_CHECK_BS 0 / 1) "
                     "interleaved per round, 2 untimed lead-in steps each; bytes from the shapes (check: n B read; "
                     "decode + check: that plus the chunk written); bitsliced_over_direct = direct ms / bit-sliced ms",
           "lib_digest": bench.lib_digest(), "cases": {}}
    for c in CASES + (EXTRA if a.extra else []):
        if a.only and c["name"] not in a.only.split(","):
            continue
        res["cases"][c["name"]] = run_case(engs, torch, c, a.rounds, a.reps)
        print(json.dumps({c["name"]: res["cases"][c["name"]]}), flush=True)
        torch.cuda.empty_cache()
    for e in engs:
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
