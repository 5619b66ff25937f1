#!/usr/bin/env python3
"""The bit-sliced repair kernel (sec_repair_bs_kernel) against the direct (v_perm) repair kernels, on
the same device-resident buffers in one process: every data piece of every chunk held and the basis
(choose_blocks' pick when all are held), block k-1 read in place with its avail, the lost pieces all
parity.

  repair         sec_repair_batch: reads k * B per chunk, writes lost * B
  repair_check   sec_repair_check_batch with every surviving piece held: reads (m - lost) * B per
                 chunk, writes lost * B and the results

each with SEC_CHECK_BS = 0 (direct, the yardstick) and = 1 (bit-sliced), on two contexts of the same
process so neither re-plans when the other runs.  Kernel times are the library's per-launch HIP
events (sec_ctx_set_timing).  Every schedule gets 2 untimed lead-in steps, then `--reps` steps per
round, `--rounds` rounds interleaved over a case's schedules, median of the rounds.  Bytes are the
algorithm's, from the shapes.  Before anything is timed both paths must reproduce the encode's
parity rows in the targets, report a clean batch clean and find one flipped parity byte.

    python tools/bench_repair_bs.py [--rounds 5] [--reps 10] [--only NAMES]
                                    [--out profiles/repair_bs_rate.json]
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


def rows(first, count):
    return list(range(first, first + count))


# lost: name -> the parity pieces lost (a plain repair from the k data pieces);
# every shape also runs repair + check with 1 and 2 pieces lost and every other piece held
CASES = [
    dict(name="zfec16_24_8MiB", sizes=[8 << 20] * 128, k=16, m=24,
         lost={"1": [16], "2": [16, 20], "4": [16, 18, 20, 22], "8": rows(16, 8)}),
    dict(name="zfec16_24_1MiB", sizes=[1 << 20] * 1024, k=16, m=24,
         lost={"1": [16], "2": [16, 20], "4": [16, 18, 20, 22], "8": rows(16, 8)}),
    dict(name="zfec32_48_1MiB", sizes=[1 << 20] * 1024, k=32, m=48,
         lost={"1": [32], "4": [32, 36, 40, 44], "16": rows(32, 16)}),
    dict(name="zfec32_48_64MiB", sizes=[64 << 20] * 16, k=32, m=48,
         lost={"1": [32], "4": [32, 36, 40, 44], "16": rows(32, 16)}),
    dict(name="zfec64_96_1MiB", sizes=[1 << 20] * 1024, k=64, m=96,
         lost={"1": [64], "8": rows(64, 8), "16_one_group": rows(64, 16), "16_both_groups": rows(72, 16),
               "32": rows(64, 32)}),
    dict(name="zfec64_96_256MiB", sizes=[256 << 20] * 4, k=64, m=96,
         lost={"1": [64], "8": rows(64, 8), "16_one_group": rows(64, 16), "16_both_groups": rows(72, 16),
               "32": rows(64, 32)}),
    dict(name="c4_rs10_4", sizes=[64 << 10] * 8192, k=10, m=14, lost={"1": [10], "2": [10, 12], "4": rows(10, 4)}),
    dict(name="zfec8_12_4MiB", sizes=[4 << 20] * 256, k=8, m=12, lost={"4": rows(8, 4)}),
]


def run_case(engs, torch, c, rounds, reps):
    from storb_amd._lib import CHK_CONSISTENT, CHK_RESULT_DTYPE, ENC_DTYPE, RCHK_DTYPE, REP_DTYPE

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
    tgt = torch.empty(ptotal, dtype=torch.uint8, device="cuda:0")  # targets land where the encode put them
    ed = np.zeros(nch, dtype=ENC_DTYPE)
    ed["in_off"], ed["n"], ed["parity_off"], ed["parity_stride"], ed["k"], ed["m"] = in_off, sizes, par_off, Bs, k, m
    engs[0].encode_batch(ed, src, par)

    s = np.arange(m, dtype=np.uint64)[None, :]
    data_addr = np.uint64(src.data_ptr()) + in_off[:, None] + s * Bs[:, None]
    par_addr = np.uint64(par.data_ptr()) + par_off[:, None] + (s - np.uint64(k)) * Bs[:, None]
    addr = np.where(s < k, data_addr, par_addr).astype(np.uint64)
    avail = np.where(s == k - 1, (Bs - pad)[:, None], Bs[:, None]).astype(np.uint64)
    res = torch.zeros(16 * nch, dtype=torch.uint8, device="cuda:0")
    rb = torch.zeros(nch * m, dtype=torch.uint8, device="cuda:0")
    col = torch.zeros(nch * m, dtype=torch.uint8, device="cuda:0")

    def make(lost, checks):
        """The call's arrays: entries = the data pieces (then, with checks, every surviving parity
        piece), targets = `lost` at their place in a parity-shaped buffer."""
        held = rows(0, k) + ([r for r in range(k, m) if r not in lost] if checks else [])
        n, nt = len(held), len(lost)
        a = dict(sn=np.tile(np.array(held, np.int32), nch), bo=addr[:, held].ravel().copy(),
                 av=avail[:, held].ravel().copy(), tn=np.tile(np.array(lost, np.int32), nch),
                 to=(par_off[:, None] + (np.array(lost, np.uint64) - np.uint64(k))[None, :] * Bs[:, None]).ravel(),
                 n=n, nt=nt, held=held, lost=lost, checks=checks)
        d = np.zeros(nch, dtype=RCHK_DTYPE if checks else REP_DTYPE)
        d["B"], d["ntargets"], d["k"], d["m"] = Bs, nt, k, m
        d["slot0"] = np.arange(nch, dtype=np.uint64) * n
        d["tgt0"] = np.arange(nch, dtype=np.uint64) * nt
        if checks:
            d["n"] = n
        a["descs"] = d
        a["moved"] = int((Bs * np.uint64(n + nt)).sum())
        return a

    def call(eng, a):
        if a["checks"]:
            eng.repair_check_batch(a["descs"], a["sn"], a["bo"], 0, a["tn"], a["to"], tgt, res, block_avail=a["av"],
                                   row_bad=rb, column=col, asynchronous=True)
        else:
            eng.repair_batch(a["descs"], a["sn"], a["bo"], 0, a["tn"], a["to"], tgt, block_avail=a["av"],
                             asynchronous=True)

    def results(eng):
        eng.sync()
        return np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)

    def targets_right(a):
        """every target equals the encode's row (chunk by chunk: the rows between are not written)"""
        for ci in (0, nch // 3, nch - 1):
            B, o = int(Bs[ci]), int(par_off[ci])
            for t in a["lost"]:
                lo = o + (t - k) * B
                if not torch.equal(tgt[lo:lo + B], par[lo:lo + B]):
                    return False
        return True

    # both kernels against the encode before anything is timed: the targets, clean results, and one
    # flipped byte in a held parity piece found
    scheds = [("repair", name, make(lost, False)) for name, lost in c["lost"].items()]
    scheds += [("repair_check", f"{nl}", make(rows(k, nl), True)) for nl in (1, 2)]
    for bs, eng in enumerate(engs):
        for kind, name, a in scheds:
            b0, d0 = eng.repair_methods()
            tgt.zero_()
            call(eng, a)
            eng.sync()
            assert eng.repair_methods() == ((b0 + nch, d0) if bs else (b0, d0 + nch)), "the path under test"
            assert targets_right(a), f"{kind} {name}: targets"
            if not a["checks"]:
                continue
            assert (results(eng)["first"] == CHK_CONSISTENT).all(), "clean data"
            ci, r = nch // 3, m - 1  # the last parity piece is held in both repair + check schedules
            at = int(Bs[ci]) - 2
            spot = int(par_off[ci]) + (r - k) * int(Bs[ci]) + at
            par[spot] ^= 0x10
            call(eng, a)
            got = results(eng)
            par[spot] ^= 0x10
            assert int(got[ci]["first"]) == at and int(got[ci]["nbad"]) == 1
            assert int(rb[ci * a["n"] + a["held"].index(r)]) == 1
            assert int((got["first"] != CHK_CONSISTENT).sum()) == 1

    def timed(eng, kind, a):
        for _ in range(2):  # untimed lead-in: plan cached, steady state
            call(eng, a)
        eng.sync()
        eng.set_timing(True)
        for _ in range(reps):
            call(eng, a)
        eng.sync()
        eng.set_timing(False)
        return eng.collect_timing(kind)[0] / reps

    samples = {(kind, name, bs): [] for kind, name, _ in scheds for bs in (0, 1)}
    for _ in range(rounds):
        for kind, name, a in scheds:
            for bs in (0, 1):
                samples[(kind, name, bs)].append(timed(engs[bs], kind, a))
    o = {"case": f"{nch} chunks of {sorted(set(int(x) for x in sizes))} B zfec({k},{m}), the {k} data pieces the "
                 "basis; repair: they alone held; repair + check: every surviving piece held",
         "B": sorted(set(int(x) for x in Bs)), "repair": {}, "repair_check": {}}
    for kind, name, a in scheds:
        e = {"lost": a["lost"], "compared_rows": a["n"] - k, "bytes_moved": a["moved"]}
        for bs in (0, 1):
            ms = float(np.median(samples[(kind, name, bs)]))
            tbs = a["moved"] / (ms / 1e3) / 1e12
            e["bitsliced" if bs else "direct"] = {
                "ms": round(ms, 4), "ms_rounds": [round(x, 4) for x in samples[(kind, name, bs)]],
                "TBs": round(tbs, 3), "fraction_of_8TBs": round(tbs / PEAK_TBS, 3)}
        e["bitsliced_over_direct"] = round(e["direct"]["ms"] / e["bitsliced"]["ms"], 3)
        o[kind][name] = e
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_bs_rate.json"))
    a = ap.parse_args()

    import torch

    import bench
    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_repair_bs needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    engs = [Engine(0, options={"SEC_CHECK_BS": 0}), Engine(0, options={"SEC_CHECK_BS": 1})]
    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing); median of {a.rounds} rounds "
                     f"of {a.reps} steps, a case's schedules (lost sets x SEC_CHECK_BS 0 / 1) interleaved per "
                     "round, 2 untimed lead-in steps each; bytes from the shapes (held pieces read, lost pieces "
                     "written); bitsliced_over_direct = direct ms / bit-sliced ms on the same build",
           "lib_digest": bench.lib_digest(), "cases": {}}
    for c in CASES:
        if a.only and c["name"] not in a.only.split(","):
            continue
        res["cases"][c["name"]] = run_case(engs, torch, c, a.rounds, a.reps)
        print(json.dumps({c["name"]: res["cases"][c["name"]]}), flush=True)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # after every case: a run cut short keeps what it measured
            json.dump(res, f, indent=1)
            f.write("\n")
    for e in engs:
        e.close()


if __name__ == "__main__":
    main()
