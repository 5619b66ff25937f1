#!/usr/bin/env python3
"""Piece check (sec_check_batch) against the only route the library had before it, on the same
device-resident buffers in one process, every piece of every chunk held (n = m):

  check    sec_check_batch: the m - k parity pieces predicted from the k data pieces and compared
           with the stored ones; reads n * B per chunk, writes nothing but the results
  repair   sec_repair_batch of the same m - k rows from the same k pieces into scratch: the
           repair kernel alone, the same tiles and arithmetic with stores instead of the compare
  route    `repair`, then a compare of the scratch with the stored parity pieces
           ((scratch == parity).all(), two torch kernels): what a caller had to do

Cases: repair's three shapes: 1024 x 1 MiB RS(4,2), 8192 x 64 KiB RS(10,4), zfec(16,24) on 8 MiB
chunks.  Kernel times are HIP events: the library's own (sec_ctx_set_timing; on the kernels'
dispatch packets) for check and repair, torch.cuda events around the compare, whose time is added
to repair's for the route.  Every schedule is warmed up, then `--reps` steps per round, `--rounds`
rounds interleaved over the schedules, median of the rounds.  Bytes are the algorithm's, from the
shapes: check n * B; repair k * B read + (m - k) * B written (the same count); route that plus
2 (m - k) * B read by the compare (torch's temporary not counted).

    python tools/bench_check.py [--rounds 5] [--reps 10] [--out profiles/check_rate.json]
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

CASES = [
    dict(name="c2_rs4_2", nch=1024, n=1 << 20, k=4, m=6),
    dict(name="c4_rs10_4", nch=8192, n=64 << 10, k=10, m=14),
    dict(name="zfec16_24_8MiB", nch=128, n=8 << 20, k=16, m=24),
]


def run_case(eng, torch, c, rounds, reps):
    from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, ENC_DTYPE, REP_DTYPE

    nch, n, k, m = c["nch"], c["n"], c["k"], c["m"]
    p = m - k
    B = -(-n // k)
    padlen = k * B - n
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2024)
    src = torch.randint(0, 256, (nch * n,), dtype=torch.uint8, device="cuda:0", generator=g)
    par = torch.empty(nch * p * B, dtype=torch.uint8, device="cuda:0")
    ed = np.zeros(nch, dtype=ENC_DTYPE)
    ed["in_off"] = np.arange(nch, dtype=np.uint64) * n
    ed["n"], ed["parity_stride"], ed["k"], ed["m"] = n, B, k, m
    ed["parity_off"] = np.arange(nch, dtype=np.uint64) * (p * B)
    eng.encode_batch(ed, src, par)

    def block_addr(ci, s):
        return (src.data_ptr() + ci * n + s * B) if s < k else (par.data_ptr() + (ci * p + s - k) * B)

    # check: all m pieces, the data pieces the basis (choose_blocks' pick when all are held)
    cd = np.zeros(nch, dtype=CHK_DTYPE)
    cd["B"], cd["n"], cd["k"], cd["m"] = B, m, k, m
    cd["slot0"] = np.arange(nch, dtype=np.uint64) * m
    csn = np.tile(np.arange(m, dtype=np.int32), nch)
    cbo = np.array([block_addr(ci, s) for ci in range(nch) for s in range(m)], np.uint64)
    cav = np.array([(B - padlen if s == k - 1 else B) for _ in range(nch) for s in range(m)], np.uint64)
    res = torch.zeros(16 * nch, dtype=torch.uint8, device="cuda:0")
    rb = torch.zeros(nch * m, dtype=torch.uint8, device="cuda:0")
    col = torch.zeros(nch * m, dtype=torch.uint8, device="cuda:0")
    # repair of the same rows from the same k pieces
    rd = np.zeros(nch, dtype=REP_DTYPE)
    rd["B"], rd["k"], rd["m"], rd["ntargets"] = B, k, m, p
    rd["slot0"] = np.arange(nch, dtype=np.uint64) * k
    rd["tgt0"] = np.arange(nch, dtype=np.uint64) * p
    rsn = np.tile(np.arange(k, dtype=np.int32), nch)
    rbo = np.array([block_addr(ci, s) for ci in range(nch) for s in range(k)], np.uint64)
    rav = np.array([(B - padlen if s == k - 1 else B) for _ in range(nch) for s in range(k)], np.uint64)
    rtn = np.tile(np.arange(k, m, dtype=np.int32), nch)
    rto = np.arange(nch * p, dtype=np.uint64) * B
    scratch = torch.empty_like(par)

    def check():
        eng.check_batch(cd, csn, cbo, 0, res, block_avail=cav, row_bad=rb, column=col, asynchronous=True)

    def repair():
        eng.repair_batch(rd, rsn, rbo, 0, rtn, rto, scratch, block_avail=rav, asynchronous=True)

    def results():
        eng.sync()
        return np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)

    # both routes agree before anything is timed: clean, then one flipped parity byte
    check()
    repair()
    assert (results()["first"] == CHK_CONSISTENT).all() and torch.equal(scratch, par), "clean data"
    ci, r, at = nch // 3, p - 1, B - 2
    par[(ci * p + r) * B + at] ^= 0x10
    check()
    got = results()
    assert int(got[ci]["first"]) == at and int(got[ci]["nbad"]) == 1 and int(rb[ci * m + k + r]) == 1
    assert int((got["first"] != CHK_CONSISTENT).sum()) == 1 and not torch.equal(scratch, par)
    par[(ci * p + r) * B + at] ^= 0x10

    def timed(fn, kind):
        for _ in range(2):  # untimed lead-in: plan cached, steady state
            fn()
        eng.sync()
        eng.set_timing(True)
        for _ in range(reps):
            fn()
        eng.sync()
        eng.set_timing(False)
        return eng.collect_timing(kind)[0] / reps

    def compare_ms():
        torch.cuda.synchronize()
        for _ in range(2):
            (scratch == par).all()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            (scratch == par).all()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    samples = {"check": [], "repair": [], "compare": []}
    for _ in range(rounds):
        samples["check"].append(timed(check, "check"))
        samples["repair"].append(timed(repair, "repair"))
        samples["compare"].append(compare_ms())
    moved = {"check": nch * m * B, "repair": nch * m * B, "compare": nch * 2 * p * B}
    out = {"case": f"{nch} x {n} B zfec({k},{m}), all {m} pieces held, data pieces the basis", "B": B}
    for name, s in samples.items():
        ms = float(np.median(s))
        tbs = moved[name] / (ms / 1e3) / 1e12
        out[name] = {"bytes_moved": int(moved[name]), "ms": round(ms, 4), "ms_rounds": [round(x, 4) for x in s],
                     "TBs": round(tbs, 3), "fraction_of_8TBs": round(tbs / PEAK_TBS, 3)}
    route_ms = out["repair"]["ms"] + out["compare"]["ms"]
    out["route"] = {"bytes_moved": int(moved["repair"] + moved["compare"]), "ms": round(route_ms, 4)}
    out["route_over_check"] = round(route_ms / out["check"]["ms"], 3)
    out["route_over_check_by_bytes"] = round((m + 2 * p) / m, 3)
    out["repair_over_check"] = round(out["repair"]["ms"] / out["check"]["ms"], 3)
    out["repair_over_check_by_bytes"] = 1.0  # the same count; the check's are all reads
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_rate.json"))
    a = ap.parse_args()

    import torch

    import bench
    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_check needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    eng = Engine(0)
    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing) for check and repair, "
                     f"torch.cuda events around (scratch == parity).all() for the compare; median of {a.rounds} "
                     f"rounds of {a.reps} steps, schedules interleaved per round, 2 untimed lead-in steps each; "
                     "route = repair + compare; bytes from the shapes",
           "lib_digest": bench.lib_digest(), "cases": {}}
    for c in CASES:
        if a.only and c["name"] not in a.only.split(","):
            continue
        res["cases"][c["name"]] = run_case(eng, torch, c, a.rounds, a.reps)
        print(json.dumps({c["name"]: res["cases"][c["name"]]}), flush=True)
        torch.cuda.empty_cache()
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
