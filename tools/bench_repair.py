#!/usr/bin/env python3
"""Piece repair (sec_repair_batch) against the only route the library had before it, on the same
device-resident buffers in one process:

  repair       sec_repair_batch: the lost pieces, data and parity, from k survivors
  route        sec_decode_batch reassembly of the chunk from the same k survivors, then
               sec_encode_batch of the reassembled chunk (every parity piece again)
  repair_data  sec_repair_batch of the lost DATA pieces only
  recover      sec_decode_batch SEC_F_RECOVER from the same survivors: the existing kernel that
               moves the same bytes as repair_data

Cases: 1024 x 1 MiB RS(4,2) sources {0,2,3,4} targets {1,5}; 8192 x 64 KiB RS(10,4) with two data
and one parity piece lost; zfec(16,24) on 8 MiB chunks with four data and four parity pieces lost.
Kernel times are the library's HIP events (sec_ctx_set_timing; per launch, on the kernels' own
dispatch packets); every schedule is warmed up, then `--reps` steps per round, `--rounds` rounds
interleaved over the schedules, median of the rounds.  Bytes are the algorithm's: what each
route must read and write, computed from the shapes.

    python tools/bench_repair.py [--rounds 5] [--reps 10] [--out profiles/repair_rate.json]
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
    dict(name="c2_rs4_2", nch=1024, n=1 << 20, k=4, m=6, lost=[1, 5]),
    dict(name="c4_rs10_4", nch=8192, n=64 << 10, k=10, m=14, lost=[2, 7, 12]),
    dict(name="zfec16_24_8MiB", nch=128, n=8 << 20, k=16, m=24, lost=[1, 5, 9, 13, 17, 19, 21, 23]),
]


def run_case(eng, torch, c, rounds, reps):
    from storb_amd._lib import DEC_DTYPE, ENC_DTYPE, REP_DTYPE

    nch, n, k, m, lost = c["nch"], c["n"], c["k"], c["m"], c["lost"]
    p = m - k
    B = -(-n // k)
    padlen = k * B - n
    # the k survivors the repair reads: every surviving data piece, then the lowest parity pieces
    alive = [s for s in range(m) if s not in lost]
    srcs = [s for s in alive if s < k]
    srcs += [s for s in alive if s >= k][:k - len(srcs)]
    assert len(srcs) == k
    lost_data = [t for t in lost if t < k]
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

    sn = np.tile(np.array(srcs, np.int32), nch)
    bo = np.array([block_addr(ci, s) for ci in range(nch) for s in srcs], np.uint64)
    av = np.array([(B - padlen if s == k - 1 else B) for _ in range(nch) for s in srcs], np.uint64)

    def rep_args(targets):
        nt = len(targets)
        d = np.zeros(nch, dtype=REP_DTYPE)
        d["B"], d["k"], d["m"], d["ntargets"] = B, k, m, nt
        d["slot0"] = np.arange(nch, dtype=np.uint64) * k
        d["tgt0"] = np.arange(nch, dtype=np.uint64) * nt
        tn = np.tile(np.array(targets, np.int32), nch)
        to = np.arange(nch * nt, dtype=np.uint64) * B
        return d, tn, to

    rd, rtn, rto = rep_args(lost)
    dd_, dtn, dto = rep_args(lost_data)
    tgt = torch.empty(nch * len(lost) * B, dtype=torch.uint8, device="cuda:0")
    # the old route: reassemble into `out`, encode `out` into par2
    out = torch.empty(nch * n, dtype=torch.uint8, device="cuda:0")
    par2 = torch.empty_like(par)
    dec = np.zeros(nch, dtype=DEC_DTYPE)
    dec["out_off"] = np.arange(nch, dtype=np.uint64) * n
    dec["B"], dec["padlen"], dec["k"], dec["m"] = B, padlen, k, m
    dec["slot0"] = np.arange(nch, dtype=np.uint64) * k
    rec = dec.copy()
    rec["out_off"] = np.arange(nch, dtype=np.uint64) * (len(lost_data) * B)
    rout = torch.empty(max(nch * len(lost_data) * B, 1), dtype=torch.uint8, device="cuda:0")

    def repair():
        eng.repair_batch(rd, sn, bo, 0, rtn, rto, tgt, block_avail=av, asynchronous=True)

    def repair_data():
        eng.repair_batch(dd_, sn, bo, 0, dtn, dto, tgt, block_avail=av, asynchronous=True)

    def route():
        eng.decode_batch(dec, sn, bo, 0, out, block_avail=av, asynchronous=True)
        eng.encode_batch(ed, out, par2, asynchronous=True)

    def recover():
        eng.decode_batch(rec, sn, bo, 0, rout, block_avail=av, recover_only=True, asynchronous=True)

    # same bytes from both routes before anything is timed
    repair()
    route()
    eng.sync()
    assert torch.equal(out, src) and torch.equal(par2, par), "old route"
    t3 = tgt.view(nch, len(lost), B)
    for j, t in enumerate(lost):
        if t >= k:
            want = par.view(nch, p, B)[:, t - k]
        else:
            want = torch.zeros(nch, B, dtype=torch.uint8, device="cuda:0")
            w = min(B, n - t * B)
            want[:, :w] = src.view(nch, n)[:, t * B:t * B + w]
        assert torch.equal(t3[:, j], want), f"repaired piece {t}"

    schedules = {"repair": (repair, ("repair",)), "route": (route, ("decode", "encode")),
                 "repair_data": (repair_data, ("repair",)), "recover": (recover, ("decode",))}
    samples = {s: [] for s in schedules}
    for _ in range(rounds):
        for name, (fn, kinds) in schedules.items():
            for _ in range(2):  # untimed lead-in: plan cached, steady state
                fn()
            eng.sync()
            eng.set_timing(True)
            for _ in range(reps):
                fn()
            eng.sync()
            eng.set_timing(False)
            samples[name].append(sum(eng.collect_timing(kd)[0] for kd in kinds) / reps)
    nt, e = len(lost), len(lost_data)
    moved = {"repair": nch * (k + nt) * B, "route": nch * (k * B + n + n + p * B),
             "repair_data": nch * (k + e) * B, "recover": nch * (k + e) * B}
    res = {"case": f"{nch} x {n} B zfec({k},{m}), sources {srcs}, lost {lost}", "B": B}
    for name, s in samples.items():
        ms = float(np.median(s))
        tbs = moved[name] / (ms / 1e3) / 1e12
        res[name] = {"bytes_moved": int(moved[name]), "ms": round(ms, 4), "ms_rounds": [round(x, 4) for x in s],
                     "TBs": round(tbs, 3), "fraction_of_8TBs": round(tbs / PEAK_TBS, 3)}
    res["route_over_repair"] = round(res["route"]["ms"] / res["repair"]["ms"], 3)
    res["route_over_repair_by_bytes"] = round(moved["route"] / moved["repair"], 3)
    res["recover_over_repair_data"] = round(res["recover"]["ms"] / res["repair_data"]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_rate.json"))
    a = ap.parse_args()

    import torch

    import bench
    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_repair needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    eng = Engine(0)
    res = {"method": f"per-launch HIP events (sec_ctx_set_timing), median of {a.rounds} rounds of {a.reps} steps, "
                     "schedules interleaved per round, 2 untimed lead-in steps each; route = decode + encode kernels "
                     "of one step; bytes from the shapes",
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
