#!/usr/bin/env python3
"""Verified repair (sec_repair_check_batch) against the route the library had before it, on the same
device-resident buffers in one process:

  fused    sec_repair_check_batch: the t lost pieces regenerated from k of the n held pieces and the
           other n - k compared with their prediction, in one pass: reads n * B, writes t * B per chunk
  route    sec_check_batch, then sec_repair_batch from the first k entries, on the same arrays:
           reads (n + k) * B, writes t * B

Cases: 1024 x 1 MiB RS(4,2) with piece 1 lost, 8192 x 64 KiB RS(10,4) with piece 2 lost, 128 x 8 MiB
zfec(16,24) with pieces 1 and 17 lost; every other piece is held.  The basis is the held data pieces
and the first held parity pieces, the other parity pieces are the check rows.  Kernel times are the
library's HIP events (sec_ctx_set_timing, on the kernels' dispatch packets), the route's the sum of
its two calls'.  Every schedule gets 2 untimed lead-in steps, then `--reps` steps per round,
`--rounds` rounds interleaved over the schedules, median of the rounds.  Bytes are the algorithm's,
from the shapes.  Each case runs in a child process of its own under a time limit; the first one
that fails ends the run.

    python tools/bench_repair_check.py [--rounds 5] [--reps 10] [--out profiles/repair_check_rate.json]
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0  # MI355X HBM3E
CASE_TIMEOUT_S = 240

CASES = [
    dict(name="c2_rs4_2", nch=1024, n=1 << 20, k=4, m=6, lost=[1]),
    dict(name="c4_rs10_4", nch=8192, n=64 << 10, k=10, m=14, lost=[2]),
    dict(name="zfec16_24_8MiB", nch=128, n=8 << 20, k=16, m=24, lost=[1, 17]),
]


def run_case(eng, torch, c, rounds, reps):
    from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, ENC_DTYPE, RCHK_DTYPE, REP_DTYPE

    nch, n, k, m, lost = c["nch"], c["n"], c["k"], c["m"], c["lost"]
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

    entries = [s for s in range(m) if s not in lost]  # the held data pieces, then parity: the first k the basis
    nh, t = len(entries), len(lost)
    sn = np.tile(np.array(entries, np.int32), nch)
    bo = np.array([block_addr(ci, s) for ci in range(nch) for s in entries], np.uint64)
    av = np.array([(B - padlen if s == k - 1 else B) for _ in range(nch) for s in entries], np.uint64)
    tn = np.tile(np.array(lost, np.int32), nch)
    to = np.arange(nch * t, dtype=np.uint64) * B
    slot0 = np.arange(nch, dtype=np.uint64) * nh
    tgt0 = np.arange(nch, dtype=np.uint64) * t
    fd = np.zeros(nch, dtype=RCHK_DTYPE)
    fd["B"], fd["slot0"], fd["tgt0"], fd["ntargets"], fd["n"], fd["k"], fd["m"] = B, slot0, tgt0, t, nh, k, m
    cd = np.zeros(nch, dtype=CHK_DTYPE)
    cd["B"], cd["slot0"], cd["n"], cd["k"], cd["m"] = B, slot0, nh, k, m
    rd = np.zeros(nch, dtype=REP_DTYPE)
    rd["B"], rd["slot0"], rd["tgt0"], rd["ntargets"], rd["k"], rd["m"] = B, slot0, tgt0, t, k, m
    out = torch.zeros(nch * t * B, dtype=torch.uint8, device="cuda:0")
    out2 = torch.zeros(nch * t * B, dtype=torch.uint8, device="cuda:0")
    res, res2 = (torch.zeros(16 * nch, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    rb, rb2, col, col2 = (torch.zeros(nch * nh, dtype=torch.uint8, device="cuda:0") for _ in range(4))

    def fused():
        eng.repair_check_batch(fd, sn, bo, 0, tn, to, out, res, block_avail=av, row_bad=rb, column=col,
                               asynchronous=True)

    def route_check():
        eng.check_batch(cd, sn, bo, 0, res2, block_avail=av, row_bad=rb2, column=col2, asynchronous=True)

    def route_repair():
        eng.repair_batch(rd, sn, bo, 0, tn, to, out2, block_avail=av, asynchronous=True)

    def results(r):
        eng.sync()
        return np.frombuffer(r.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)

    def want_target(ci, s):  # the lost piece as encoded (a data piece: the chunk's bytes, zero-padded)
        if s >= k:
            return par[(ci * p + s - k) * B:(ci * p + s - k + 1) * B]
        piece = torch.zeros(B, dtype=torch.uint8, device="cuda:0")
        have = min(B, n - s * B)
        piece[:have] = src[ci * n + s * B:ci * n + s * B + have]
        return piece

    # both schedules agree before anything is timed: clean, then one flipped check-row byte
    fused()
    route_check()
    route_repair()
    assert (results(res)["first"] == CHK_CONSISTENT).all() and torch.equal(res, res2), "clean data"
    assert torch.equal(out, out2), "repaired pieces"
    for ci in (0, nch // 2, nch - 1):
        for j, s in enumerate(lost):
            assert torch.equal(out[(ci * t + j) * B:(ci * t + j + 1) * B], want_target(ci, s)), "repaired piece"
    ci, at = nch // 3, B - 2
    r = entries[-1] - k  # the last check row's parity row
    par[(ci * p + r) * B + at] ^= 0x10
    fused()
    route_check()
    got = results(res)
    assert int(got[ci]["first"]) == at and int(got[ci]["nbad"]) == 1 and int(rb[ci * nh + nh - 1]) == 1
    assert int((got["first"] != CHK_CONSISTENT).sum()) == 1 and torch.equal(res, res2) and torch.equal(rb, rb2)
    assert torch.equal(out, out2), "a corrupt check row leaves the repaired pieces alone"
    par[(ci * p + r) * B + at] ^= 0x10

    def timed(fns, kinds):
        for _ in range(2):  # untimed lead-in: plan cached, steady state
            for fn in fns:
                fn()
        eng.sync()
        eng.set_timing(True)
        for _ in range(reps):
            for fn in fns:
                fn()
        eng.sync()
        eng.set_timing(False)
        return [eng.collect_timing(kd)[0] / reps for kd in kinds]

    samples = {"fused": [], "route_check": [], "route_repair": []}
    for _ in range(rounds):
        samples["fused"].append(timed([fused], ["repair_check"])[0])
        ck, rp = timed([route_check, route_repair], ["check", "repair"])
        samples["route_check"].append(ck)
        samples["route_repair"].append(rp)
    samples["route"] = [a + b for a, b in zip(samples["route_check"], samples["route_repair"])]
    moved = {"fused": nch * (nh + t) * B, "route_check": nch * nh * B, "route_repair": nch * (k + t) * B,
             "route": nch * (nh + k + t) * B}
    res_out = {"case": f"{nch} x {n} B zfec({k},{m}), pieces {lost} lost, {nh} held", "B": B, "held": nh, "targets": t}
    for name, s in samples.items():
        ms = float(np.median(s))
        tbs = moved[name] / (ms / 1e3) / 1e12
        res_out[name] = {"bytes_moved": int(moved[name]), "ms": round(ms, 4), "ms_rounds": [round(x, 4) for x in s],
                         "spread": round((max(s) - min(s)) / ms, 4), "TBs": round(tbs, 3),
                         "fraction_of_8TBs": round(tbs / PEAK_TBS, 3)}
    res_out["route_over_fused"] = round(res_out["route"]["ms"] / res_out["fused"]["ms"], 3)
    res_out["route_over_fused_by_bytes"] = round((nh + k + t) / (nh + t), 3)
    return res_out


def child(a):
    import torch

    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_repair_check needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    eng = Engine(0)
    c = next(c for c in CASES if c["name"] == a.case)
    r = run_case(eng, torch, c, a.rounds, a.reps)
    eng.close()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_check_rate.json"))
    ap.add_argument("--case", help=argparse.SUPPRESS)  # child process: one case
    a = ap.parse_args()
    if a.case:
        return child(a)

    import bench

    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing), kind repair_check for fused, "
                     f"check + repair for the route; median of {a.rounds} rounds of {a.reps} steps, schedules "
                     "interleaved per round, 2 untimed lead-in steps each; spread = (max - min) / median over the "
                     "rounds; bytes from the shapes; one process per case",
           "lib_digest": bench.lib_digest(), "cases": {}}
    for c in CASES:
        if a.only and c["name"] not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", c["name"], "--rounds", str(a.rounds), "--reps",
               str(a.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"{c['name']}: no result within {CASE_TIMEOUT_S} s; nothing more is started")
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"{c['name']}: exit status {p.returncode}; nothing more is started")
        res["cases"][c["name"]] = json.loads(line[len("RESULT "):])
        print(json.dumps({c["name"]: res["cases"][c["name"]]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
