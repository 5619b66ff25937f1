#!/usr/bin/env python3
"""Corrected decode (sec_decode_correct_batch) against the route the library had before it, on the
same device-resident buffers in one process.  Both routes start with the fused round one over every
chunk (sec_decode_check_batch: what piece.decode_chunks_checked and decode_chunks_corrected both
call first); they differ in what the chunks it reports inconsistent cost:

  new      sec_decode_correct_batch over the damaged chunks: every position's column judged and the
           chunk decoded from the corrected basis, one pass: reads n * B, writes k * B per chunk
  today    sec_check_batch over the damaged chunks without the named piece (n - 1 pieces), then
           sec_decode_batch_ex from k of the rest: reads (n - 1) * B + k * B, writes k * B

so per damaged chunk, round one included, new reads 2 n B and today's n B + (n - 1) B + k B, and
both write 2 k B.  The damaged piece is data piece 1 (a basis entry, so today's route has to decode
again).  Cases: 1024 x 1 MiB RS(4,2) with one 512-byte sector of that piece damaged in every chunk,
with the whole piece junk in every chunk, and with the sector damaged in 1 % of the chunks;
8192 x 64 KiB RS(10,4) and 128 x 8 MiB zfec(16,24) with the sector damaged in every chunk.  Both
routes' outputs are compared with the source before anything is timed.  Kernel times are the
library's HIP events (sec_ctx_set_timing), summed over a route's calls; wall time is the host's
clock around the same steps, synchronised.  Every schedule gets a lead-in step, then `--reps`
steps per round, `--rounds` rounds interleaved over the schedules, median of the rounds.  Each case
runs in a child process of its own under a time limit; the first one that fails ends the run.

    python tools/bench_decode_correct.py [--rounds 5] [--reps 5] [--out profiles/decode_correct_rate.json]
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE_TIMEOUT_S = 280
SECTOR = 512

CASES = [
    dict(name="c2_rs4_2_sector", nch=1024, n=1 << 20, k=4, m=6, damage="sector", every=1),
    dict(name="c2_rs4_2_junk", nch=1024, n=1 << 20, k=4, m=6, damage="junk", every=1),
    dict(name="c2_rs4_2_sector_1pct", nch=1024, n=1 << 20, k=4, m=6, damage="sector", every=100),
    dict(name="c4_rs10_4_sector", nch=8192, n=64 << 10, k=10, m=14, damage="sector", every=1),
    dict(name="zfec16_24_8MiB_sector", nch=128, n=8 << 20, k=16, m=24, damage="sector", every=1),
]
BAD_PIECE = 1


def run_case(eng, torch, c, rounds, reps):
    from storb_amd._lib import (CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, COR_RESULT_DTYPE, DCHK_DTYPE, DEC_DTYPE,
                                ENC_DTYPE)

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

    # the pieces as held: a copy of the data with the damage in it (the source stays the reference)
    held = src.clone()
    bad = list(range(0, nch, c["every"]))
    nbad_pos = 0
    for ci in bad:
        o = ci * n + BAD_PIECE * B
        if c["damage"] == "sector":
            at = (ci * 7919) % (B - SECTOR)
            held[o + at:o + at + SECTOR] ^= 0xA5
            nbad_pos += SECTOR
        else:
            junk = torch.randint(0, 256, (B,), dtype=torch.uint8, device="cuda:0", generator=g)
            nbad_pos += int((junk != held[o:o + B]).sum())
            held[o:o + B] = junk
    nb = len(bad)

    def block_addr(ci, s):
        return (held.data_ptr() + ci * n + s * B) if s < k else (par.data_ptr() + (ci * p + s - k) * B)

    def arrays(chunks, entries):
        nh = len(entries)
        sn = np.tile(np.array(entries, np.int32), len(chunks))
        bo = np.array([block_addr(ci, s) for ci in chunks for s in entries], np.uint64)
        av = np.array([(B - padlen if s == k - 1 else B) for _ in chunks for s in entries], np.uint64)
        return nh, sn, bo, av, np.arange(len(chunks), dtype=np.uint64) * nh

    def dchk(chunks, nh, slot0):
        d = np.zeros(len(chunks), dtype=DCHK_DTYPE)
        d["out_off"] = np.array(chunks, dtype=np.uint64) * n
        d["B"], d["padlen"], d["slot0"], d["n"], d["k"], d["m"] = B, padlen, slot0, nh, k, m
        return d

    every = list(range(nch))
    nh, sn, bo, av, slot0 = arrays(every, list(range(m)))  # round one: every piece of every chunk
    fd = dchk(every, nh, slot0)
    _, bsn, bbo, bav, bslot0 = arrays(bad, list(range(m)))  # new: the damaged chunks, every piece
    cor = dchk(bad, m, bslot0)
    rest = [s for s in range(k) if s != BAD_PIECE] + [k] + list(range(k + 1, m))  # today: without the named piece
    rh, rsn, rbo, rav, rslot0 = arrays(bad, rest)
    cd = np.zeros(nb, dtype=CHK_DTYPE)
    cd["B"], cd["slot0"], cd["n"], cd["k"], cd["m"] = B, rslot0, rh, k, m
    dd = np.zeros(nb, dtype=DEC_DTYPE)
    dd["out_off"] = np.array(bad, dtype=np.uint64) * n
    dd["B"], dd["padlen"], dd["slot0"], dd["k"], dd["m"] = B, padlen, rslot0, k, m

    out = torch.zeros(nch * n, dtype=torch.uint8, device="cuda:0")
    out2 = torch.zeros(nch * n, dtype=torch.uint8, device="cuda:0")
    res, res2 = (torch.zeros(16 * nch, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    res3 = torch.zeros(16 * nb, dtype=torch.uint8, device="cuda:0")
    cres = torch.zeros(24 * nb, dtype=torch.uint8, device="cuda:0")
    hits = torch.zeros(nb * m, dtype=torch.int32, device="cuda:0")

    def round_one(o, r):
        eng.decode_check_batch(fd, sn, bo, 0, o, r, block_avail=av, asynchronous=True)

    def new():
        round_one(out, res)
        eng.decode_correct_batch(cor, bsn, bbo, 0, out, cres, block_avail=bav, entry_hits=hits, asynchronous=True)

    def today():
        round_one(out2, res2)
        eng.check_batch(cd, rsn, rbo, 0, res3, block_avail=rav, asynchronous=True)
        eng.decode_batch(dd, rsn, rbo, 0, out2, block_avail=rav, asynchronous=True)

    # both routes give the source back, and report what the damage is, before anything is timed
    new()
    today()
    eng.sync()
    assert torch.equal(out, src), "corrected decode"
    assert torch.equal(out2, src), "today's route"
    got = np.frombuffer(cres.cpu().numpy().tobytes(), dtype=COR_RESULT_DTYPE)
    assert int(got["corrected"].sum()) == nbad_pos and int(got["open"].sum()) == 0
    h = hits.cpu().numpy().reshape(nb, m)
    assert int(h[:, BAD_PIECE].sum()) == nbad_pos and int(h.sum()) == nbad_pos
    first = np.frombuffer(res.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)["first"]
    assert sorted(np.flatnonzero(first != CHK_CONSISTENT).tolist()) == bad
    assert (np.frombuffer(res3.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)["first"] == CHK_CONSISTENT).all()

    def timed(fn, kinds):
        fn()  # untimed lead-in: plans cached
        eng.sync()
        eng.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        eng.sync()
        wall = (time.perf_counter() - t0) * 1e3 / reps
        eng.set_timing(False)
        return {kd: eng.collect_timing(kd)[0] / reps for kd in kinds}, wall

    kinds = {"new": ["decode_check", "decode_correct"], "today": ["decode_check", "check", "decode"]}
    samples = {name: [] for name in kinds}
    for _ in range(rounds):
        for name, fn in (("new", new), ("today", today)):
            samples[name].append(timed(fn, kinds[name]))
    nall = m
    moved = {"new": {"read": (nch * nall + nb * nall) * B, "written": (nch + nb) * k * B},
             "today": {"read": (nch * nall + nb * (nall - 1) + nb * k) * B, "written": (nch + nb) * k * B}}
    r = {"case": f"{nch} x {n} B zfec({k},{m}), every piece held, {c['damage']} of data piece {BAD_PIECE} damaged in "
                 f"{nb} chunk(s)", "B": B, "damaged_chunks": nb, "damaged_positions": nbad_pos, "reps": reps}
    for name, s in samples.items():
        kernel = [sum(t.values()) for t, _ in s]
        ms = float(np.median(kernel))
        r[name] = {"bytes_read": int(moved[name]["read"]), "bytes_written": int(moved[name]["written"]),
                   "kernel_ms": round(ms, 4), "kernel_ms_rounds": [round(x, 4) for x in kernel],
                   "kernel_ms_by_kind": {kd: round(float(np.median([t[kd] for t, _ in s])), 4) for kd in kinds[name]},
                   "wall_ms": round(float(np.median([w for _, w in s])), 4),
                   "spread": round((max(kernel) - min(kernel)) / ms, 4),
                   "TBs": round((moved[name]["read"] + moved[name]["written"]) / (ms / 1e3) / 1e12, 3)}
    r["today_over_new"] = round(r["today"]["kernel_ms"] / r["new"]["kernel_ms"], 3)
    return r


def child(a):
    import torch

    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_decode_correct needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    eng = Engine(0)
    c = next(c for c in CASES if c["name"] == a.case)
    r = run_case(eng, torch, c, a.rounds, a.reps)
    eng.close()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_correct_rate.json"))
    ap.add_argument("--case", help=argparse.SUPPRESS)  # child process: one case
    a = ap.parse_args()
    if a.case:
        return child(a)

    import bench

    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing), summed over a route's calls "
                     f"(new: decode_check + decode_correct; today: decode_check + check + decode); wall: the host's "
                     f"clock around the same steps; median of {a.rounds} rounds of {a.reps} steps, routes interleaved "
                     "per round, one untimed lead-in step each; spread = (max - min) / median over the rounds; bytes "
                     "from the shapes; one process per case",
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
        with open(a.out, "w") as f:  # (rewritten after every case: a later one's failure keeps the earlier results)
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
