#!/usr/bin/env python3
"""Corrected repair (sec_repair_correct_batch) against the only route that yields the same pieces
without it, on the same device-resident buffers in one process.  Both routes start with the fused
round one over every chunk (sec_repair_check_batch with the lost pieces as targets: what
piece.repair_chunks_checked and repair_chunks_corrected both call first); they differ in what the
chunks it reports inconsistent cost:

  new      sec_repair_correct_batch over the damaged chunks, targets = the lost pieces and the
           damaged held ones: every position's column judged and each target made from the corrected
           basis, one pass: reads n * B, writes ntargets * B per chunk
  old      sec_decode_correct_batch over the damaged chunks (the corrected chunk, k * B), then
           sec_encode_batch on those chunks (every parity row again, (m - k) * B): reads n * B + k * B,
           writes m * B per chunk, and the pieces wanted are picked out of that

Cases: 1024 x 1 MiB RS(4,2) with all six pieces held and a 512-byte sector damaged in data piece 1 and
in parity piece 4 at different offsets, both healed; 8192 x 64 KiB RS(10,4) with data piece 3 lost and
a sector of data piece 1 damaged; 128 x 8 MiB zfec(16,24) with pieces 5 and 20 lost and a sector of
data piece 1 damaged.  Every chunk is damaged.  Both routes' pieces are compared with the source's
before anything is timed.  Kernel times are the library's HIP events (sec_ctx_set_timing), summed
over a route's calls; wall time is the host's clock around the same steps, synchronised.  Every
schedule gets a lead-in step, then `--reps` steps per round, `--rounds` rounds interleaved over the
schedules, median of the rounds.  Each case runs in a child process of its own under a time limit;
the first one that fails ends the run.

    python tools/bench_repair_correct.py [--rounds 5] [--reps 5] [--out profiles/repair_correct_rate.json]
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
    dict(name="c2_rs4_2_heal_two", nch=1024, n=1 << 20, k=4, m=6, lost=[], damaged=[1, 4]),
    dict(name="c4_rs10_4_lost_one", nch=8192, n=64 << 10, k=10, m=14, lost=[3], damaged=[1]),
    dict(name="zfec16_24_8MiB_lost_two", nch=128, n=8 << 20, k=16, m=24, lost=[5, 20], damaged=[1]),
]


def run_case(eng, torch, c, rounds, reps):
    from storb_amd._lib import CHK_CONSISTENT, CHK_RESULT_DTYPE, COR_RESULT_DTYPE, DCHK_DTYPE, ENC_DTYPE, RCHK_DTYPE

    nch, n, k, m, lost, damaged = c["nch"], c["n"], c["k"], c["m"], c["lost"], c["damaged"]
    p = m - k
    B = -(-n // k)
    padlen = k * B - n
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2024)
    src = torch.randint(0, 256, (nch * n,), dtype=torch.uint8, device="cuda:0", generator=g)
    par = torch.empty(nch * p * B, dtype=torch.uint8, device="cuda:0")

    def enc_descs(chunks):
        ed = np.zeros(len(chunks), dtype=ENC_DTYPE)
        ed["in_off"] = np.array(chunks, dtype=np.uint64) * n
        ed["n"], ed["parity_stride"], ed["k"], ed["m"] = n, B, k, m
        ed["parity_off"] = np.array(chunks, dtype=np.uint64) * (p * B)
        return ed

    every = list(range(nch))
    ed = enc_descs(every)
    eng.encode_batch(ed, src, par)

    # the pieces as held: copies with the damage in them (src and par stay the reference)
    held, hpar = src.clone(), par.clone()
    for ci in every:
        for q, s in enumerate(damaged):
            at = (ci * 7919 + q * (B // 2)) % (B - SECTOR)  # different offsets in different pieces
            buf, o = (held, ci * n + s * B) if s < k else (hpar, (ci * p + s - k) * B)
            buf[o + at:o + at + SECTOR] ^= 0xA5
    nbad_pos = nch * SECTOR * len(damaged)

    # entries: the held primaries, the parity pieces that complete the basis, then the check rows
    have = [s for s in range(m) if s not in lost]
    entries = [s for s in have if s < k]
    entries += [s for s in have if s >= k][:k - len(entries)]
    entries += [s for s in have if s not in entries]
    nh = len(entries)
    assert nh - k >= 2

    def block_addr(ci, s):
        return (held.data_ptr() + ci * n + s * B) if s < k else (hpar.data_ptr() + (ci * p + s - k) * B)

    sn = np.tile(np.array(entries, np.int32), nch)
    bo = np.array([block_addr(ci, s) for ci in every for s in entries], np.uint64)
    av = np.array([(B - padlen if s == k - 1 else B) for _ in every for s in entries], np.uint64)
    slot0 = np.arange(nch, dtype=np.uint64) * nh

    def rchk(targets):
        d = np.zeros(nch, dtype=RCHK_DTYPE)
        d["B"], d["slot0"], d["ntargets"], d["n"], d["k"], d["m"] = B, slot0, len(targets), nh, k, m
        d["tgt0"] = np.arange(nch, dtype=np.uint64) * len(targets)
        tn = np.tile(np.array(targets, np.int32), nch)
        to = np.arange(nch * len(targets), dtype=np.uint64) * B
        return d, tn, to

    want = lost + damaged  # the pieces a caller needs back
    d1, tn1, to1 = rchk(lost)
    d2, tn2, to2 = rchk(want)
    dd = np.zeros(nch, dtype=DCHK_DTYPE)
    dd["out_off"] = np.arange(nch, dtype=np.uint64) * n
    dd["B"], dd["padlen"], dd["slot0"], dd["n"], dd["k"], dd["m"] = B, padlen, slot0, nh, k, m

    first_out = torch.zeros(max(nch * len(lost) * B, 1), dtype=torch.uint8, device="cuda:0")
    fixed = torch.zeros(nch * len(want) * B, dtype=torch.uint8, device="cuda:0")
    chunk2 = torch.zeros(nch * n, dtype=torch.uint8, device="cuda:0")
    par2 = torch.zeros(nch * p * B, dtype=torch.uint8, device="cuda:0")
    res1 = torch.zeros(16 * nch, dtype=torch.uint8, device="cuda:0")
    cres, cres2 = (torch.zeros(24 * nch, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    hits, hits2 = (torch.zeros(nch * nh, dtype=torch.int32, device="cuda:0") for _ in range(2))

    def round_one():
        eng.repair_check_batch(d1, sn, bo, 0, tn1, to1, first_out, res1, block_avail=av, asynchronous=True)

    def new():
        round_one()
        eng.repair_correct_batch(d2, sn, bo, 0, tn2, to2, fixed, cres, block_avail=av, entry_hits=hits,
                                 asynchronous=True)

    def old():
        round_one()
        eng.decode_correct_batch(dd, sn, bo, 0, chunk2, cres2, block_avail=av, entry_hits=hits2, asynchronous=True)
        eng.encode_batch(ed, chunk2, par2, asynchronous=True)

    # both routes give the source's pieces back, and report what the damage is, before anything is timed
    new()
    old()
    eng.sync()
    got = fixed.view(nch, len(want), B)
    for j, s in enumerate(want):
        if s < k and (s + 1) * B <= n:
            ref = src.view(nch, n)[:, s * B:(s + 1) * B]
        elif s < k:  # data piece k-1: its bytes, then zero padding
            ref = torch.zeros(nch, B, dtype=torch.uint8, device="cuda:0")
            ref[:, :B - padlen] = src.view(nch, n)[:, s * B:]
        else:
            ref = par.view(nch, p, B)[:, s - k]
        assert torch.equal(got[:, j], ref), f"corrected repair, piece {s}"
    assert torch.equal(chunk2, src) and torch.equal(par2, par), "decode + correct, then encode"
    for r, h in ((cres, hits), (cres2, hits2)):
        rr = np.frombuffer(r.cpu().numpy().tobytes(), dtype=COR_RESULT_DTYPE)
        assert int(rr["corrected"].sum()) == nbad_pos and int(rr["open"].sum()) == 0
        hh = h.cpu().numpy().reshape(nch, nh)
        assert all(int(hh[:, entries.index(s)].sum()) == nch * SECTOR for s in damaged) and int(hh.sum()) == nbad_pos
    first = np.frombuffer(res1.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)["first"]
    assert (first != CHK_CONSISTENT).all()

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

    kinds = {"new": ["repair_check", "decode_correct"], "old": ["repair_check", "decode_correct", "encode"]}
    samples = {name: [] for name in kinds}
    for _ in range(rounds):
        for name, fn in (("new", new), ("old", old)):
            samples[name].append(timed(fn, kinds[name]))
    one = {"read": nch * nh * B, "written": nch * len(lost) * B}
    moved = {"new": {"read": one["read"] + nch * nh * B, "written": one["written"] + nch * len(want) * B},
             "old": {"read": one["read"] + nch * nh * B + nch * k * B, "written": one["written"] + nch * m * B}}
    r = {"case": f"{nch} x {n} B zfec({k},{m}), pieces {lost} lost, a {SECTOR} B sector of piece(s) {damaged} damaged "
                 f"in every chunk, pieces {want} returned", "B": B, "held": nh, "damaged_positions": nbad_pos,
         "reps": reps}
    for name, s in samples.items():
        kernel = [sum(t.values()) for t, _ in s]
        ms = float(np.median(kernel))
        r[name] = {"bytes_read": int(moved[name]["read"]), "bytes_written": int(moved[name]["written"]),
                   "kernel_ms": round(ms, 4), "kernel_ms_rounds": [round(x, 4) for x in kernel],
                   "kernel_ms_by_kind": {kd: round(float(np.median([t[kd] for t, _ in s])), 4) for kd in kinds[name]},
                   "wall_ms": round(float(np.median([w for _, w in s])), 4),
                   "spread": round((max(kernel) - min(kernel)) / ms, 4),
                   "TBs": round((moved[name]["read"] + moved[name]["written"]) / (ms / 1e3) / 1e12, 3)}
    r["old_over_new"] = round(r["old"]["kernel_ms"] / r["new"]["kernel_ms"], 3)
    return r


def child(a):
    import torch

    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_repair_correct needs a GPU (no CPU fallback)"
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_correct_rate.json"))
    ap.add_argument("--case", help=argparse.SUPPRESS)  # child process: one case
    a = ap.parse_args()
    if a.case:
        return child(a)

    import bench

    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing), summed over a route's calls "
                     f"(new: repair_check + repair_correct; old: repair_check + decode_correct + encode; both "
                     f"correcting calls are timing kind decode_correct); wall: the host's clock around the same steps; "
                     f"median of {a.rounds} rounds of {a.reps} steps, routes interleaved per round, one untimed "
                     "lead-in step each; spread = (max - min) / median over the rounds; bytes from the shapes; one "
                     "process per case",
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
