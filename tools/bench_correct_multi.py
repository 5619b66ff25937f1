#!/usr/bin/env python3
"""Corrected decode with several errors per byte position (sec_decode_correct_ex_batch), measured on
device-resident buffers, one process per case.  The capability is the deliverable; the figures are
recorded, no threshold is met.

  judge   the cost of the general judge where the existing one suffices: 1024 x 1 MiB RS(4,2), one
          512-byte sector of data piece 1 damaged in every chunk; max_errors = 0 (sec_decode_correct_
          ex_batch; t = 1 there) against sec_decode_correct_batch, same buffers, interleaved.
  junk2   work only this route does: 8192 x 64 KiB RS(10,4) and 128 x 8 MiB zfec(16,24) with two WHOLE
          pieces (data piece 1 and parity piece k + 1) replaced by random bytes in `--junk-every`-th
          chunks; the new call over the damaged chunks (max_errors = 0), beside the kernels of
          decode_chunks_checked's dropping rounds where those still end located: a check without the
          first named piece, a check without both (consistent), and the decode from k of the rest.
          The existing sec_decode_correct_batch reports every such position open; it is not timed.

Outputs are compared with the source before anything is timed.  Kernel times are the library's HIP
events (sec_ctx_set_timing) summed over a route's calls; every route gets an untimed lead-in step,
then `--reps` steps per round, `--rounds` rounds interleaved over the routes, median of the rounds
and (max - min) / median as spread.  The first case that fails or runs out of time ends the run.

The defaults are the run the committed profile records (5 rounds of 1 step: a junk2 step is tens of
milliseconds of kernel time, so one step per round already measures to under 1 %).

    python tools/bench_correct_multi.py [--rounds 5] [--reps 1] [--out profiles/correct_multi_rate.json]
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
    dict(name="judge_rs4_2_sector", kind="judge", nch=1024, n=1 << 20, k=4, m=6),
    dict(name="junk2_rs10_4_64KiB", kind="junk2", nch=8192, n=64 << 10, k=10, m=14),
    dict(name="junk2_zfec16_24_8MiB", kind="junk2", nch=128, n=8 << 20, k=16, m=24),
]


def run_case(eng, torch, c, rounds, reps, junk_every):
    from storb_amd._lib import CHK_CONSISTENT, CHK_DTYPE, CHK_RESULT_DTYPE, COR_RESULT_DTYPE, DCHK_DTYPE, DEC_DTYPE, ENC_DTYPE

    nch, n, k, m = c["nch"], c["n"], c["k"], c["m"]
    p = m - k
    B = -(-n // k)
    padlen = k * B - n
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2025)
    src = torch.randint(0, 256, (nch * n,), dtype=torch.uint8, device="cuda:0", generator=g)
    par = torch.empty(nch * p * B, dtype=torch.uint8, device="cuda:0")
    ed = np.zeros(nch, dtype=ENC_DTYPE)
    ed["in_off"] = np.arange(nch, dtype=np.uint64) * n
    ed["n"], ed["parity_stride"], ed["k"], ed["m"] = n, B, k, m
    ed["parity_off"] = np.arange(nch, dtype=np.uint64) * (p * B)
    eng.encode_batch(ed, src, par)

    held, hpar = src.clone(), par.clone()  # the pieces as held; src stays the reference
    junk = c["kind"] == "junk2"
    bad = list(range(0, nch, junk_every if junk else 1))
    damaged = [1, k + 1] if junk else [1]
    nbad_pos = 0
    for ci in bad:
        o = ci * n + B
        if not junk:
            at = (ci * 7919) % (B - SECTOR)
            held[o + at:o + at + SECTOR] ^= 0xA5
            nbad_pos += SECTOR
            continue
        q = (ci * p + 1) * B
        j1 = torch.randint(0, 256, (B,), dtype=torch.uint8, device="cuda:0", generator=g)
        j2 = torch.randint(0, 256, (B,), dtype=torch.uint8, device="cuda:0", generator=g)
        nbad_pos += int(((j1 != held[o:o + B]) | (j2 != hpar[q:q + B])).sum())
        held[o:o + B] = j1
        hpar[q:q + B] = j2
    nb = len(bad)

    def block_addr(ci, s):
        return (held.data_ptr() + ci * n + s * B) if s < k else (hpar.data_ptr() + (ci * p + s - k) * B)

    def arrays(entries):
        sn = np.tile(np.array(entries, np.int32), nb)
        bo = np.array([block_addr(ci, s) for ci in bad for s in entries], np.uint64)
        av = np.array([(B - padlen if s == k - 1 else B) for _ in bad for s in entries], np.uint64)
        return len(entries), sn, bo, av, np.arange(nb, dtype=np.uint64) * len(entries)

    def dchk(nh, slot0):
        d = np.zeros(nb, dtype=DCHK_DTYPE)
        d["out_off"] = np.array(bad, dtype=np.uint64) * n
        d["B"], d["padlen"], d["slot0"], d["n"], d["k"], d["m"] = B, padlen, slot0, nh, k, m
        return d

    nh, sn, bo, av, slot0 = arrays(list(range(m)))
    cor = dchk(nh, slot0)
    out = {name: torch.zeros(nch * n, dtype=torch.uint8, device="cuda:0") for name in ("ex", "other")}
    cres = {name: torch.zeros(24 * nb, dtype=torch.uint8, device="cuda:0") for name in ("ex", "other")}
    hits = {name: torch.zeros(nb * m, dtype=torch.int32, device="cuda:0") for name in ("ex", "other")}

    def ex():
        eng.decode_correct_batch(cor, sn, bo, 0, out["ex"], cres["ex"], block_avail=av, entry_hits=hits["ex"],
                                 asynchronous=True, max_errors=0)

    routes, kinds = {"ex": ex}, {"ex": ["decode_correct"]}
    if not junk:
        def one():
            eng.decode_correct_batch(cor, sn, bo, 0, out["other"], cres["other"], block_avail=av,
                                     entry_hits=hits["other"], asynchronous=True)

        routes["one"], kinds["one"] = one, ["decode_correct"]
    else:
        # the dropping rounds that still end located: without piece 1 (inconsistent: names k + 1), without
        # both (consistent), then the decode from k of the rest
        rest1 = [s for s in range(m) if s != 1]
        rest1 = [s for s in rest1 if s != k][:k - 1] + [k] + [s for s in rest1 if s > k]  # parity k stands in for 1
        rest2 = [s for s in rest1 if s != k + 1]
        a1, a2 = arrays(rest1), arrays(rest2)
        cds = []
        for a in (a1, a2):
            cd = np.zeros(nb, dtype=CHK_DTYPE)
            cd["B"], cd["slot0"], cd["n"], cd["k"], cd["m"] = B, a[4], a[0], k, m
            cds.append(cd)
        dd = np.zeros(nb, dtype=DEC_DTYPE)
        dd["out_off"] = np.array(bad, dtype=np.uint64) * n
        dd["B"], dd["padlen"], dd["slot0"], dd["k"], dd["m"] = B, padlen, a2[4], k, m
        r1, r2 = (torch.zeros(16 * nb, dtype=torch.uint8, device="cuda:0") for _ in range(2))

        def dropping():
            eng.check_batch(cds[0], a1[1], a1[2], 0, r1, block_avail=a1[3], asynchronous=True)
            eng.check_batch(cds[1], a2[1], a2[2], 0, r2, block_avail=a2[3], asynchronous=True)
            eng.decode_batch(dd, a2[1], a2[2], 0, out["other"], block_avail=a2[3], asynchronous=True)

        routes["dropping"], kinds["dropping"] = dropping, ["check", "decode"]

    # every route gives the source back and reports the damage put in, before anything is timed
    for fn in routes.values():
        fn()
    eng.sync()
    sel = torch.zeros(nch, dtype=torch.bool, device="cuda:0")
    sel[bad] = True
    want = src.view(nch, n)[sel]
    for name in ("ex", "other"):
        assert torch.equal(out[name].view(nch, n)[sel], want), name
    names = ["ex"] + (["other"] if not junk else [])
    for name in names:
        got = np.frombuffer(cres[name].cpu().numpy().tobytes(), dtype=COR_RESULT_DTYPE)
        assert int(got["corrected"].sum()) == nbad_pos and int(got["open"].sum()) == 0, name
        h = hits[name].cpu().numpy().reshape(nb, m)
        assert not h[:, [s for s in range(m) if s not in damaged]].any() and h[:, damaged].all(), name
    if junk:
        first = [np.frombuffer(r.cpu().numpy().tobytes(), dtype=CHK_RESULT_DTYPE)["first"] for r in (r1, r2)]
        assert (first[0] != CHK_CONSISTENT).all() and (first[1] == CHK_CONSISTENT).all()

    def timed(fn, kd):
        fn()  # untimed lead-in: plans cached
        eng.sync()
        eng.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        eng.sync()
        wall = (time.perf_counter() - t0) * 1e3 / reps
        eng.set_timing(False)
        return {q: eng.collect_timing(q)[0] / reps for q in kd}, wall

    samples = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            samples[name].append(timed(fn, kinds[name]))
    r = {"case": f"{nch} x {n} B zfec({k},{m}), every piece held, " +
                 (f"pieces {damaged} whole junk" if junk else f"a {SECTOR} B sector of data piece 1 damaged") +
                 f" in {nb} chunk(s)", "B": B, "damaged_chunks": nb, "damaged_positions": nbad_pos, "reps": reps}
    for name, s in samples.items():
        kernel = [sum(t.values()) for t, _ in s]
        ms = float(np.median(kernel))
        r[name] = {"kernel_ms": round(ms, 4), "kernel_ms_rounds": [round(x, 4) for x in kernel],
                   "kernel_ms_by_kind": {q: round(float(np.median([t[q] for t, _ in s])), 4) for q in kinds[name]},
                   "wall_ms": round(float(np.median([w for _, w in s])), 4),
                   "spread": round((max(kernel) - min(kernel)) / ms, 4)}
    other = "one" if not junk else "dropping"
    r[f"ex_over_{other}"] = round(r["ex"]["kernel_ms"] / r[other]["kernel_ms"], 3)
    r["ex_us_per_damaged_position"] = round(r["ex"]["kernel_ms"] * 1e3 / max(nbad_pos, 1), 6)
    return r


def child(a):
    import torch

    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_correct_multi needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    eng = Engine(0)
    c = next(c for c in CASES if c["name"] == a.case)
    r = run_case(eng, torch, c, a.rounds, a.reps, a.junk_every)
    eng.close()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--junk-every", type=int, default=1, help="junk2: every how many-th chunk is damaged")
    ap.add_argument("--only", default="", help="comma list of case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_multi_rate.json"))
    ap.add_argument("--case", help=argparse.SUPPRESS)  # child process: one case
    a = ap.parse_args()
    if a.case:
        return child(a)

    import bench

    res = {"method": f"HIP events: the library's per-launch ones (sec_ctx_set_timing), summed over a route's calls; "
                     f"wall: the host's clock around the same steps; median of {a.rounds} rounds of {a.reps} steps, "
                     "routes interleaved per round, one untimed lead-in step each; spread = (max - min) / median over "
                     f"the rounds; one process per case; junk2: every {a.junk_every}-th chunk damaged",
           "lib_digest": bench.lib_digest(), "cases": {}}
    for c in CASES:
        if a.only and c["name"] not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", c["name"], "--rounds", str(a.rounds), "--reps",
               str(a.reps), "--junk-every", str(a.junk_every)]
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
