#!/usr/bin/env python3
"""The tagged encode (sec_encode_tag_batch, sec_encode_pieces_tags) against the calls it replaces,
on the same buffers in one process.  Three routes per shape, `old` being the library's calls
before the tagged encode existed:

  host    old  sec_encode_digest_batch(HOST) + sec_apdp_tag_batch(HOST) over all m pieces
          new  sec_encode_tag_batch(HOST) with digests
  pieces  old  sec_encode_pieces with ids + sec_apdp_tag_batch(HOST) over the new pieces
          new  sec_encode_pieces_tags
  device  old  sec_encode_digest_batch + sec_apdp_tag_batch on device-resident buffers
          new  sec_encode_tag_batch on the same buffers (the same kernels: expected level; the
               sanity check of the other two routes)

Shapes: 1024 x 1 MiB RS(4,2), 128 x 8 MiB zfec(16,24), and one 8 MiB zfec(16,24) chunk per call
(the validator's granularity).  Every schedule gets 2 untimed lead-in steps, then `--reps` steps
per round, `--rounds` rounds interleaved over old / new, median of the rounds.  Recorded per
schedule: wall time per step, the library's kernel times (sec_ctx_set_timing) of kind 0 (encode;
a staged host call does not time its encode kernels, so 0 there), kind 2 (SHA-1 calls) and kind 3
(bignum: the tag kernels), and the bytes staged host-to-device, from the shapes.  The key is a
fixed test key with CRT.  Each (shape, route) runs in a child process of its own under a time
limit; the first one that fails ends the run.

    python tools/bench_upload_tags.py [--rounds 5] [--reps 10] [--out profiles/upload_tags_rate.json]
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

CASE_TIMEOUT_S = 400
PRF_KEY = b"prf-key-for-bench-0123456789abcdef0123456789="

SHAPES = [
    dict(name="c2_rs4_2", nch=1024, n=1 << 20, k=4, m=6),
    dict(name="zfec16_24_8MiB", nch=128, n=8 << 20, k=16, m=24),
    dict(name="one_8MiB_chunk", nch=1, n=8 << 20, k=16, m=24),
]
ROUTES = ["host", "pieces", "device"]


def make_key(eng):
    from oracle import apdp_ref
    from storb_amd import bn

    n, e, d, p, q = apdp_ref.test_key(11)
    mk = bn.ModKey(n, eng)
    mk.set_crt(p, q)
    mk.set_tag(pow(31337, 2, n), apdp_ref.full_domain_hash(n, apdp_ref.prf(PRF_KEY, 0)), d)
    return mk


def run_case(eng, torch, c, route, rounds, reps):
    from storb_amd._lib import ENC_DTYPE, MSG_DTYPE

    nch, n, k, m = c["nch"], c["n"], c["k"], c["m"]
    p, B = m - k, -(-n // k)
    mk = make_key(eng)
    rng = np.random.default_rng(2024)
    host_src = rng.integers(0, 256, nch * n, dtype=np.uint8)
    ed = np.zeros(nch, dtype=ENC_DTYPE)
    ed["in_off"] = np.arange(nch, dtype=np.uint64) * n
    ed["n"], ed["parity_stride"], ed["k"], ed["m"] = n, B, k, m
    ed["parity_off"] = np.arange(nch, dtype=np.uint64) * (p * B)
    nslots = nch * m

    def block_msgs(src_addr, par_addr):  # the chunks' m blocks as messages, slot order
        msgs = np.zeros((nch, m), dtype=MSG_DTYPE)
        ci = np.arange(nch, dtype=np.uint64)[:, None]
        j = np.arange(k, dtype=np.uint64)[None, :]
        msgs["addr"][:, :k] = src_addr + ci * n + j * B
        msgs["len"][:, :] = B
        msgs["avail"][:, :k] = np.minimum(B, n - j.astype(np.int64) * B)
        r = np.arange(p, dtype=np.uint64)[None, :]
        msgs["addr"][:, k:] = par_addr + (ci * p + r) * B
        msgs["avail"][:, k:] = B
        return msgs.reshape(-1)

    if route == "device":
        src = torch.from_numpy(host_src).to("cuda:0")
        par, par2 = (torch.empty(max(nch * p * B, 1), dtype=torch.uint8, device="cuda:0") for _ in range(2))
        dig, dig2 = (torch.zeros(20 * nslots, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        tags, tags2 = (torch.zeros(256 * nslots, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        msgs = block_msgs(src.data_ptr(), par2.data_ptr())

        def new():
            eng.encode_tag_batch(ed, src, par, tags, mk, digests=dig, asynchronous=True)
            eng.sync()

        def old():
            eng.encode_digest_batch(ed, src, par2, dig2, asynchronous=True)
            mk.tag_batch(msgs, tags2, asynchronous=True)
            eng.sync()

        def same():
            return torch.equal(par, par2) and torch.equal(dig, dig2) and torch.equal(tags, tags2)

        staged = {"old": 0, "new": 0}
    elif route == "host":
        par, par2 = (np.empty(max(nch * p * B, 1), np.uint8) for _ in range(2))
        dig, dig2 = (np.zeros(20 * nslots, np.uint8) for _ in range(2))
        tags, tags2 = (np.zeros(256 * nslots, np.uint8) for _ in range(2))
        msgs = block_msgs(host_src.ctypes.data, par2.ctypes.data)

        def new():
            eng.encode_tag_batch(ed, host_src, par, tags, mk, digests=dig, host=True)

        def old():
            eng.encode_digest_batch(ed, host_src, par2, dig2, host=True)
            mk.tag_batch(msgs, tags2, host=True)

        def same():
            return (par == par2).all() and (dig == dig2).all() and (tags == tags2).all()

        staged = {"old": nch * n + int(msgs["avail"].sum()), "new": nch * n}
    else:  # pieces: every piece in a buffer of its own
        chunks = [host_src[i * n:(i + 1) * n] for i in range(nch)]
        shapes = [(k, m)] * nch
        bufs, bufs2 = ([np.empty(B, np.uint8) for _ in range(nslots)] for _ in range(2))
        addrs, addrs2 = ([b.ctypes.data for b in bs] for bs in (bufs, bufs2))
        dig, dig2 = (np.zeros(20 * nslots, np.uint8) for _ in range(2))
        tags, tags2 = (np.zeros(256 * nslots, np.uint8) for _ in range(2))
        msgs = np.zeros(nslots, dtype=MSG_DTYPE)
        msgs["addr"], msgs["len"], msgs["avail"] = addrs2, B, B

        def new():
            eng.encode_pieces_into(chunks, shapes, addrs, dig, staged=True, tags=tags, tag_key=mk)

        def old():
            eng.encode_pieces_into(chunks, shapes, addrs2, dig2, staged=True)
            mk.tag_batch(msgs, tags2, host=True)

        def same():
            return (all((a == b).all() for a, b in zip(bufs, bufs2)) and (dig == dig2).all()
                    and (tags == tags2).all())

        staged = {"old": nch * n + nslots * B, "new": nch * n}

    new()
    old()
    assert same(), "the fused call and the calls it replaces disagree"

    kinds = ["encode", "sha1", "bignum"]

    def timed(fn):
        for _ in range(2):  # untimed lead-in: plans cached, pinned slabs in the pool
            fn()
        eng.sync()
        eng.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        eng.sync()
        wall = (time.perf_counter() - t0) / reps * 1e3
        eng.set_timing(False)
        return [wall] + [eng.collect_timing(kd)[0] / reps for kd in kinds]

    samples = {"old": [], "new": []}
    for _ in range(rounds):
        for name, fn in (("old", old), ("new", new)):
            samples[name].append(timed(fn))
    out = {"case": f"{nch} x {n} B zfec({k},{m}), route {route}", "B": B, "tags_per_step": nslots,
           "piece_bytes_per_step": nslots * B}
    for name, rows in samples.items():
        a = np.array(rows)
        med = np.median(a, axis=0)
        wall = float(med[0])
        out[name] = {"wall_ms": round(wall, 3), "wall_ms_rounds": [round(float(x), 3) for x in a[:, 0]],
                     "spread": round(float((a[:, 0].max() - a[:, 0].min()) / wall), 4),
                     "kernel_ms_kind0_encode": round(float(med[1]), 4), "kernel_ms_kind2_sha1": round(float(med[2]), 4),
                     "kernel_ms_kind3_bignum": round(float(med[3]), 4), "bytes_staged_h2d": int(staged[name]),
                     "pieces_GBs": round(nslots * B / (wall / 1e3) / 1e9, 2),
                     "tags_per_s": round(nslots / (wall / 1e3), 1)}
    out["old_over_new_wall"] = round(out["old"]["wall_ms"] / out["new"]["wall_ms"], 3)
    if staged["new"]:
        out["old_over_new_bytes_staged"] = round(staged["old"] / staged["new"], 3)
    mk.close()
    return out


def child(a):
    import torch

    from storb_amd.engine import Engine

    assert torch.cuda.is_available(), "bench_upload_tags needs a GPU (no CPU fallback)"
    torch.cuda.set_device(0)
    eng = Engine(0)
    shape, route = a.case.split(":")
    c = next(c for c in SHAPES if c["name"] == shape)
    r = run_case(eng, torch, c, route, a.rounds, a.reps)
    eng.close()
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of shape names (default: all)")
    ap.add_argument("--box", default="", help="a note on the machine the numbers come from, kept in the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upload_tags_rate.json"))
    ap.add_argument("--case", help=argparse.SUPPRESS)  # child process: one shape:route
    a = ap.parse_args()
    if a.case:
        return child(a)

    import bench

    res = {"method": f"wall time per step around the synchronous calls (device route: the calls, then sec_sync); "
                     f"kernel times from sec_ctx_set_timing; median of {a.rounds} rounds of {a.reps} steps, old / new "
                     "interleaved per round, 2 untimed lead-in steps each; spread = (max - min) / median of the wall "
                     "times over the rounds; bytes staged from the shapes; one process per shape and route",
           "box": a.box, "lib_digest": bench.lib_digest(), "cases": {}}
    for c in SHAPES:
        if a.only and c["name"] not in a.only.split(","):
            continue
        for route in ROUTES:
            case = f"{c['name']}:{route}"
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--rounds", str(a.rounds), "--reps",
                   str(a.reps)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                sys.exit(f"{case}: no result within {CASE_TIMEOUT_S} s; nothing more is started")
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(f"{case}: exit status {p.returncode}; nothing more is started")
            res["cases"][case] = json.loads(line[len("RESULT "):])
            print(json.dumps({case: res["cases"][case]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
