#!/usr/bin/env python3
"""The one-call challenge round (sec_apdp_prove_batch, sec_apdp_verify_batch over
sec_bn_crt_modexp2_batch) against the routes it replaces, which stay callable in the same
library: the same buffers, old and new interleaved, median of `--rounds` rounds.

  verify_kernels   16384 verifications, device-resident operands, exponents derived beforehand:
                   old  crt_modexp (T^e, F^c) + crt_modexp (Fermat inverse) + 2 mulmod + crt_modexp (^s)
                   new  one crt_modexp2 launch
  prove_kernels    4096 proofs of 256 KiB pieces, device-resident:
                   old  reduce + modexp (T^c and g_s^(c X) with 288-byte exponents, formed beforehand)
                   new  prove
  drop_in          ChallengeSystem.generate_proofs / verify_proofs on 1024 items of 256 KiB from
                   host memory: old = the compositions over ModKey.reduce / powmod / crt_powmod /
                   mulmod that apdp.py held before (restated below), new = the methods themselves
  batch_of_1       the same two methods on one item, where the number of launches matters

Kernel times are the library's (sec_ctx_set_timing, kind 3), wall times a host clock around calls
that end in a synchronise.  Every schedule gets one untimed lead-in step per round.  The old and
new results are compared before anything is timed.

    python tools/bench_apdp_round.py [--rounds 5] [--out profiles/apdp_round_rate.json]
"""

from __future__ import annotations

import argparse
import base64
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRF_KEY = b"prf-key-for-bench-0123456789abcdef0123456789="


# ---- the routes apdp.py took before the one-call round ----------------------------------------
def old_generate_proofs(cs, items, n):
    from storb_amd.apdp import CryptoUtils, Proof, _fit, int_to_bytes

    mk = cs._modkey(n)
    xs = mk.reduce([d for d, _, _ in items])
    coefs = [int.from_bytes(CryptoUtils.prf(ch.prf_key, 0), "big") % n for _, _, ch in items]
    aggs = [c * x for c, x in zip(coefs, xs)]
    res = mk.powmod([_fit(t.tag_value, n) for _, t, _ in items] + [_fit(ch.g_s, n) for _, _, ch in items],
                    coefs + aggs)
    k = len(items)
    return [Proof(tag_value=res[i], block_value=aggs[i],
                  hashed_result=base64.b64encode(hashlib.sha256(int_to_bytes(res[k + i])).digest()).decode("utf-8"))
            for i in range(k)]


def old_verify_proofs(cs, items, n, e):
    from storb_amd.apdp import CryptoUtils, _fit, int_to_bytes

    rsa_key = cs.key.rsa
    priv = rsa_key.private_numbers()
    mk = cs._modkey(n)
    k = len(items)
    coefs = [int.from_bytes(CryptoUtils.prf(ch.prf_key, 0), "big") % n for _, ch, _ in items]
    fdhs = [CryptoUtils.full_domain_hash(rsa_key, t.prf_value) for _, _, t in items]
    r1 = mk.crt_powmod([_fit(p.tag_value, n) for p, _, _ in items] + fdhs, [e] * k + coefs)
    taus, dens = r1[:k], r1[k:]
    invs = mk.crt_powmod_pq(dens, [priv.p - 2] * k, [priv.q - 2] * k)
    r2 = mk.mulmod(dens + taus, invs + invs)
    assert all(v == 1 for v in r2[:k])
    tau_s = mk.crt_powmod(r2[k:], [ch.s for _, ch, _ in items])
    return [base64.b64encode(hashlib.sha256(int_to_bytes(v)).digest()).decode("utf-8") == proof.hashed_result
            for (proof, _, _), v in zip(items, tau_s)]


# ---- timing -------------------------------------------------------------------------------------
def timed(eng, fn, reps):
    fn()  # untimed lead-in
    eng.sync()
    eng.collect_timing("bignum")
    eng.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    eng.sync()
    wall = (time.perf_counter() - t0) / reps * 1e3
    eng.set_timing(False)
    return wall, eng.collect_timing("bignum")[0] / reps


def compare(eng, old, new, rounds, reps, items):
    samples = {"old": [], "new": []}
    for _ in range(rounds):
        for name, fn in (("old", old), ("new", new)):
            samples[name].append(timed(eng, fn, reps))
    out = {"items": items, "reps_per_round": reps}
    for name, rows in samples.items():
        a = np.array(rows)
        wall, kern = (float(x) for x in np.median(a, axis=0))
        out[name] = {"wall_ms": round(wall, 4), "kernel_ms": round(kern, 4),
                     "wall_ms_rounds": [round(float(x), 4) for x in a[:, 0]],
                     "kernel_ms_rounds": [round(float(x), 4) for x in a[:, 1]],
                     "wall_spread": round(float((a[:, 0].max() - a[:, 0].min()) / wall), 4),
                     "kernel_spread": round(float((a[:, 1].max() - a[:, 1].min()) / kern), 4) if kern else None,
                     "items_per_s_wall": round(items / wall * 1e3, 1)}
    out["old_over_new_wall"] = round(out["old"]["wall_ms"] / out["new"]["wall_ms"], 3)
    if out["new"]["kernel_ms"]:
        out["old_over_new_kernel"] = round(out["old"]["kernel_ms"] / out["new"]["kernel_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--verifies", type=int, default=16384)
    ap.add_argument("--proofs", type=int, default=4096)
    ap.add_argument("--piece-bytes", type=int, default=262144)
    ap.add_argument("--api-items", type=int, default=1024)
    ap.add_argument("--box", default="", help="a note on the machine the numbers come from, kept in the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apdp_round_rate.json"))
    a = ap.parse_args()

    import torch

    import bench
    from oracle import apdp_ref
    from storb_amd import apdp, bn
    from storb_amd._lib import MSG_DTYPE
    from storb_amd.engine import get_engine

    assert torch.cuda.is_available(), "bench_apdp_round needs a GPU (no CPU fallback)"
    eng = get_engine(0)
    n, e, d, p, q = apdp_ref.test_key(11)
    g = pow(31337, 2, n)
    half = bn.ModKey._half_exp
    rng = random.Random(2025)
    dev = lambda rows: torch.from_numpy(rows).cuda()  # noqa: E731
    buf = lambda rows: torch.empty(rows * 256, dtype=torch.uint8, device="cuda")  # noqa: E731
    res = {"method": f"median of {a.rounds} rounds, old / new interleaved per round, one untimed lead-in step "
                     "each; kernel_ms from sec_ctx_set_timing kind 3 per step, wall_ms a host clock around the "
                     "step and its synchronise; spread = (max - min) / median over the rounds; one process",
           "box": a.box, "lib_digest": bench.lib_digest(), "cases": {}}

    # -- verify kernels --------------------------------------------------------------------------
    mc = bn.ModKey(n, eng)
    mc.set_crt(p, q)
    V = a.verifies
    T = [rng.randrange(n) for _ in range(V)]
    F = [rng.randrange(2, n) for _ in range(V)]
    c = [rng.getrandbits(256) for _ in range(V)]
    s = [rng.randrange(2, n) for _ in range(V)]
    # old: the four calls' operands, exponents reduced per factor as crt_powmod does (width: the
    # widest of e and c, 32 bytes; 128 for the inverse and the s power)
    tf = dev(bn.to_be(T + F))
    e1p = dev(bn.to_be([half(e, p - 1)] * V + [half(x, p - 1) for x in c], 32))
    e1q = dev(bn.to_be([half(e, q - 1)] * V + [half(x, q - 1) for x in c], 32))
    ip, iq = dev(bn.to_be([p - 2] * V, 128)), dev(bn.to_be([q - 2] * V, 128))
    sp, sq = dev(bn.to_be([half(x, p - 1) for x in s], 128)), dev(bn.to_be([half(x, q - 1) for x in s], 128))
    r1, invs, chk, tau, old_out = buf(2 * V), buf(V), buf(V), buf(V), buf(V)

    def old_verify():
        # the composition made one 2V-item mulmod; two V-item ones here, so that no copy of the
        # inverses is needed on the device (the same products, one more launch)
        mc.crt_modexp_batch(tf, e1p, e1q, 32, 2 * V, r1, asynchronous=True)
        mc.crt_modexp_batch(r1[V * 256:], ip, iq, 128, V, invs, asynchronous=True)
        mc.mulmod_batch(r1[V * 256:], invs, V, chk, asynchronous=True)
        mc.mulmod_batch(r1, invs, V, tau, asynchronous=True)
        mc.crt_modexp_batch(tau, sp, sq, 128, V, old_out, asynchronous=True)
        eng.sync()

    # new: the exponents sec_apdp_verify_batch derives, formed beforehand as well
    ta, fb = dev(bn.to_be(T)), dev(bn.to_be(F))
    ex = [dev(bn.to_be([f(x, y, m) for x, y in zip(c, s)], 128))
          for f in (lambda x, y, m: half(e * y, m), lambda x, y, m: (-x * y) % m) for m in (p - 1, q - 1)]
    new_out = buf(V)

    def new_verify():
        mc.crt_modexp2_batch(ta, fb, *ex, 128, V, new_out, asynchronous=True)
        eng.sync()

    old_verify()
    new_verify()
    assert torch.equal(old_out, new_out), "the one-launch verify and the four calls disagree"
    assert bn.from_be(new_out[:256].cpu().numpy())[0] == pow(pow(T[0], e, n) * pow(pow(F[0], c[0], n), -1, n) % n,
                                                             s[0], n)
    res["cases"]["verify_kernels"] = compare(eng, old_verify, new_verify, a.rounds, 3, V)
    print(json.dumps({"verify_kernels": res["cases"]["verify_kernels"]}), flush=True)
    del tf, e1p, e1q, ip, iq, sp, sq, r1, invs, chk, tau, ta, fb, ex

    # -- prove kernels ---------------------------------------------------------------------------
    mk = bn.ModKey(n, eng)  # the miner: the modulus alone
    P, L = a.proofs, a.piece_bytes
    src = torch.randint(0, 256, (P * L,), dtype=torch.uint8, device="cuda")
    msgs = np.zeros(P, dtype=MSG_DTYPE)
    msgs["addr"] = src.data_ptr() + np.arange(P, dtype=np.uint64) * L
    msgs["len"] = msgs["avail"] = L
    tags = [rng.randrange(n) for _ in range(P)]
    g_ss = [rng.randrange(n) for _ in range(P)]
    coefs = [rng.getrandbits(256) for _ in range(P)]
    xs_d = buf(P)
    mk.reduce_batch(msgs, xs_d)
    xs = bn.from_be(xs_d.cpu().numpy())
    bases = dev(bn.to_be(tags + g_ss))
    exps = dev(bn.to_be(coefs + [x * y for x, y in zip(coefs, xs)], 288))
    old_res = buf(2 * P)

    def old_prove():
        mk.reduce_batch(msgs, xs_d, asynchronous=True)
        mk.modexp_batch(bases, exps, 288, 2 * P, old_res, asynchronous=True)
        eng.sync()

    dt, dg, dc = dev(bn.to_be(tags)), dev(bn.to_be(g_ss)), dev(bn.to_be(coefs, 32))
    tag_c, rho = buf(P), buf(P)
    block = torch.empty(P * 288, dtype=torch.uint8, device="cuda")

    def new_prove():
        mk.prove_batch(msgs, dt, dg, dc, tag_c, block, rho, asynchronous=True)
        eng.sync()

    old_prove()
    new_prove()
    assert torch.equal(old_res[:P * 256], tag_c) and torch.equal(old_res[P * 256:], rho)
    assert torch.equal(block, exps.reshape(-1)[P * 288:]), "c * X from the kernel and from Python ints disagree"
    res["cases"]["prove_kernels"] = compare(eng, old_prove, new_prove, a.rounds, 2, P)
    res["cases"]["prove_kernels"]["piece_bytes"] = L
    print(json.dumps({"prove_kernels": res["cases"]["prove_kernels"]}), flush=True)
    del src, bases, exps, old_res, dt, dg, dc, tag_c, rho, block

    # -- the drop-in methods, host memory --------------------------------------------------------
    cs = apdp.ChallengeSystem()
    cs.key.rsa = apdp.RSAPrivateKey(p, q, e)
    cs.key.g = g
    cs.key.prf_key = PRF_KEY
    K = a.api_items
    datas = [os.urandom(L) for _ in range(K)]
    tg = cs.generate_tags(datas)
    chs = cs.issue_challenges(tg)
    pitems = list(zip(datas, tg, chs))
    proofs = cs.generate_proofs(pitems, n)
    assert proofs == old_generate_proofs(cs, pitems, n)
    vitems = list(zip(proofs, chs, tg))
    assert cs.verify_proofs(vitems, n, e) == old_verify_proofs(cs, vitems, n, e) == [True] * K
    for label, k, reps in (("drop_in", K, 1), ("batch_of_1", 1, 20)):
        res["cases"][f"{label}_generate_proofs"] = compare(
            eng, lambda: old_generate_proofs(cs, pitems[:k], n), lambda: cs.generate_proofs(pitems[:k], n),
            a.rounds, reps, k)
        res["cases"][f"{label}_verify_proofs"] = compare(
            eng, lambda: old_verify_proofs(cs, vitems[:k], n, e), lambda: cs.verify_proofs(vitems[:k], n, e),
            a.rounds, reps, k)
        for case in ("generate_proofs", "verify_proofs"):
            print(json.dumps({f"{label}_{case}": res["cases"][f"{label}_{case}"]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
