"""CPU: the algebra behind sec_apdp_verify_batch and sec_apdp_prove_batch in pure Python ints,
against the arithmetic of oracle/apdp_ref.verify / proof, so that a change to the derivation is
not judged by the GPU alone.

verify_proof's (T^e * (F^c)^-1)^s mod n equals, mod each prime factor h of n and whenever F^c is
invertible, T^a_h * F^b_h with
    a_h = 0 if e*s == 0 else (e*s - 1) mod (h - 1) + 1       (exact for T a multiple of h too)
    b_h = (-c*s) mod (h - 1)
recombined by CRT; F^c has no inverse exactly when c != 0 and F is a multiple of p or q.
generate_proof's g_s^(c*X) equals (g_s^c)^X."""

import base64
import hashlib
import itertools
import random

import pytest

from oracle import apdp_ref

R = 1 << 2048


@pytest.fixture(scope="module")
def key():
    return apdp_ref.test_key(11)


def half_exps(e, s, c, h):
    t = e * s
    return (0 if t == 0 else (t - 1) % (h - 1) + 1), (-c * s) % (h - 1)


def joint(T, F, e, s, c, n, p, q):
    """The value the library computes, and its status."""
    if c != 0 and (F % p == 0 or F % q == 0):
        return 0, 1
    parts = []
    for h in (p, q):
        a, b = half_exps(e, s, c, h)
        assert 0 <= a < h and 0 <= b < h - 1
        parts.append(pow(T % h, a, h) * pow(F % h, b, h) % h)
    cp, cq = q * pow(q, -1, p), p * pow(p, -1, q)
    return (parts[0] * cp + parts[1] * cq) % n, 0


def oracle_tau_s(T, F, e, s, c, n):
    """apdp_ref.verify's arithmetic (its lines between the PRF and the hash); ValueError where
    pow(den, -1, n) has no inverse."""
    tau = pow(T, e, n)
    den = pow(F, c, n) % n
    tau = tau * pow(den, -1, n) % n
    return pow(tau, s, n)


def test_identity_over_edge_cases(key):
    n, e, d, p, q = key
    rng = random.Random(7)
    Ts = [rng.randrange(n), 0, 1, p * rng.randrange(1, q), q * rng.randrange(1, p), n - 1, R - 1]
    Fs = [rng.randrange(2, n), 1, n - 1, rng.getrandbits(256)]
    cs = [rng.getrandbits(256), 0, 1, (1 << 256) - 1]
    ss = [rng.randrange(2, n), 0, 1, (p - 1) * (q - 1), p - 1, R - 1]
    es = [e, 0, 3]
    count = 0
    for T, F, c, s, ee in itertools.product(Ts, Fs, cs, ss, es):
        assert joint(T, F, ee, s, c, n, p, q) == (oracle_tau_s(T, F, ee, s, c, n), 0), (T, F, c, s, ee)
        count += 1
    assert count == 7 * 4 * 4 * 6 * 3


def test_non_invertible_denominator_is_the_status(key):
    n, e, d, p, q = key
    rng = random.Random(8)
    for F in (p * rng.randrange(1, q), q * rng.randrange(1, p), 0, p, q):
        T, s = rng.randrange(n), rng.randrange(2, n)
        for c in (1, rng.getrandbits(256), (1 << 256) - 1):
            assert joint(T, F, e, s, c, n, p, q) == (0, 1)
            with pytest.raises(ValueError):
                oracle_tau_s(T, F, e, s, c, n)
        # c == 0: F^0 = 1 is invertible whatever F is
        assert joint(T, F, e, s, 0, n, p, q) == (oracle_tau_s(T, F, e, s, 0, n), 0)


def test_through_the_oracle_functions(key):
    """The same value through apdp_ref.verify itself: real PRF keys, an honest proof and a
    tampered one."""
    n, e, d, p, q = key
    rng = random.Random(9)
    g = pow(31337, 2, n)
    prf_key = b"k" * 44
    for ln in (1, 300, 9000):
        data = rng.randbytes(ln)
        tag = apdp_ref.tag_value(n, g, d, prf_key, data)
        s = rng.randrange(2, n)
        ch_key = rng.randbytes(44)
        for blob in (data, data[:-1] + bytes([data[-1] ^ 1])):
            agg_tag, agg_blocks, hashed = apdp_ref.proof(n, blob, tag, ch_key, pow(g, s, n))
            c = int.from_bytes(apdp_ref.prf(ch_key, 0), "big") % n
            F = apdp_ref.full_domain_hash(n, apdp_ref.prf(prf_key, 0))
            v, status = joint(agg_tag, F, e, s, c, n, p, q)
            assert status == 0
            mine = base64.b64encode(hashlib.sha256(apdp_ref.int_to_bytes(v)).digest()).decode()
            assert apdp_ref.verify(n, e, agg_tag, mine, ch_key, apdp_ref.prf(prf_key, 0), s)
            assert (mine == hashed) == (blob == data)


def test_rho_by_two_powers(key):
    n = key[0]
    rng = random.Random(10)
    cases = [(rng.randrange(n), rng.getrandbits(256), rng.randrange(n)) for _ in range(20)]
    cases += [(0, 0, 0), (0, 5, 0), (0, 0, 7), (1, 9, 9), (n - 1, (1 << 256) - 1, n - 1), (rng.randrange(n), 0, 5)]
    for g_s, c, X in cases:
        assert pow(pow(g_s, c, n), X, n) == pow(g_s, c * X, n)
