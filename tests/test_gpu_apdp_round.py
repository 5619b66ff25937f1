"""GPU: the challenge round's one-call prove and verify (sec_apdp_prove_batch,
sec_apdp_verify_batch) and the double-exponentiation call under verify (sec_bn_crt_modexp2_batch),
against Python ints and oracle/apdp_ref.py; then storb_amd.apdp.ChallengeSystem through them.

Sizes are the smallest at which the kernels take another path: exponent widths of 1, 3, 128, 256
and 288 bytes, counts of 1, 2 and 67 blocks, messages of one, two and several 8 KiB segments with
ragged heads, and operands that drive c * X's carries through all 72 limbs."""

import base64
import hashlib
import random

import numpy as np
import pytest

from oracle import apdp_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from storb_amd import _lib, apdp, bn  # noqa: E402
from storb_amd._lib import MSG_DTYPE  # noqa: E402
from storb_amd.engine import ECRuntimeError  # noqa: E402

R = 1 << 2048
C_MAX = (1 << 256) - 1


@pytest.fixture(scope="module")
def key():
    return apdp_ref.test_key(11)


@pytest.fixture(scope="module")
def mk(key, engine):
    """The miner's key: the modulus alone."""
    return bn.ModKey(key[0], engine)


@pytest.fixture(scope="module")
def mk_crt(key, engine):
    """The validator's key: with its factors."""
    k = bn.ModKey(key[0], engine)
    k.set_crt(key[3], key[4])
    return k


def b64sha(x: int) -> str:
    return base64.b64encode(hashlib.sha256(apdp_ref.int_to_bytes(x)).digest()).decode()


# ---- sec_bn_crt_modexp2_batch -----------------------------------------------------------------
def modexp2(mk_crt, a, b, ea, eb, width, device=False):
    """The raw call at an explicit exponent width.  Width 128 takes the exponents reduced per
    factor, any other width the exponents themselves (congruent to themselves, nonzero when they
    are): the kernel then walks all 8 * width bits."""
    p, q = mk_crt.p, mk_crt.q
    red = (lambda e, m: bn.ModKey._half_exp(e, m)) if width == 128 else (lambda e, m: e)
    ins = [bn.to_be(a), bn.to_be(b)] + [bn.to_be([red(e, m) for e in es], width)
                                        for es in (ea, eb) for m in (p - 1, q - 1)]
    if device:
        ins = [torch.from_numpy(x).cuda() for x in ins]
        out = torch.empty(len(a) * 256, dtype=torch.uint8, device="cuda")
        mk_crt.crt_modexp2_batch(*ins, width, len(a), out)
        return bn.from_be(out.cpu().numpy())
    out = np.empty((len(a), 256), np.uint8)
    mk_crt.crt_modexp2_batch(*ins, width, len(a), out, host=True)
    return bn.from_be(out)


def want2(n, a, b, ea, eb):
    return [pow(x, s, n) * pow(y, t, n) % n for x, y, s, t in zip(a, b, ea, eb)]


def joint_digits(ea: int, eb: int) -> list:
    """The (i, j) 2-bit digit pairs of the two exponents, least significant first."""
    out = []
    while ea or eb:
        out.append((ea & 3, eb & 3))
        ea >>= 2
        eb >>= 2
    return out


@pytest.mark.parametrize("width", [1, 3, 128, 256, 288])
def test_crt_powmod2_widths_and_edge_operands(mk_crt, key, width):
    n, e, d, p, q = key
    rng = random.Random(100 + width)
    top = (1 << (8 * width)) - 1 if width != 128 else R - 1  # width 128: reduced from up to 2048 bits
    bases = [rng.randrange(R), 0, 1, n, n + 1, R - 1, n - 1, p * rng.randrange(1, q), q * rng.randrange(1, p),
             p, 2 * q, rng.randrange(n)]
    a = bases + bases[::-1] + [rng.randrange(R) for _ in range(4)]
    b = bases[3:] + bases[:3] + bases + [rng.randrange(R) for _ in range(4)]
    ea = [rng.randrange(top + 1) for _ in a]
    eb = [rng.randrange(top + 1) for _ in a]
    ea[:6] = [0, rng.randrange(1, top + 1), 0, top, top, 1]
    eb[:6] = [rng.randrange(1, top + 1), 0, 0, top, 1, top]
    assert modexp2(mk_crt, a, b, ea, eb, width) == want2(n, a, b, ea, eb)


@pytest.mark.parametrize("count", [1, 2, 67])
def test_crt_powmod2_counts(mk_crt, key, count):
    n = key[0]
    rng = random.Random(count)
    a, b = ([rng.randrange(R) for _ in range(count)] for _ in range(2))
    ea, eb = ([rng.getrandbits(2048) for _ in range(count)] for _ in range(2))
    want = want2(n, a, b, ea, eb)
    assert mk_crt.crt_powmod2(a, b, ea, eb) == want
    assert modexp2(mk_crt, a, b, ea, eb, 128, device=True) == want


def test_crt_powmod2_window_shapes(mk_crt, key):
    n, e, d, p, q = key
    rng = random.Random(31)
    # every one of the 16 table entries, twice over: once as the leading pair's pick or a
    # product, then as a product
    every_a = sum((k // 4) << (2 * k) for k in range(16))
    every_b = sum((k % 4) << (2 * k) for k in range(16))
    every_a |= every_a << 32
    every_b |= every_b << 32
    assert {(i, j) for i in range(4) for j in range(4)} == set(joint_digits(every_a, every_b))
    assert len(joint_digits(every_a, every_b)) == 32
    # long interior runs of (0, 0) pairs
    runs_a = (1 << 1000) | (1 << 500) | 1
    runs_b = (1 << 1001) | (1 << 3)
    pairs = joint_digits(runs_a, runs_b)
    assert max(len(run) for run in "".join("z" if pr == (0, 0) else " " for pr in pairs).split()) >= 240
    # the top 100 bits zero in one exponent only
    full = rng.getrandbits(1022) | (1 << 1023)  # below 3 * 2^1022 <= p, q
    short = rng.getrandbits(924) | (1 << 923)
    assert full < p - 1 and full < q - 1  # the reduced exponents are these themselves
    ea = [every_a, every_b, runs_a, runs_b, full, short]
    eb = [every_b, every_a, runs_b, runs_a, short, full]
    a = [rng.randrange(R) for _ in ea]
    b = [rng.randrange(R) for _ in ea]
    a[2], b[3] = p * 5, q * 7
    assert modexp2(mk_crt, a, b, ea, eb, 128) == want2(n, a, b, ea, eb)
    assert mk_crt.crt_powmod2(a, b, ea, eb) == want2(n, a, b, ea, eb)


def test_round_call_errors(mk, mk_crt, engine):
    lib, ctx = engine.lib, engine._ctx
    z = np.zeros(4096, np.uint8)
    pz = z.ctypes.data
    st = np.zeros(1, np.int32)
    msgs = np.zeros(1, dtype=MSG_DTYPE)
    msgs[0] = (pz, 10, 10)
    H, A = _lib.SEC_F_HOST, _lib.SEC_F_ASYNC

    def m2(k, width, count, flags, ptr=pz):
        return lib.sec_bn_crt_modexp2_batch(ctx, k._key, ptr, ptr, ptr, ptr, ptr, ptr, width, count, ptr, flags)

    assert m2(mk_crt, 1, 1, H | A) == _lib.SEC_EINVAL
    assert m2(mk_crt, 1, 1, H | 4) == _lib.SEC_EINVAL
    assert m2(mk_crt, 1, 1, H, None) == _lib.SEC_EINVAL
    assert m2(mk_crt, 1, -1, H) == _lib.SEC_EINVAL
    assert m2(mk, 1, 1, H) == _lib.SEC_ENOCRT
    assert m2(mk, 0, 1, H) == _lib.SEC_ENOCRT        # the missing factors come before the width
    assert m2(mk_crt, 0, 1, H) == _lib.SEC_EINVAL
    assert m2(mk_crt, 4097, 1, H) == _lib.SEC_EINVAL
    assert m2(mk_crt, 1, 0, H, None) == _lib.SEC_OK

    def pr(flags, count=1, ptr=pz):
        return lib.sec_apdp_prove_batch(ctx, mk._key, msgs.ctypes.data, count, ptr, ptr, ptr, ptr, ptr, ptr, flags)

    assert pr(H | A) == _lib.SEC_EINVAL
    assert pr(H | 8) == _lib.SEC_EINVAL
    assert pr(H, 1, None) == _lib.SEC_EINVAL
    assert pr(H, 0, None) == _lib.SEC_OK

    def vf(k, flags, count=1, ptr=pz):
        return lib.sec_apdp_verify_batch(ctx, k._key, ptr, ptr, ptr, ptr, ptr, count, ptr, st.ctypes.data if ptr else None,
                                         flags)

    assert vf(mk_crt, 0) == _lib.SEC_EINVAL          # host memory only
    assert vf(mk_crt, H | A) == _lib.SEC_EINVAL
    assert vf(mk_crt, H, 1, None) == _lib.SEC_EINVAL
    assert vf(mk, H) == _lib.SEC_ENOCRT
    assert vf(mk_crt, H, 0, None) == _lib.SEC_OK
    assert not z.any() and st[0] == 0
    with pytest.raises(ECRuntimeError):
        mk.crt_powmod2([1], [1], [1], [1])
    with pytest.raises(ECRuntimeError):
        mk.verify_values([1], [1], [1], [1], 3)


def test_round_kernels_report_bignum_time(mk, mk_crt, engine):
    rng = random.Random(2)
    engine.sync()
    engine.collect_timing("bignum")
    engine.set_timing(True)
    mk_crt.crt_powmod2([rng.randrange(R)], [rng.randrange(R)], [rng.getrandbits(2048)], [rng.getrandbits(2048)])
    engine.sync()
    ms2, n2 = engine.collect_timing("bignum")
    mk.prove([b"piece"], [5], [7], [9])
    engine.sync()
    engine.set_timing(False)
    ms1, n1 = engine.collect_timing("bignum")
    assert n2 >= 1 and ms2 > 0 and n1 >= 1 and ms1 > 0, (ms2, n2, ms1, n1)


# ---- sec_apdp_prove_batch -----------------------------------------------------------------------
def test_prove_against_the_oracle_over_lengths(mk, key):
    n, e, d, p, q = key
    rng = random.Random(41)
    g = pow(31337, 2, n)
    lens = [1, 255, 256, 257, 8192, 8193, 24577, 262147]
    datas = [rng.randbytes(ln) for ln in lens]
    datas[3] = b"\xff" * 257
    tags = [rng.randrange(n) for _ in lens]
    ch_keys = [rng.randbytes(44) for _ in lens]
    g_ss = [pow(g, rng.randrange(2, n), n) for _ in lens]
    coefs = [int.from_bytes(apdp_ref.prf(k, 0), "big") % n for k in ch_keys]
    tag_c, block, rho = mk.prove(datas, tags, g_ss, coefs)
    for i, data in enumerate(datas):
        agg_tag, agg_blocks, hashed = apdp_ref.proof(n, data, tags[i], ch_keys[i], g_ss[i])
        assert (tag_c[i], block[i], b64sha(rho[i])) == (agg_tag, agg_blocks, hashed), lens[i]
        assert rho[i] == pow(g_ss[i], agg_blocks, n)


def test_prove_edge_coefficients_and_bases(mk, key):
    n = key[0]
    rng = random.Random(42)
    cs = [0, 1, C_MAX, rng.getrandbits(256)]
    gs = [0, 1, n - 1, rng.randrange(n)]
    ones = int("00000000ffffffff" * 32, 16)       # runs of all-ones limbs, below n
    almost = (1 << 2047) - 1                        # 63 all-ones limbs under 0x7fffffff
    assert ones < n and almost < n
    xs, tags, coefs, g_ss = [], [], [], []
    for i, c in enumerate(cs):
        for j, g_s in enumerate(gs):
            xs.append([rng.randrange(n), ones, almost, 0][(i + j) % 4])
            tags.append([rng.randrange(n), R - 1, n, n + 5][(i + 2 * j) % 4])
            coefs.append(c)
            g_ss.append(g_s)
    xs += [ones, almost, n - 1]
    tags += [rng.randrange(R)] * 3
    coefs += [C_MAX] * 3
    g_ss += [rng.randrange(R)] * 3                 # g_s beyond n too
    datas = [x.to_bytes(256, "big") for x in xs]
    tag_c, block, rho = mk.prove(datas, tags, g_ss, coefs)
    for i, x in enumerate(xs):
        want = (pow(tags[i], coefs[i], n), coefs[i] * x, pow(g_ss[i], coefs[i] * x, n))
        assert (tag_c[i], block[i], rho[i]) == want, i


@pytest.mark.parametrize("n", [R - 1, (1 << 2047) + 1], ids=["2^2048-1", "2^2047+1"])
def test_prove_edge_moduli_carry_through_the_top_limbs(engine, n):
    rng = random.Random(n % 1000)
    k = bn.ModKey(n, engine)
    xs = [n - 1, n - 1, (n - 1) // 2, 1]
    coefs = [C_MAX, rng.getrandbits(256) | (1 << 255), C_MAX, C_MAX]
    tags = [rng.randrange(R) for _ in xs]
    g_ss = [rng.randrange(R) for _ in xs]
    # X = n - 1 from a longer message too: (n - 1) + n * 2^2048 reduces to it
    datas = [xs[0].to_bytes(256, "big"), (xs[1] + (n << 2048)).to_bytes(513, "big"), xs[2].to_bytes(256, "big"),
             xs[3].to_bytes(1, "big")]
    tag_c, block, rho = k.prove(datas, tags, g_ss, coefs)
    for i, x in enumerate(xs):
        assert block[i] == coefs[i] * x and (i == 3 or block[i].bit_length() > 2048 + 32), i
        assert (tag_c[i], rho[i]) == (pow(tags[i], coefs[i], n), pow(g_ss[i], coefs[i] * x, n)), i
    k.close()


def test_prove_device_with_zero_tail(mk, key):
    n = key[0]
    rng = np.random.default_rng(5)
    pr = random.Random(6)
    buf = torch.from_numpy(rng.integers(0, 256, 1 << 17, dtype=np.uint8)).cuda()
    host = buf.cpu().numpy().tobytes()
    shapes = [(0, 20000, 20000), (30000, 9000, 100), (50000, 8193, 8192), (70000, 300, 0), (80000, 1, 1)]
    msgs = np.zeros(len(shapes), dtype=MSG_DTYPE)
    xs = []
    for i, (off, ln, av) in enumerate(shapes):
        msgs[i] = (buf.data_ptr() + off, ln, av)
        xs.append(int.from_bytes(host[off:off + av] + b"\0" * (ln - av), "big") % n)
    tags = [pr.randrange(R) for _ in shapes]
    g_ss = [pr.randrange(n) for _ in shapes]
    coefs = [pr.getrandbits(256) for _ in shapes]
    dev = [torch.from_numpy(x).cuda() for x in (bn.to_be(tags), bn.to_be(g_ss), bn.to_be(coefs, 32))]
    tag_c, rho = (torch.zeros(len(shapes) * 256, dtype=torch.uint8, device="cuda") for _ in range(2))
    block = torch.zeros(len(shapes) * 288, dtype=torch.uint8, device="cuda")
    mk.prove_batch(msgs, *dev, tag_c, block, rho)
    assert bn.from_be(tag_c.cpu().numpy()) == [pow(t, c, n) for t, c in zip(tags, coefs)]
    got = [int.from_bytes(r.tobytes(), "big") for r in block.cpu().numpy().reshape(-1, 288)]
    assert got == [c * x for c, x in zip(coefs, xs)]
    assert bn.from_be(rho.cpu().numpy()) == [pow(g, c * x, n) for g, c, x in zip(g_ss, coefs, xs)]


# ---- sec_apdp_verify_batch ----------------------------------------------------------------------
def oracle_tau_s(n, e, T, F, c, s):
    """apdp_ref.verify's arithmetic up to the hash."""
    return pow(pow(T, e, n) * pow(pow(F, c, n) % n, -1, n) % n, s, n)


def test_verify_values_against_the_oracle(mk_crt, key):
    n, e, d, p, q = key
    rng = random.Random(51)
    g = pow(31337, 2, n)
    prf_key = b"validator-prf-key-0123456789abcdef0123456789"
    prf_value = apdp_ref.prf(prf_key, 0)
    F = apdp_ref.full_domain_hash(n, prf_value)
    items = []
    for i in range(9):
        data = rng.randbytes(rng.randrange(1, 3000))
        tag = apdp_ref.tag_value(n, g, d, prf_key, data)
        s = rng.randrange(2, n)
        ch_key = rng.randbytes(44)
        held = data if i < 8 else data[:-1] + bytes([data[-1] ^ 0x40])  # the ninth miner's piece is damaged
        agg_tag, _blocks, hashed = apdp_ref.proof(n, held, tag, ch_key, pow(g, s, n))
        items.append((agg_tag, hashed, ch_key, s, i < 8))
    coefs = [int.from_bytes(apdp_ref.prf(k, 0), "big") % n for _, _, k, _, _ in items]
    values, status = mk_crt.verify_values([t for t, *_ in items], [F] * 9, coefs, [s for *_, s, _ in items], e)
    assert status == [0] * 9
    for (agg_tag, hashed, ch_key, s, honest), v in zip(items, values):
        # v is the oracle's tau_s: the oracle accepts its hash; the proof's hash matches when honest
        assert apdp_ref.verify(n, e, agg_tag, b64sha(v), ch_key, prf_value, s)
        assert (b64sha(v) == hashed) == honest
        assert apdp_ref.verify(n, e, agg_tag, hashed, ch_key, prf_value, s) == honest


def test_verify_values_edges_and_status(mk_crt, key):
    n, e, d, p, q = key
    rng = random.Random(52)
    r = lambda: rng.randrange(2, n)  # noqa: E731
    c = lambda: rng.getrandbits(256)  # noqa: E731
    cases = [  # (T, F, c, s, invertible)
        (r(), r(), 0, r(), True), (r(), r(), c(), 0, True), (p * 77, r(), c(), r(), True),
        (q * 5, r(), C_MAX, r(), True), (0, r(), c(), r(), True), (R - 1, R - 1, c(), R - 1, True),
        (r(), r(), c(), (p - 1) * (q - 1), True), (r(), p * 991, 0, r(), True),   # c == 0: F^0 = 1
        (r(), p * 991, c(), r(), False), (r(), q * 3, 1, r(), False), (r(), 0, c(), r(), False),
        (r(), r(), c(), r(), True),
    ]
    for ee in (e, 0, 3, R - 1):
        values, status = mk_crt.verify_values([t for t, *_ in cases], [f for _, f, *_ in cases],
                                              [x for _, _, x, _, _ in cases], [s for *_, s, _ in cases], ee)
        for (T, F, cc, s, ok), v, st in zip(cases, values, status):
            if ok:
                assert (v, st) == (oracle_tau_s(n, ee, T, F, cc, s), 0), (T, F, cc, s, ee)
            else:
                assert (v, st) == (0, 1)
                with pytest.raises(ValueError):
                    oracle_tau_s(n, ee, T, F, cc, s)
    with pytest.raises(ValueError):
        mk_crt.verify_values([1], [1], [1], [-1], e)


def test_verify_values_many_items_use_the_host_threads(mk_crt, key):
    """More items than one host task derives (64): the exponents come from the library's threads."""
    n, e, d, p, q = key
    rng = random.Random(53)
    k = 150
    T, F, s = ([rng.randrange(n) for _ in range(k)] for _ in range(3))
    c = [rng.getrandbits(256) for _ in range(k)]
    F[70] = p * 3
    values, status = mk_crt.verify_values(T, F, c, s, e)
    assert status == [int(i == 70) for i in range(k)]
    assert values == [0 if i == 70 else oracle_tau_s(n, e, T[i], F[i], c[i], s[i]) for i in range(k)]


# ---- ChallengeSystem ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cs(key):
    n, e, d, p, q = key
    cs = apdp.ChallengeSystem()
    cs.key.rsa = apdp.RSAPrivateKey(p, q, e)
    cs.key.g = pow(31337, 2, n)
    cs.key.prf_key = b"prf-key-for-tests-0123456789abcdef0123456789="
    return cs


def test_challenge_round_equals_the_oracle(cs, key):
    n, e, d, p, q = key
    rng = random.Random(61)
    datas = [rng.randbytes(ln) for ln in (1, 8193, 70000)]
    tags = cs.generate_tags(datas)
    chs = cs.issue_challenges(tags)
    proofs = cs.generate_proofs(list(zip(datas, tags, chs)), n)
    for data, t, ch, pr in zip(datas, tags, chs, proofs):
        assert t.tag_value == apdp_ref.tag_value(n, cs.key.g, d, cs.key.prf_key, data)
        assert (pr.tag_value, pr.block_value, pr.hashed_result) == apdp_ref.proof(n, data, t.tag_value, ch.prf_key,
                                                                                  ch.g_s)
        assert apdp_ref.verify(n, e, pr.tag_value, pr.hashed_result, ch.prf_key, t.prf_value, ch.s)
    assert cs.verify_proofs(list(zip(proofs, chs, tags)), n, e) == [True] * 3
    wrong = [proofs[1], proofs[0], proofs[2].model_copy(update={"tag_value": proofs[2].tag_value + R})]
    want = [apdp_ref.verify(n, e, pr.tag_value, pr.hashed_result, ch.prf_key, t.prf_value, ch.s)
            for pr, ch, t in zip(wrong, chs, tags)]
    assert want == [False] * 3
    assert cs.verify_proofs(list(zip(wrong, chs, tags)), n, e) == want
    # a foreign modulus, a negative s, an s wider than the modulus
    assert cs.verify_proofs(list(zip(proofs, chs, tags)), n + 2, e) == [False] * 3
    with pytest.raises(ValueError):
        cs.verify_proofs([(proofs[0], chs[0].model_copy(update={"s": -5}), tags[0])], n, e)
    lam = (p - 1) * (q - 1)
    wide = chs[0].model_copy(update={"s": chs[0].s + 3 * lam})
    assert wide.s >= R and cs.verify_proofs([(proofs[0], wide, tags[0])], n, e) == [True]


def test_challenge_round_after_json(cs):
    data = random.Random(62).randbytes(5000)
    tag = apdp.APDPTag.model_validate_json(cs.generate_tag(data).model_dump_json())
    ch = apdp.Challenge.model_validate_json(cs.issue_challenge(tag.model_dump_json()).model_dump_json())
    pr = apdp.Proof.model_validate_json(cs.generate_proof(data, ch.tag, ch).model_dump_json())
    assert cs.verify_proof(pr, ch, tag)
    assert not cs.verify_proof(pr.model_copy(update={"tag_value": pr.tag_value + 1}), ch, tag)


def test_non_invertible_denominator_raises(cs, key, monkeypatch):
    """An FDH value that is a multiple of p has no inverse: status 1 from the library, the
    reference's APDPError from the system.  (No PRF value hashes to such a number on purpose, so
    the hash is replaced for this test.)"""
    n, e, d, p, q = key
    data = b"some piece"
    tag = cs.generate_tag(data)
    ch = cs.issue_challenge(tag)
    pr = cs.generate_proof(data, tag, ch)
    monkeypatch.setattr(apdp.CryptoUtils, "full_domain_hash", staticmethod(lambda rsa_key, data: p * 12345))
    with pytest.raises(apdp.APDPError, match="Failed to invert denominator modulo n."):
        cs.verify_proofs([(pr, ch, tag)])
