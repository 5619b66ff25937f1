"""GPU: the bignum kernels' data-dependent carry, compare and borrow paths (bignum.hip).

Every operand family of tests/bn_vectors.py goes through the real entry points and is judged
bit-exactly by Python ints.  Which paths those operands take is certified on the CPU by the
limb-level model (oracle/bn_model.py, tests/test_bn_model.py); the model is never the judge
here.  Uniformly random operands (tests/test_apdp_gpu.py) take those paths with probability
~2^-32 per limb.
"""

import random

import numpy as np
import pytest

from tests import bn_vectors as bv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from storb_amd import bn  # noqa: E402
from storb_amd._lib import MSG_DTYPE  # noqa: E402

R = bv.R


def same(got, want, labels):
    """Bit-exact, naming the vectors that differ."""
    assert len(got) == len(want) == len(labels)
    bad = [lab for g, w, lab in zip(got, want, labels) if g != w]
    assert not bad, "%d of %d differ: %s" % (len(bad), len(got), bad[:12])


@pytest.fixture(scope="module")
def keys(engine):
    return {name: bn.ModKey(bv.modulus(name), engine) for name in bv.FULL_NAMES}


@pytest.fixture(scope="module")
def crt_keys(engine):
    out = {}
    for name in bv.PAIR_NAMES:
        p, q = bv.pair(name)
        out[name] = bn.ModKey(p * q, engine)
        out[name].set_crt(p, q)
    return out


# ---- mulmod, powmod ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", bv.FULL_NAMES)
def test_mulmod_targets(keys, name):
    n = bv.modulus(name)
    labels, a, b = map(list, zip(*bv.mulmod_vectors(name)))
    same(keys[name].mulmod(a, b), [x * y % n for x, y in zip(a, b)], labels)


@pytest.mark.parametrize("name", bv.FULL_NAMES)
def test_powmod_targets_and_window_shapes(keys, name):
    n = bv.modulus(name)
    labels, bases, exps = map(list, zip(*bv.powmod_vectors(name)))
    same(keys[name].powmod(bases, exps), [pow(b, e, n) for b, e in zip(bases, exps)], labels)


@pytest.mark.parametrize("name", ["key", "ones_minus_mid"])
def test_powmod_widest_exponent(keys, name):
    """2^32767 at the maximum width of 4096 bytes (8191 zero nibbles after the leading one),
    next to short exponents padded to the same width."""
    n = bv.modulus(name)
    tg = bv.targets(n)
    bases = [tg[0][1], tg[40][1], n - 1, R - 1, 3]
    exps = [bv.WIDE_EXP, bv.WIDE_EXP, bv.WIDE_EXP, 1, 0x1001]
    same(keys[name].powmod(bases, exps), [pow(b, e, n) for b, e in zip(bases, exps)], exps)


# ---- CRT halves -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bv.PAIR_NAMES)
def test_crt_powmod_pq_targets(crt_keys, name):
    items = bv.crt_vectors(name)
    got = crt_keys[name].crt_powmod_pq([it["x"] for it in items], [it["ep"] for it in items],
                                       [it["eq"] for it in items])
    same(got, [bv.crt_expected(name, it["x"], it["ep"], it["eq"]) for it in items], [it["label"] for it in items])


@pytest.mark.parametrize("name", bv.PAIR_NAMES)
def test_crt_powmod_targets(crt_keys, name):
    """crt_powmod against pow(b, e, n).  The half exponents are e itself for e below p-1 and
    q-1, which is exact for any coprime pair; only the key's factors are prime, so only there
    do exponents that wrap around p-1 have pow(b, e, n) as their reference."""
    p, q = bv.pair(name)
    n = p * q
    items = bv.crt_vectors(name)[::5]
    small = (1, 2, 3, 16, 17, 65537)
    bases = [it["x"] for it in items]
    exps = [small[i % len(small)] for i in range(len(bases))]
    if name == "key":
        rng = random.Random(77)
        wrap = [p - 1, (p - 1) * (q - 1), (p - 1) * (q - 1) + 1, p, q - 1, rng.getrandbits(2048), rng.getrandbits(2048)]
        bases += [it["x"] for it in items[:len(wrap)]]
        exps += wrap
    same(crt_keys[name].crt_powmod(bases, exps), [pow(b, e, n) for b, e in zip(bases, exps)],
         [it["label"] for it in items] + ["wrap"] * (len(bases) - len(items)))


# ---- reduce -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bv.FULL_NAMES)
def test_reduce_two_chunk_targets(keys, name):
    n = bv.modulus(name)
    labels, msgs, _ = map(list, zip(*bv.reduce_two_chunk(name)))
    same(keys[name].reduce(msgs), [int.from_bytes(m, "big") % n for m in msgs], labels)


@pytest.mark.parametrize("name", ["key", "ones", "low_ones"])
def test_reduce_segment_boundary_lengths(keys, name):
    n = bv.modulus(name)
    msgs = bv.reduce_boundary_messages()
    same(keys[name].reduce(msgs), [int.from_bytes(m, "big") % n for m in msgs], [len(m) for m in msgs])


@pytest.mark.parametrize("name", ["key", "ones_minus_mid"])
@pytest.mark.parametrize("fill", ["random", "ones"])
def test_reduce_device_avail_edges(keys, name, fill):
    """reduce_batch on device memory with `avail` cut at segment, chunk and limb edges."""
    n = bv.modulus(name)
    size = 1 << 15
    host = np.random.default_rng(5).integers(0, 256, size, dtype=np.uint8) if fill == "random" else \
        np.full(size, 0xFF, np.uint8)
    buf = torch.from_numpy(host).cuda()
    raw = host.tobytes()
    cases = bv.avail_cases()
    msgs = np.zeros(len(cases), dtype=MSG_DTYPE)
    want = []
    for i, (ln, av) in enumerate(cases):
        off = (37 * i) % (size - 20000)
        msgs[i] = (buf.data_ptr() + off, ln, av)
        want.append(int.from_bytes(raw[off:off + av] + b"\0" * (ln - av), "big") % n)
    out = torch.empty(len(cases) * 256, dtype=torch.uint8, device="cuda")
    keys[name].reduce_batch(msgs, out)
    same(bn.from_be(out.cpu().numpy()), want, cases)


def test_reduce_weight_table_grows(engine):
    """The per-key table of R^(32j) grows on demand: a 20 KiB message (3 segments), then a
    300 KiB one (38 segments: the table is reallocated and its old entries copied), then the
    first again, on a fresh key."""
    n = bv.modulus("key")
    k = bn.ModKey(n, engine)
    rng = random.Random(31)
    small, big = rng.randbytes(20 << 10), rng.randbytes(300 << 10)
    first = k.reduce([small])
    assert first == [int.from_bytes(small, "big") % n]
    assert k.reduce([big]) == [int.from_bytes(big, "big") % n]
    again = k.reduce([small])
    assert again == [int.from_bytes(small, "big") % n]
    assert again == first
    k.close()


# ---- fixed-base powers and tags -----------------------------------------------------------------

TAG_KEYS = [(name, False) for name in bv.FULL_NAMES] + [("key", True)]


@pytest.fixture(scope="module", params=TAG_KEYS, ids=["%s-%s" % (n, "crt" if c else "plain") for n, c in TAG_KEYS])
def tag_key(request, engine):
    """(ModKey with tag constants, n, g, fdh, d).  Only the RSA key has a meaningful d and
    prime factors; the arithmetic (fdh * g^X)^d mod n is defined for any of the moduli."""
    name, crt = request.param
    n = bv.modulus(name)
    rng = random.Random("tag key " + name)
    g = pow(rng.randrange(2, n), 2, n)
    fdh = rng.getrandbits(256)
    d = bv.key()[2] if name == "key" else rng.getrandbits(2048)
    k = bn.ModKey(n, engine)
    if crt:
        k.set_crt(*bv.key()[3:5])
    k.set_tag(g, fdh, d)
    yield k, n, g, fdh, d
    k.close()


def test_gpow_byte_positions(tag_key):
    k, n, g, _, _ = tag_key
    by_width = {}
    for label, width, e in bv.gpow_cases():
        by_width.setdefault(width, []).append((label, e))
    for width, cases in sorted(by_width.items()):
        exps = [e for _, e in cases]
        out = np.empty((len(exps), bn.NBYTES), dtype=np.uint8)
        k.gpow_batch(bn.to_be(exps, width), width, len(exps), out, host=True)
        same(bn.from_be(out), [pow(g, e, n) for e in exps], [lab for lab, _ in cases])


def test_tags_half_empty_residues(tag_key):
    k, n, g, fdh, d = tag_key
    labels, pieces = map(list, zip(*bv.tag_pieces(n)))
    want = [pow(fdh * pow(g, int.from_bytes(x, "big") % n, n) % n, d, n) for x in pieces]
    same(k.tags(pieces), want, labels)


# ---- device-resident batches, mixed batches -------------------------------------------------------

def _dev(rows):
    return torch.from_numpy(rows).cuda()


def test_device_resident_mulmod_and_modexp(keys, engine):
    n = bv.modulus("key")
    k = keys["key"]
    labels, a, b = map(list, zip(*bv.mulmod_vectors("key")[:120]))
    out = torch.empty(len(a) * 256, dtype=torch.uint8, device="cuda")
    k.mulmod_batch(_dev(bn.to_be(a)), _dev(bn.to_be(b)), len(a), out)
    engine.sync()
    same(bn.from_be(out.cpu().numpy()), [x * y % n for x, y in zip(a, b)], labels)
    labels, bases, exps = map(list, zip(*bv.powmod_vectors("key")[:120]))
    out = torch.empty(len(bases) * 256, dtype=torch.uint8, device="cuda")
    k.modexp_batch(_dev(bn.to_be(bases)), _dev(bn.to_be(exps, 4)), 4, len(bases), out)
    engine.sync()
    same(bn.from_be(out.cpu().numpy()), [pow(x, e, n) for x, e in zip(bases, exps)], labels)


@pytest.mark.parametrize("name", ["key", "ones_minus_mid"])
def test_targeted_and_random_items_mixed(keys, name):
    """Neighbouring workgroups take different paths: targeted and random items alternate."""
    n = bv.modulus(name)
    rng = random.Random("mixed " + name)
    labels, a, b = [], [], []
    for lab, x, y in bv.mulmod_vectors(name)[::3]:
        labels += [lab, "random"]
        a += [x, rng.randrange(R)]
        b += [y, rng.randrange(R)]
    same(keys[name].mulmod(a, b), [x * y % n for x, y in zip(a, b)], labels)
    labels, bases, exps = [], [], []
    for lab, x, e in bv.powmod_vectors(name)[::3]:
        labels += [lab, "random"]
        bases += [x, rng.randrange(R)]
        exps += [e, rng.getrandbits(32)]
    same(keys[name].powmod(bases, exps), [pow(x, e, n) for x, e in zip(bases, exps)], labels)


def test_crt_targeted_and_random_items_mixed(crt_keys):
    name = "mid"
    rng = random.Random("mixed crt")
    xs, eps, eqs, labels = [], [], [], []
    for it in bv.crt_vectors(name)[::4]:
        labels += [it["label"], "random"]
        xs += [it["x"], rng.randrange(R)]
        eps += [it["ep"], rng.getrandbits(48)]
        eqs += [it["eq"], rng.getrandbits(48)]
    same(crt_keys[name].crt_powmod_pq(xs, eps, eqs),
         [bv.crt_expected(name, x, ep, eq) for x, ep, eq in zip(xs, eps, eqs)], labels)
