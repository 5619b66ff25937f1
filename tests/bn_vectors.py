"""Seeded, deterministic operand families for the bignum kernels (storb_amd/csrc/bignum.hip),
shared by tests/test_bn_model.py (CPU: the limb-level model certifies which carry / compare /
borrow paths each family reaches) and tests/test_gpu_bn_paths.py (GPU: the same operands
through the real entry points, judged by Python ints).

Uniformly random operands reach the data-dependent branches of the carry-lookahead, the
compare and the subtract with probability ~2^-32 per limb.  The families here choose the
RESULT of a product or sum (a target T with runs of extreme limbs, next to 0 or the modulus,
or equal to the modulus down to a chosen limb) and derive operands that make one specific
product or sum inside a kernel land on it.

Everything is a pure function of the names below; nothing here touches a GPU.
"""

from __future__ import annotations

import functools
import math
import random

from oracle import apdp_ref

R = 1 << 2048
RH = 1 << 1024  # R of a 1024-bit CRT half
M32 = 0xFFFFFFFF
SEG_BYTES = 8192  # kSegChunks * 256 (bignum.hpp)

# ---- moduli ---------------------------------------------------------------------------------

FULL_NAMES = ("key", "ones", "top_plus_one", "ones_minus_mid", "low_ones", "limb0_one")
TOP_HEAVY = ("ones", "ones_minus_mid")  # nearly 2^2048: the carry out of limb 63 is common
PAIR_NAMES = ("key", "p105", "ones", "three_quarters", "mid")


@functools.lru_cache(maxsize=None)
def key():
    """The suite's RSA test key (n, e, d, p, q)."""
    return apdp_ref.test_key(11)


@functools.lru_cache(maxsize=None)
def modulus(name: str) -> int:
    """A full 2048-bit odd modulus.  low_ones has limbs 0..31 all ones (n0inv = 1), limb0_one
    has limb 0 equal to 1 (n0inv = 0xFFFFFFFF), as has top_plus_one."""
    if name == "key":
        return key()[0]
    if name == "ones":
        return R - 1
    if name == "top_plus_one":
        return (1 << 2047) + 1
    if name == "ones_minus_mid":
        return R - (1 << 1024) - 1
    rng = random.Random("bn_vectors modulus " + name)
    if name == "low_ones":
        return ((rng.getrandbits(1024) | 1 << 1023) << 1024) | (RH - 1)
    if name == "limb0_one":
        return ((rng.getrandbits(2048) | 1 << 2047) >> 32 << 32) | 1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def pair(name: str) -> tuple[int, int]:
    """1024-bit odd coprime (p, q) whose product has 2048 bits.  Only "key" is a pair of
    primes: for the others the reference is the CRT of pow(b, ep, p) and pow(b, eq, q)."""
    p, q = {
        "key": key()[3:5],
        "p105": (RH - 105, (1 << 1023) + 1155),
        "ones": (RH - 1, RH - 3),
        "three_quarters": ((1 << 1023) + (1 << 1022) + 1, (1 << 1023) + (1 << 1022) + 3),
        "mid": (RH - (1 << 512) - 1, RH - (1 << 32) + 1),
    }[name]
    assert p.bit_length() == q.bit_length() == 1024 and p & q & 1
    assert math.gcd(p, q) == 1 and (p * q).bit_length() == 2048
    return p, q


def crt(p: int, q: int, tp: int, tq: int) -> int:
    """x mod p*q with x = tp mod p and x = tq mod q."""
    return (tp * q * pow(q, -1, p) + tq * p * pow(p, -1, q)) % (p * q)


# ---- targets: chosen results ------------------------------------------------------------------

def _limb(x: int, j: int) -> int:
    return (x >> (32 * j)) & M32


def rand_unit(rng: random.Random, m: int) -> int:
    while True:
        a = rng.randrange(2, m)
        if math.gcd(a, m) == 1:
            return a


def differ_limbs(bits: int) -> tuple[int, ...]:
    return (0, 1, 31, 32, 62) if bits == 2048 else (0, 1, 15, 16, 30)


def near_distances(bits: int) -> tuple[int, ...]:
    far = (1 << 1024, 1 << 2016) if bits == 2048 else (1 << 512, 1 << 992)
    return (0, 1, 2, 3, 4, 5, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 64) + far


@functools.lru_cache(maxsize=None)
def targets(m: int, bits: int = 2048) -> tuple[tuple[str, int], ...]:
    """(label, T) with 0 <= T < m:
      run:<kind><len>   a run of `len` (1..21) zero / all-ones limbs in a random value, or of
                        random limbs in an all-ones / all-zero value; the top limb stays below
                        m's so that T < m
      near:<d> / near:m-1-<d>
      below<j>          equal to m in every limb above j, smaller at limb j
      above<j>          V - m for V equal to m above limb j and larger at j (so a product or
                        sum whose unreduced value is V compares at limb j, then subtracts)
      borrow<k>         c * 2^(32k) - d: where the unreduced value is T + m, its limb 0 is below
                        m's, limbs 1..k-1 equal m's and limb k is above: the subtract's borrow
                        travels through the equal limbs
    """
    L = bits // 32
    rng = random.Random("bn_vectors targets %x" % m)
    top = m >> (32 * (L - 1))
    body = (1 << (32 * (L - 1))) - 1
    out: list[tuple[str, int]] = []
    for ln in range(1, 22):
        for kind in ("zero", "ones", "rand"):
            pos = rng.randrange(0, L - ln)  # the run lies in limbs [pos, pos+ln), below the top limb
            mask = ((1 << (32 * ln)) - 1) << (32 * pos)
            t = rng.getrandbits(32 * (L - 1))
            if kind == "zero":
                t &= ~mask
            elif kind == "ones":
                t |= mask
            else:
                t = (t & mask) | (body & ~mask if ln & 1 else 0)
            out.append(("run:%s%d" % (kind, ln), t | rng.randrange(top) << (32 * (L - 1))))
    for i, d in enumerate(near_distances(bits)):
        if d < m:
            out.append(("near:d%d" % i, d))
            out.append(("near:m-1-d%d" % i, m - 1 - d))
    for j in differ_limbs(bits):
        hi = m >> (32 * (j + 1)) << (32 * (j + 1))
        mj = _limb(m, j)
        low = rng.getrandbits(32 * j) if j else 0
        if mj > 0:
            out.append(("below%d" % j, hi | (mj - 1) << (32 * j) | low))
            out.append(("below%d:ones" % j, hi | (mj - 1) << (32 * j) | ((1 << (32 * j)) - 1)))
        if mj < M32:
            out.append(("above%d" % j, (hi | (mj + 1) << (32 * j) | low) - m))
            out.append(("above%d:zero" % j, (hi | (mj + 1) << (32 * j)) - m))
    for k in (1, 2, 8, 16, 31, 32, 62):
        if k < L:
            for c, d in ((1, 1), (2, 3), (1, 1 << 31)):
                out.append(("borrow%d:%d" % (k, c), (c << (32 * k)) - d))
    assert all(0 <= t < m for _, t in out)
    return tuple(out)


# ---- structured operands: limbs drawn from {0, 1, 0xFFFFFFFE, 0xFFFFFFFF} ----------------------

_DIGIT = (0, 1, 0xFFFFFFFE, 0xFFFFFFFF)


def from_digits(s: str) -> int:
    """'0123...' (limb 0 first) -> the integer with limbs 0, 1, 0xFFFFFFFE, 0xFFFFFFFF."""
    return sum(_DIGIT[int(c)] << (32 * j) for j, c in enumerate(s))


def structured_digits(rng: random.Random, nlimbs: int = 64) -> str:
    return "".join(rng.choice("0123") for _ in range(nlimbs))


# carry_two (a lane owing two carries after the rows): found by search_carry_two(name,
# seed=2024, bound=300): structured pairs (a, b) through the two products of mulmod, in the
# limb-level model.  The first hits per modulus are kept (digits as for from_digits).  A
# modulus listed in CARRY_TWO_NOT_FOUND had no hit within that bound.
CARRY_TWO_SEED = 2024
CARRY_TWO_BOUND = 300
CARRY_TWO: dict[str, tuple[tuple[str, str], ...]] = {
    "ones": (
        ("2201303332231111200020133113113112133021202311110200000320002230",
         "2331020023001320200102201000322002220111222302200221013220301313"),
    ),
    "ones_minus_mid": (
        ("2132322303232330020113231201032201330233323100003322332313010022",
         "0123213301320003010100302123332230002220300031120303121210220113"),
        ("3003320330222133230213210020110302310120131223302111222030112213",
         "3303302330201000111100313121202030223222330001311001333332333303"),
        ("3131002010312323300012022000113233312120113110310102201320102032",
         "0223023100300301203100301013232331011321211130231201201310021122"),
    ),
}
# It takes a lane's second add to overflow on top of the first: its sum must be 0xFFFFFFFF
# before the carry bit of p2 comes in, which structured limbs give only where the modulus'
# own limbs are extreme.
CARRY_TWO_NOT_FOUND: tuple[str, ...] = ("key", "top_plus_one", "low_ones", "limb0_one")


def search_carry_two(name: str, seed: int = CARRY_TWO_SEED, bound: int = CARRY_TWO_BOUND, keep: int = 3):
    """Bounded seeded search on the CPU model; returns up to `keep` (a_digits, b_digits)."""
    from oracle import bn_model as bm

    M = bm.make_mod(modulus(name))
    rng = random.Random("carry_two %s %d" % (name, seed))
    found = []
    for _ in range(bound):
        a, b = structured_digits(rng), structured_digits(rng)
        ev = bm.Collector()
        bm.mulmod(M, bm.limbs(from_digits(a)), bm.limbs(from_digits(b)), ev)
        if ev.count("carry_two"):
            found.append((a, b))
            if len(found) == keep:
                break
    return found


# ---- mulmod -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mulmod_vectors(name: str) -> tuple[tuple[str, int, int], ...]:
    """(label, a, b) for ModKey.mulmod (am = mont(a, R^2), out = mont(b, am)):
      final:<target>   the second product lands on T: a a random unit, b = T / a
      first:<target>   the first product lands on T: a = T / R (every second target)
      final_big:<t>    as final:, with a*R mod n within 2^64 of n and b lifted by n
      equal:*          an operand equal to the modulus: the unreduced product is exactly n
      struct:*         both operands with limbs from {0, 1, 0xFFFFFFFE, 0xFFFFFFFF}
      carry2:*         the searched carry_two vectors
    Every third operand is lifted by n where that stays below 2^2048 (operands need not be
    reduced)."""
    m = modulus(name)
    rng = random.Random("bn_vectors mulmod " + name)
    rinv = pow(R, -1, m)
    out = []
    for i, (label, t) in enumerate(targets(m)):
        a = rand_unit(rng, m)
        b = t * pow(a, -1, m) % m
        if i % 3 == 0 and b + m < R:
            b += m
        out.append(("final:" + label, a, b))
        if i % 2 == 0:
            a = t * rinv % m
            if i % 4 == 0 and a + m < R:
                a += m
            out.append(("first:" + label, a, rng.randrange(R)))
        if label.startswith(("borrow", "above", "near:d")):
            # both factors of the final product as large as they go, so that its unreduced
            # value tends to be T + n and the subtract runs on it
            while True:
                a = (m - 1 - rng.getrandbits(64)) * rinv % m
                if math.gcd(a, m) == 1:
                    break
            b = t * pow(a, -1, m) % m
            out.append(("final_big:" + label, a, b + m if b + m < R else b))
    r = [rng.randrange(R) for _ in range(4)]
    out += [("equal:a", m, r[0]), ("equal:b", r[1] % m or 1, m), ("equal:ab", m, m), ("equal:a1", m, 1),
            ("equal:b1", 1, m), ("edge:00", 0, 0), ("edge:11", 1, 1), ("edge:m-1", m - 1, m - 1),
            ("edge:R-1", R - 1, R - 1), ("edge:R-1,m-1", R - 1, m - 1), ("edge:rand", r[2], r[3])]
    for i in range(24):
        out.append(("struct:%d" % i, from_digits(structured_digits(rng)), from_digits(structured_digits(rng))))
    for i, (a, b) in enumerate(CARRY_TWO.get(name, ())):
        out.append(("carry2:%d" % i, from_digits(a), from_digits(b)))
    return tuple(out)


# ---- powmod -----------------------------------------------------------------------------------

SMALL_EXPS = (1, 2, 3, 16, 17)


def exponent_shapes() -> tuple[tuple[str, int], ...]:
    """Exponents the 4-bit window code treats specially (all at most 4 bytes wide)."""
    out = []
    for k in range(8):
        out.append(("nibble1@%d" % k, 1 << (4 * k)))  # also 16^k
        out.append(("nibbleF@%d" % k, 15 << (4 * k)))
    out += [("alt:F00F", 0xF00F), ("alt:0FF0", 0x0FF0), ("alt:F00FF00F", 0xF00FF00F), ("alt:0FF00FF0", 0x0FF00FF0),
            ("gap:1001", 0x1001), ("gap:100001", 0x100001), ("gap:F0000003", 0xF0000003), ("gap:10203", 0x10203),
            ("gap:80000001", 0x80000001), ("zero", 0)]
    return tuple(out)


WIDE_EXP = 1 << 32767  # the widest exponent the library takes (4096 bytes), sparse


@functools.lru_cache(maxsize=None)
def powmod_vectors(name: str) -> tuple[tuple[str, int, int], ...]:
    """(label, base, e) for ModKey.powmod.  Small exponents: the base is an e-th root of the
    target where that is cheap (the key modulus, e coprime to lambda(n)), else the target
    itself (its conversion to Montgomery form and back pass through T*R and T).  Window
    shapes: on a targeted and a random base each."""
    m = modulus(name)
    rng = random.Random("bn_vectors powmod " + name)
    tg = targets(m)
    lam = None
    if name == "key":
        _, _, _, p, q = key()
        lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    out = []
    for i, (label, t) in enumerate(tg):
        e = SMALL_EXPS[i % len(SMALL_EXPS)]
        base = t
        if lam is not None and e > 1 and math.gcd(e, lam) == 1 and math.gcd(t, m) == 1:
            base = pow(t, pow(e, -1, lam), m)
            label += ":root"
        out.append(("e%d:%s" % (e, label), base, e))
    for i, (label, e) in enumerate(exponent_shapes()):
        out.append(("shape:%s:t" % label, tg[(7 * i) % len(tg)][1], e))
        out.append(("shape:%s:r" % label, rng.randrange(R), e))
    return tuple(out)


# ---- CRT --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crt_vectors(name: str) -> tuple[dict, ...]:
    """Items for ModKey.crt_powmod_pq: dicts with label, kind, x, ep, eq and, for the kinds that
    aim at one 32-row product or sum, `site`: a list of (half, what, operand ints) the model
    test replays.
      plain    ep = eq = 1, x = CRT(Tp, Tq): the 32-row product by 1 yields the chosen residues,
               and x itself passes through the final add_mod mod n
      tomont   x = CRT(Tp/Rh, Tq/Rh): the conversion product mont(r, Rh^2) lands on T
      hi       x >= 2^1024 with high half T/Rh mod h: to_half_m's first product lands on T
      hi_equal x's high half equal to p (or q): that product is exactly h before the subtract
      lo       x = hi * 2^1024 + lo with lo making to_half_m's add_mod land on T, T+h or T+2h
      mult     multiples of p and q
      exps     ep != eq, zero exponents, 64-bit exponents (site: the window table's first
               product, the square of x*Rh mod h)
    """
    p, q = pair(name)
    n = p * q
    rng = random.Random("bn_vectors crt " + name)
    tp, tq = targets(p, 1024), targets(q, 1024)
    rinv = (pow(RH, -1, p), pow(RH, -1, q))
    out: list[dict] = []

    def item(label, kind, x, ep=1, eq=1, site=()):
        assert 0 <= x < R
        out.append(dict(label=label, kind=kind, x=x, ep=ep, eq=eq, site=tuple(site)))

    cnt = max(len(tp), len(tq))
    for i in range(cnt):
        (lp, a), (lq, b) = tp[i % len(tp)], tq[(i + 5) % len(tq)]
        item("plain:%s|%s" % (lp, lq), "plain", crt(p, q, a, b),
             site=[(0, "by_one", a * RH % p), (1, "by_one", b * RH % q)])
        ra, rb = a * rinv[0] % p, b * rinv[1] % q
        item("tomont:%s|%s" % (lp, lq), "tomont", crt(p, q, ra, rb),
             site=[(0, "to_mont", ra), (1, "to_mont", rb)])
    for h, (hm, tg) in enumerate(((p, tp), (q, tq))):
        for i, (lab, t) in enumerate(tg):
            hi = t * rinv[h] % hm
            lo = (rng.getrandbits(1024), 0, RH - 1)[i % 3]
            item("hi%d:%s" % (h, lab), "hi", hi << 1024 | lo, site=[(h, "hi", hi, lo)])
            hi = rng.randrange(RH)
            k = i % 3
            lo = (t - hi * RH) % hm + k * hm
            while lo >= RH:
                lo -= hm
            item("lo%d:%s" % (h, lab), "lo", hi << 1024 | lo, site=[(h, "hi", hi, lo)])
        for i, lo in enumerate((0, 1, rng.getrandbits(1024), RH - 1)):
            item("hi_equal%d:%d" % (h, i), "hi_equal", hm << 1024 | lo, site=[(h, "hi", hm, lo)])
    for k in (1, 2, 7, (1 << 1023) // 3):
        for hm in (p, q):
            if hm * k < R:
                item("mult:%d" % (k % 1000), "mult", hm * k)
    for label, v in (("0", 0), ("1", 1), ("n-1", n - 1), ("n", n), ("n+1", n + 1), ("R-1", R - 1)):
        item("edge:" + label, "mult", v)
    pairs = [(1, 2), (2, 1), (3, 17), (16, 1), (17, 16), (0, 1), (1, 0), (0, 0), (0x1001, 0xF00F),
             (rng.getrandbits(64), rng.getrandbits(64)), (rng.getrandbits(64), 5)]
    for i, (ep, eq) in enumerate(pairs):
        src = out[(11 * i) % cnt]
        item("exps:%d:%s" % (i, src["label"]), "exps", src["x"], ep, eq)
        x = rng.randrange(R)  # the window table's first product squares x*Rh mod h
        item("exps:%d:rand" % i, "exps", x, ep, eq, site=[(0, "square", x * RH % p), (1, "square", x * RH % q)])
    return tuple(out)


def crt_expected(name: str, x: int, ep: int, eq: int) -> int:
    p, q = pair(name)
    return crt(p, q, pow(x, ep, p), pow(x, eq, q))


# ---- reduce -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reduce_two_chunk(name: str) -> tuple[tuple[str, bytes, tuple], ...]:
    """(label, message, (r, chunk)) with 257..512-byte messages: the first chunk c0 is random
    (r = c0 mod n), the second is (T - r*R) mod n, plus k*n for k = 0, 1, 2 in turn where that
    stays below 2^2048, so the Horner add_mod lands on T after k subtractions."""
    m = modulus(name)
    rng = random.Random("bn_vectors reduce " + name)
    out = []
    for i, (label, t) in enumerate(targets(m)):
        c0 = rng.randbytes(rng.randrange(1, 257))
        r = int.from_bytes(c0, "big") % m
        k = i % 3
        chunk = (t - r * R) % m + k * m
        while chunk >= R:
            chunk -= m
            k -= 1
        out.append(("k%d:%s" % (k, label), c0 + chunk.to_bytes(256, "big"), (r, chunk)))
        # r*R mod n just below n, so that a second chunk near 2^2048 makes the sum T + 2n
        # (impossible for n = 2^2048 - 1: a + x <= 2n - 1 there)
        base = m - 1 - rng.randrange(4)
        chunk = t + 2 * m - base
        if label.startswith(("near:d", "above", "borrow")) and chunk < R:
            r = base * pow(R, -1, m) % m
            out.append(("k2:%s" % label, r.to_bytes(256, "big") + chunk.to_bytes(256, "big"), (r, chunk)))
    return tuple(out)


BOUNDARY_LENGTHS = (8191, 8192, 8193, 16383, 16384, 16385, 8192 * 32 - 1, 8192 * 32, 8192 * 32 + 1)


def reduce_boundary_messages() -> list[bytes]:
    """Random messages whose lengths sit on the segment boundaries, and all-ones ones."""
    rng = random.Random("bn_vectors reduce lengths")
    return [rng.randbytes(ln) for ln in BOUNDARY_LENGTHS] + [b"\xff" * 8193, b"\xff" * 16384]


def avail_cases() -> list[tuple[int, int]]:
    """(len, avail) for device messages: avail at 0, 1, len-1, len and within +-1 of the start
    and end of a segment, of a chunk, and of a limb (bytes at or beyond avail read as zero)."""
    cases = []
    for ln in (300, SEG_BYTES + 100, 20000):
        cuts = {0, 1, ln - 1, ln}
        end = ln
        while end > 0:
            start = max(0, end - SEG_BYTES)
            nch = (end - start + 255) // 256
            first = (end - start) - 256 * (nch - 1)
            edges = [start, start + first, start + first + 256 if nch > 1 else end, end - 256 if nch > 1 else end,
                     end]
            edges += [start + first - 4, start + first - 8, start + first + 252, end - 4, end - 128]
            for e in edges:
                cuts.update((e - 1, e, e + 1))
            end = start
        cases += [(ln, a) for a in sorted(cuts) if 0 <= a <= ln]
    return cases


# ---- fixed-base powers and tags -------------------------------------------------------------------

def gpow_cases() -> list[tuple[str, int, int]]:
    """(label, width in bytes, exponent): one nonzero byte at position k (no product at all,
    only the product by 1), zero bytes between nonzero ones, leading-zero-padded widths."""
    out = []
    for k in (0, 1, 127, 128, 255):
        for v in (1, 0x80, 0xFF):
            out.append(("byte%d=%02x" % (k, v), 256, v << (8 * k)))
            out.append(("byte%d=%02x:tight" % (k, v), k + 1, v << (8 * k)))
    gaps = [(0, 255), (0, 128), (127, 128), (1, 127), (0, 2, 4, 6), (126, 129), (0, 1, 254, 255)]
    for i, ks in enumerate(gaps):
        e = sum((0x11 * (j + 1) & 0xFF) << (8 * k) for j, k in enumerate(ks))
        out.append(("gap%d" % i, max(ks) + 1, e))
        out.append(("gap%d:padded" % i, 256, e))
    rng = random.Random("bn_vectors gpow")
    for width, pad in ((1, 7), (5, 64), (32, 33), (100, 256), (255, 256)):
        out.append(("pad%d->%d" % (width, pad), pad, rng.getrandbits(8 * width)))
    out += [("zero:1", 1, 0), ("zero:256", 256, 0), ("ones", 256, R - 1)]
    return out


def tag_pieces(n: int) -> list[tuple[str, bytes]]:
    """Pieces whose residue X = piece mod n is zero in its low 128 bytes and nonzero above, and
    the reverse: the tag kernel's two waves split g^X's bytes [0, 128) and [128, 256)."""
    rng = random.Random("bn_vectors tags %x" % n)
    hi = rng.randrange(1, n >> 1024) << 1024
    lo = rng.getrandbits(1024) | 1
    xs = [("high_only", hi), ("low_only", lo), ("zero", 0), ("byte127", 0xA5 << (8 * 127)),
          ("byte128", 0x5A << (8 * 128)), ("byte127+128", 0x0102 << (8 * 127)), ("byte0+255", 1 | (1 << (8 * 255))),
          ("random", rng.randrange(n))]
    out = []
    for label, x in xs:
        assert x < n
        out.append((label, x.to_bytes(256, "big")))
        k = rng.getrandbits(300)
        out.append((label + ":long", (x + k * n).to_bytes(300, "big")))
    return out


if __name__ == "__main__":  # the carry_two search, reproducible on the CPU
    for nm in FULL_NAMES:
        print(repr(nm), search_carry_two(nm))
