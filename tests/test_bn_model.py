"""CPU: the limb-level model of bignum.hip (oracle/bn_model.py) equals Python ints, and the
vector families of tests/bn_vectors.py reach the kernels' data-dependent paths.

Two kinds of assertion:
  * the model computes a*b/R mod n (64 and 32 rows), (a + x) mod n, x mod h and the entry
    points built from them exactly, on every vector and on seeded random operands;
  * coverage: run over the shipped vectors, the model records each named path event in at
    least MIN_HITS products.  These conditions are about the vectors, not about the GPU: the
    same operands go through the kernels in tests/test_gpu_bn_paths.py, judged by Python ints.

An event that a modulus cannot reach, or that the vectors do not reach, is listed in the
tables below with its reason, and the test checks that the listing is still true.
"""

import functools
import random

import pytest

from oracle import bn_model as bm
from tests import bn_vectors as bv

R, RH = bv.R, bv.RH
MIN_HITS = 3

# required in >= MIN_HITS products of the mulmod family (64 rows) for every full modulus
FULL_EVENTS = ("resolve_propagate", "resolve_propagate_run8", "geq_below63", "geq_below32", "geq_equal", "geq_top",
               "sub_borrow_equal", "final_subtract", "no_subtract", "p2_carry64", "pos64_bit")
# required in >= MIN_HITS 32-row products for every factor pair.  A half's limbs 32..63 are
# zero, so geq_below63 / geq_below32 say little there: geq_below31 / geq_below16 are their
# counterparts, and geq_limb32 (the value reaches 2^1024) is the counterpart of geq_top.
HALF_EVENTS = ("resolve_propagate", "resolve_propagate_run8", "geq_below63", "geq_below32", "geq_below31",
               "geq_below16", "geq_equal", "geq_limb32", "sub_borrow_equal", "final_subtract", "no_subtract",
               "p2_carry64")

_TOP_PLUS_ONE = "n = 2^2047+1 has limbs 1, 0.., 2^31: m*n_j + p1_j stays below 2^64 and the value below 2^2048+2"
UNREACHED_FULL = {
    "top_plus_one": {"p2_carry64": _TOP_PLUS_ONE, "pos64_bit": _TOP_PLUS_ONE, "geq_top": _TOP_PLUS_ONE},
}
_TINY_R2 = ("R^2 mod h is tiny (h within 2^32 of 2^1024), so the conversion products exceed h by less than that "
            "and subtract without a borrow chain; a general product with a chosen result needs a modular root")
UNREACHED_HALF = {
    "p105": {"sub_borrow_equal": _TINY_R2},
    "ones": {"sub_borrow_equal": _TINY_R2},
}
# never in a 32-row product, for any pair: lane 63 holds nothing
HALF_NEVER = {"geq_top": "limbs 32..63 of a half are zero: no limb 64",
              "resolve_carry_out": "limbs 32..63 of a half are zero: no carry out of limb 63",
              "pos64_bit": "limbs 32..63 of a half are zero: position 64 is never reached"}


def report(title, counts, required, unreached=()):
    lines = ["%-24s %5d%s" % (e, counts[e], "   (listed: not reached)" if e in unreached else "")
             for e in required]
    print("\n%s\n  %s" % (title, "\n  ".join(lines)))
    missing = [(e, counts[e]) for e in required if e not in unreached and counts[e] < MIN_HITS]
    assert not missing, "%s: events below %d hits: %s" % (title, MIN_HITS, missing)
    stale = [(e, counts[e]) for e in unreached if counts[e] >= MIN_HITS]
    assert not stale, "%s: listed as not reached but reached: %s" % (title, stale)


@functools.lru_cache(maxsize=None)
def full_mod(name):
    return bm.make_mod(bv.modulus(name))


@functools.lru_cache(maxsize=None)
def half_mods(name):
    p, q = bv.pair(name)
    return bm.make_mod(p, 1024), bm.make_mod(q, 1024)


# ---- the pieces against ints --------------------------------------------------------------------

def test_moduli_and_pairs_are_what_the_families_assume():
    for name in bv.FULL_NAMES:
        n = bv.modulus(name)
        assert n.bit_length() == 2048 and n & 1, name
        assert bm.neg_inv32(n & bm.M32) == (-pow(n, -1, 1 << 32)) % (1 << 32)
    assert len({bv.modulus(name) for name in bv.FULL_NAMES}) == len(bv.FULL_NAMES)
    assert full_mod("low_ones").n[:32] == [bm.M32] * 32 and full_mod("low_ones").n0inv == 1
    assert full_mod("limb0_one").n[0] == 1 and full_mod("limb0_one").n0inv == bm.M32
    for name in bv.PAIR_NAMES:
        bv.pair(name)  # asserts widths, oddness, gcd = 1, 2048-bit product
    assert set(bv.CARRY_TWO) | set(bv.CARRY_TWO_NOT_FOUND) == set(bv.FULL_NAMES)
    assert not set(bv.CARRY_TWO) & set(bv.CARRY_TWO_NOT_FOUND)


def test_carry_lookahead_compare_subtract_random():
    rng = random.Random(1)
    for _ in range(300):
        G = rng.getrandbits(64) & rng.getrandbits(64)
        P = rng.getrandbits(64) & ~G & (rng.getrandbits(64) | -(rng.random() < 0.5))
        C, out = bm.carry_in(G, P)
        c = 0
        for j in range(64):  # ripple reference
            assert (C >> j) & 1 == c
            c = 1 if (G >> j) & 1 else (c if (P >> j) & 1 else 0)
        assert out == bool(c)
    for i in range(300):
        digits = i % 2
        a = bv.from_digits(bv.structured_digits(rng)) if digits else rng.getrandbits(2048)
        b = bv.from_digits(bv.structured_digits(rng)) if digits else rng.getrandbits(2048)
        t, co = bm.resolve([x + y for x, y in zip(bm.limbs(a), bm.limbs(b))])
        assert bm.value(t) + (co << 2048) == a + b
        for top in (0, 1):
            assert bm.geq(bm.limbs(a), bm.limbs(b), top) == ((top << 2048) + a >= b)
        assert bm.geq(bm.limbs(a), bm.limbs(a), 0)
        assert bm.value(bm.sub_n(bm.limbs(a), bm.limbs(b))) == (a - b) % R


@pytest.mark.parametrize("name", bv.FULL_NAMES)
def test_setup_derives_the_key_constants(name):
    assert bm.setup(bv.modulus(name)) == full_mod(name)


@pytest.mark.parametrize("name", bv.PAIR_NAMES)
def test_setup_derives_the_half_constants(name):
    for h, M in zip(bv.pair(name), half_mods(name)):
        assert bm.setup(h, 1024) == M
        assert M.n[32:] == M.r2[32:] == M.one[32:] == [0] * 32


def test_random_products_both_row_counts():
    rng = random.Random(2)
    mods = [(bv.modulus(name), 2048) for name in bv.FULL_NAMES]
    mods += [(h, 1024) for name in bv.PAIR_NAMES for h in bv.pair(name)]
    for m, bits in mods:
        M = bm.make_mod(m, bits)
        Rr = 1 << bits
        for _ in range(6):
            a, b = rng.randrange(Rr), rng.randrange(m)
            got = bm.value(bm.mont_mul(bm.limbs(a), bm.limbs(b), M.n, M.n0inv, bits // 32))
            assert got == a * b * pow(Rr, -1, m) % m


@pytest.mark.parametrize("bits", [2048, 1024])
def test_add_mod_lands_on_targets(bits):
    """(a + x) mod n with the sum chosen: T, T + n and T + 2n."""
    mods = [bv.modulus(n) for n in bv.FULL_NAMES] if bits == 2048 else [h for n in bv.PAIR_NAMES for h in bv.pair(n)]
    rng = random.Random(bits)
    ev = bm.Collector()
    for m in mods:
        nl = bm.limbs(m)
        for i, (label, t) in enumerate(bv.targets(m, bits)[::2]):
            k = i % 3
            a = (m - 1 - rng.getrandbits(32)) if k == 2 else rng.randrange(m)
            x = t + k * m - a
            while x < 0:
                x += m
            while x >= 1 << bits:
                x -= m
            if x < 0:
                continue
            assert bm.value(bm.add_mod(bm.limbs(a), bm.limbs(x), nl, ev)) == (a + x) % m == t, label
        a = rng.randrange(1, m)  # the sum is exactly n, and exactly 2n where x = 2n - a fits
        for x in (m - a, 2 * m - (m - 1)):
            if x < 1 << bits:
                a = a if x == m - a else m - 1
                assert bm.value(bm.add_mod(bm.limbs(a), bm.limbs(x), nl, ev)) == 0
    counts = ev.counts("add_mod")
    report("add_mod, %d-bit moduli" % bits, counts,
           ("resolve_propagate", "resolve_propagate_run8", "geq_equal", "geq_below32", "geq_below16",
            "sub_borrow_equal", "add_mod_no_subtract", "add_mod_one_subtract", "add_mod_two_subtracts"))


# ---- mulmod family: values and coverage, per full modulus ----------------------------------------

@functools.lru_cache(maxsize=None)
def run_mulmod(name):
    m, M = bv.modulus(name), full_mod(name)
    ev = bm.Collector()
    bad = [label for label, a, b in bv.mulmod_vectors(name)
           if bm.value(bm.mulmod(M, bm.limbs(a), bm.limbs(b), ev)) != a * b % m]
    return ev, bad


@pytest.mark.parametrize("name", bv.FULL_NAMES)
def test_mulmod_family_matches_ints_and_reaches_paths(name):
    ev, bad = run_mulmod(name)
    assert not bad
    assert ev.n_ops("mont64") == 2 * len(bv.mulmod_vectors(name))
    report("mulmod family, modulus %s: products with the event (of %d)" % (name, ev.n_ops("mont64")),
           ev.counts("mont64"), FULL_EVENTS, UNREACHED_FULL.get(name, {}))


def test_carry_out_of_limb_63_on_a_top_heavy_modulus():
    counts = {name: run_mulmod(name)[0].count("resolve_carry_out", "mont64") for name in bv.TOP_HEAVY}
    print("\nresolve_carry_out in the mulmod family:", counts)
    assert max(counts.values()) >= MIN_HITS, counts


def test_carry_two_vectors_found_by_search():
    """The committed vectors (bv.CARRY_TWO, found by bv.search_carry_two with the seed and bound
    recorded there) do make a lane owe two carries; the moduli where the bounded search found
    none are listed in bv.CARRY_TWO_NOT_FOUND."""
    total = 0
    for name, vecs in bv.CARRY_TWO.items():
        assert vecs
        for a, b in vecs:
            ev = bm.Collector()
            bm.mulmod(full_mod(name), bm.limbs(bv.from_digits(a)), bm.limbs(bv.from_digits(b)), ev)
            assert ev.count("carry_two", "mont64") >= 1, (name, a, b)
            total += 1
    family = {name: run_mulmod(name)[0].count("carry_two", "mont64") for name in bv.FULL_NAMES}
    print("\ncarry_two in the mulmod family:", family, "committed vectors:", total)
    assert total >= 1 and all(family[name] >= 1 for name in bv.CARRY_TWO)


def test_carry_two_search_is_reproducible():
    """A short prefix of the recorded search finds the first committed vector again."""
    name = "ones_minus_mid"
    assert tuple(bv.search_carry_two(name, keep=1)) == bv.CARRY_TWO[name][:1]


def _no_propagate(G, P):  # carry-lookahead that forgets the propagate limbs
    return (G << 1) & bm.M64, bool(G >> 63)


def _geq_equal_is_less(a, n, top, ev=None):  # the compare with its equality case wrong
    return bool(top) or a != n and bm.value(a) > bm.value(n)


def _sub_without_chain(a, n, ev=None):  # a borrow that stops at an equal limb
    G = bm.ballot(x < y for x, y in zip(a, n))
    return [(a[j] - n[j] - (((G << 1) >> j) & 1)) & bm.M32 for j in range(bm.LANES)]


@pytest.mark.parametrize("fn,broken", [("carry_in", _no_propagate), ("geq", _geq_equal_is_less),
                                       ("sub_n", _sub_without_chain)])
def test_vectors_catch_what_random_operands_miss(monkeypatch, fn, broken):
    """The point of the families: with one path of the model broken, 40 seeded random products
    on the key modulus still all agree with Python ints, and the mulmod family does not."""
    m, M = bv.modulus("key"), full_mod("key")
    monkeypatch.setattr(bm, fn, broken)
    rng = random.Random(fn)
    for _ in range(20):
        a, b = rng.randrange(R), rng.randrange(R)
        assert bm.value(bm.mulmod(M, bm.limbs(a), bm.limbs(b))) == a * b % m
    caught = None
    for label, a, b in bv.mulmod_vectors("key"):
        if bm.value(bm.mulmod(M, bm.limbs(a), bm.limbs(b))) != a * b % m:
            caught = label
            break
    print("\nbroken %s first caught by %s" % (fn, caught))
    assert caught is not None


# ---- 32-row products: values and coverage, per factor pair ---------------------------------------

@functools.lru_cache(maxsize=None)
def run_half_sites(name):
    """Replays the one 32-row product (and add_mod) each CRT vector aims at."""
    hs = bv.pair(name)
    H = half_mods(name)
    ev = bm.Collector()
    bad = []
    for it in bv.crt_vectors(name):
        for site in it["site"]:
            h, what = site[0], site[1]
            hm, M = hs[h], H[h]
            if what == "by_one":  # leaving Montgomery form
                got, want = bm.mmul(M, bm.limbs(site[2]), bm.ONE_PLAIN, 32, ev), site[2] * pow(RH, -1, hm) % hm
            elif what == "to_mont":
                got, want = bm.mmul(M, bm.limbs(site[2]), M.r2, 32, ev), site[2] * RH % hm
            elif what == "square":
                got = bm.mmul(M, bm.limbs(site[2]), bm.limbs(site[2]), 32, ev)
                want = site[2] * site[2] * pow(RH, -1, hm) % hm
            else:  # "hi": to_half_m's first product and its add_mod
                hi, lo = site[2], site[3]
                got = bm.add_mod(bm.mmul(M, bm.limbs(hi), M.r2, 32, ev), bm.limbs(lo), M.n, ev)
                want = (hi << 1024 | lo) % hm
            if bm.value(got) != want:
                bad.append(it["label"])
    return ev, bad


@pytest.mark.parametrize("name", bv.PAIR_NAMES)
def test_half_products_match_ints_and_reach_paths(name):
    ev, bad = run_half_sites(name)
    assert not bad
    counts = ev.counts("mont32")
    report("CRT family, pair %s: 32-row products with the event (of %d)" % (name, ev.n_ops("mont32")),
           counts, HALF_EVENTS, UNREACHED_HALF.get(name, {}))
    assert all(counts[e] == 0 for e in HALF_NEVER), counts
    report("CRT family, pair %s: add_mod of to_half_m (of %d)" % (name, ev.n_ops("add_mod")), ev.counts("add_mod"),
           ("resolve_propagate", "geq_below16", "geq_limb32", "sub_borrow_equal", "add_mod_no_subtract",
            "add_mod_one_subtract"))


@pytest.mark.parametrize("name", bv.PAIR_NAMES)
def test_to_half_m_and_whole_crt_items(name):
    """x mod h through to_half_m and the product by 1, and whole crt_powmod_pq items (short
    exponents) through both halves and the final add_mod."""
    p, q = bv.pair(name)
    Hp, Hq = half_mods(name)
    N = bm.make_mod(p * q)
    items = bv.crt_vectors(name)
    for it in items[::61]:
        x = bm.limbs(it["x"])
        for hm, H in ((p, Hp), (q, Hq)):
            assert bm.value(bm.mmul(H, bm.to_half_m(H, x), bm.ONE_PLAIN, 32)) == it["x"] % hm, it["label"]
    cp = bm.limbs(q * pow(q, -1, p) % (p * q) * R % (p * q))
    cq = bm.limbs(p * pow(p, -1, q) % (p * q) * R % (p * q))
    short = [it for it in items if it["kind"] == "exps" and max(it["ep"], it["eq"]) < 1 << 16][:3] + [items[0]]
    for it in short:
        x = bm.limbs(it["x"])
        yp = bm.crt_half(N, Hp, cp, x, 4, bm.exp_nibbles(it["ep"], 2))
        yq = bm.crt_half(N, Hq, cq, x, 4, bm.exp_nibbles(it["eq"], 2))
        assert bm.value(bm.add_mod(yp, yq, N.n)) == bv.crt_expected(name, it["x"], it["ep"], it["eq"]), it["label"]


# ---- reduce family ---------------------------------------------------------------------------------

_ONES_TWO = "a + x <= (n - 1) + (2^2048 - 1) < 2n for n = 2^2048 - 1"
UNREACHED_REDUCE = {"ones": {"add_mod_two_subtracts": _ONES_TWO}}


@pytest.mark.parametrize("name", bv.FULL_NAMES)
def test_reduce_two_chunk_family(name):
    m, M = bv.modulus(name), full_mod(name)
    ev = bm.Collector()
    for label, msg, (r, chunk) in bv.reduce_two_chunk(name):
        assert 257 <= len(msg) <= 512
        assert bm.value(bm.reduce_msg(M, msg, None, ev)) == int.from_bytes(msg, "big") % m == (r * R + chunk) % m, label
    report("reduce family, modulus %s: add_mod with the event (of %d)" % (name, ev.n_ops("add_mod")),
           ev.counts("add_mod"),
           ("resolve_propagate", "resolve_propagate_run8", "resolve_carry_out", "geq_top", "geq_below32",
            "sub_borrow_equal", "add_mod_no_subtract", "add_mod_one_subtract", "add_mod_two_subtracts"),
           UNREACHED_REDUCE.get(name, {}))


def test_reduce_segments_and_zero_tails():
    """Segment boundaries (up to two segments here: the longer ones run on the GPU only) and
    `avail` cut at chunk and limb edges, through the segmented reduction."""
    m, M = bv.modulus("key"), full_mod("key")
    for msg in bv.reduce_boundary_messages():
        if len(msg) <= 8193:
            assert bm.value(bm.reduce_segmented(M, msg)) == int.from_bytes(msg, "big") % m, len(msg)
    rng = random.Random(8)
    data = rng.randbytes(300)
    for ln, av in bv.avail_cases():
        if ln == 300:
            want = int.from_bytes(data[:av] + b"\0" * (ln - av), "big") % m
            assert bm.value(bm.reduce_segmented(M, data, av)) == want, (ln, av)
    cases = bv.avail_cases()
    assert {ln for ln, _ in cases} == {300, bv.SEG_BYTES + 100, 20000}
    for ln in (300, bv.SEG_BYTES + 100, 20000):
        avs = {a for l, a in cases if l == ln}
        assert {0, 1, ln - 1, ln} <= avs
        assert {ln - bv.SEG_BYTES + d for d in (-1, 0, 1) if ln > bv.SEG_BYTES} <= avs


# ---- exponentiation schedules -----------------------------------------------------------------------

def test_short_modexp_matches_pow():
    m, M = bv.modulus("key"), full_mod("key")
    vecs = [v for v in bv.powmod_vectors("key") if v[2] < 1 << 16]
    for label, base, e in vecs[::23]:
        assert bm.value(bm.modexp(M, bm.limbs(base), e, 2)) == pow(base, e, m), label


def test_window_schedule_of_the_exponent_shapes():
    """Which products a short powmod call performs: 14 table products, then 4 squarings per
    nibble below the leading one and one more product per nonzero nibble among them."""
    for label, e in bv.exponent_shapes():
        ops = bm.mont_pow_schedule(8, bm.exp_nibbles(e, 4))
        assert ops[:14] == [("table", w) for w in range(2, 16)]
        nibs = [(e >> (4 * k)) & 15 for k in range(8)]
        lead = max((k for k in range(8) if nibs[k]), default=None)
        rest = ops[14:]
        if lead is None:
            assert rest == [("load_one",)], label
            continue
        assert rest[0] == ("load", nibs[lead]), label
        assert rest.count(("square",)) == 4 * lead, label
        assert [op[1] for op in rest[1:] if op[0] == "times"] == [nibs[k] for k in range(lead - 1, -1, -1) if nibs[k]]
    wide = bm.mont_pow_schedule(8192, bm.exp_nibbles(bv.WIDE_EXP, 4096))
    assert wide[14] == ("load", 8) and wide[15:] == [("square",)] * (4 * 8191)


def test_fixed_base_schedule_of_the_gpow_cases():
    """One nonzero byte: its table entry is loaded and no product runs before the product by
    1; zero bytes between nonzero ones are skipped; the tag kernel's two waves take bytes
    [0, 128) and [128, 256)."""
    for label, width, e in bv.gpow_cases():
        be = e.to_bytes(width, "big")
        entries = bm.fixed_pow_schedule(width, lambda k: be[width - 1 - k])
        assert entries == [(k, (e >> (8 * k)) & 255) for k in range(width) if (e >> (8 * k)) & 255], label
        if label.startswith("byte"):
            assert len(entries) == 1
    n = bv.modulus("key")
    for label, piece in bv.tag_pieces(n):
        x = int.from_bytes(piece, "big") % n
        xb = x.to_bytes(256, "little")
        low = bm.fixed_pow_schedule(256, lambda k: xb[k], 0, 128)
        high = bm.fixed_pow_schedule(256, lambda k: xb[k], 128, 256)
        if label.startswith("high_only"):
            assert not low and high
        if label.startswith("low_only"):
            assert low and not high
        if label.startswith("zero"):
            assert not low and not high
