"""Limb-level restatement of storb_amd/csrc/bignum.hip — TEST INFRASTRUCTURE ONLY.

The kernels keep one 2048-bit integer per 64-lane wave, limb j in lane j.  This module
restates their arithmetic the same way: a value is a list of 64 u32 limbs (little-endian),
a ballot or an SGPR carry mask is a Python int of 64 bits.  Every function computes what
its namesake in bignum.hip computes, step by step (same masks, same shifts, same order),
so that a test can ask WHICH data-dependent paths a given operand takes: propagate chains
in the carry-lookahead, where the compare is decided, borrows through equal limbs, the
redundant carries of the hand-scheduled rows.

The model certifies test vectors (tests/bn_vectors.py, tests/test_bn_model.py).  It never
judges the GPU: that is Python's int arithmetic (tests/test_gpu_bn_paths.py).

Events are recorded into a :class:`Collector` per operation (one Montgomery product or one
add_mod), so "event E occurs in at least k products" can be counted.

Event names
  resolve_propagate        a limb equal to 0xFFFFFFFF that receives a carry (resolve)
  resolve_propagate_run8   a run of >= 8 consecutive such limbs
  resolve_carry_out        carry out of limb 63 from resolve
  carry_two                a lane owing two carries (k1 + k2 == 2) after the rows
  p2_carry64               the 64-bit carry-out of p2 = m*n_j + p1_j in some row
  pos64_bit                one of the three position-64 bits (k1, k2, K of lane 63) set
  geq_top                  compare decided by limb 64 (top != 0)
  geq_equal                compare on equality (a == n)
  geq_below63 / below32    compare decided at a limb below 63 / below 32
  geq_limb32               compare decided exactly at limb 32 (a half's value >= 2^1024)
  geq_below31 / below16    the halves' counterparts of below63 / below32 (a 1024-bit value
                           has limbs 32..63 zero, so "below 32" alone says nothing there)
  sub_borrow_equal         a borrow entering a limb where a == n (sub_n)
  final_subtract / no_subtract       the conditional subtract of mont_finish
  add_mod_no_subtract / add_mod_one_subtract / add_mod_two_subtracts
"""

from __future__ import annotations

from collections import namedtuple
from contextlib import contextmanager

LANES = 64
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
BIT63 = 1 << 63
SEG_CHUNKS = 32  # sec::kSegChunks (bignum.hpp): 32 x 256 B per segment

EVENTS = (
    "resolve_propagate", "resolve_propagate_run8", "resolve_carry_out", "carry_two", "p2_carry64", "pos64_bit",
    "geq_top", "geq_equal", "geq_below63", "geq_below32", "geq_limb32", "geq_below31", "geq_below16",
    "sub_borrow_equal", "final_subtract", "no_subtract",
    "add_mod_no_subtract", "add_mod_one_subtract", "add_mod_two_subtracts",
)


class Collector:
    """Path events, grouped by operation.  ops: list of (kind, frozenset of event names);
    kind is "mont64", "mont32" or "add_mod" (events outside an operation go to "loose")."""

    def __init__(self):
        self.ops: list[tuple[str, frozenset]] = []
        self._cur: set | None = None

    def add(self, name: str) -> None:
        assert name in EVENTS, name
        if self._cur is None:
            self.ops.append(("loose", frozenset((name,))))
        else:
            self._cur.add(name)

    @contextmanager
    def op(self, kind: str):
        assert self._cur is None, "operations do not nest in bignum.hip"
        self._cur = set()
        try:
            yield
        finally:
            self.ops.append((kind, frozenset(self._cur)))
            self._cur = None

    def count(self, name: str, kind: str | None = None) -> int:
        """Number of operations (of `kind`, or of any kind) in which `name` occurred."""
        assert name in EVENTS, name
        return sum(1 for k, ev in self.ops if name in ev and (kind is None or k == kind))

    def n_ops(self, kind: str | None = None) -> int:
        return sum(1 for k, _ in self.ops if kind is None or k == kind)

    def counts(self, kind: str | None = None) -> dict:
        return {e: self.count(e, kind) for e in EVENTS}


class _Null:
    def add(self, name):
        pass

    @contextmanager
    def op(self, kind):
        yield


_NULL = _Null()


def limbs(x: int) -> list[int]:
    assert 0 <= x < 1 << (32 * LANES)
    return [(x >> (32 * j)) & M32 for j in range(LANES)]


def value(t) -> int:
    return sum(v << (32 * j) for j, v in enumerate(t))


def ballot(bits) -> int:
    m = 0
    for j, b in enumerate(bits):
        if b:
            m |= 1 << j
    return m


# ---- carry-lookahead, compare, subtract ---------------------------------------------------

def carry_in(G: int, P: int) -> tuple[int, bool]:
    """Carry-in mask of a multi-limb add from its generate / propagate masks, and the carry
    out of limb 63: X = G << 1, S = X + P (64-bit), C = S ^ P."""
    assert G & P == 0
    X = (G << 1) & M64
    S = (X + P) & M64
    out = S < X or bool(G >> 63)
    return S ^ P, out


def resolve(u, ev=_NULL) -> tuple[list[int], int]:
    """Per-limb 64-bit sums u_j (high words 0 or 1) -> normalised 32-bit limbs and the carry
    out of limb 63."""
    assert all(x >> 32 <= 1 for x in u)
    v = [x & M32 for x in u]
    G = ballot(x >> 32 != 0 for x in u)
    P = ballot(x == M32 for x in v)
    C, co = carry_in(G, P)
    hit = C & P
    if hit:
        ev.add("resolve_propagate")
        if _longest_run(hit) >= 8:
            ev.add("resolve_propagate_run8")
    if co:
        ev.add("resolve_carry_out")
    return [(v[j] + ((C >> j) & 1)) & M32 for j in range(LANES)], 1 if co else 0


def _longest_run(mask: int) -> int:
    best = 0
    while mask:
        mask &= mask << 1
        best += 1
    return best


def geq(a, n, top: int, ev=_NULL) -> bool:
    """a >= n where `top` is a's limb 64: decided at the most significant differing limb."""
    if top:
        ev.add("geq_top")
        return True
    ne = ballot(x != y for x, y in zip(a, n))
    if not ne:
        ev.add("geq_equal")
        return True
    h = ne.bit_length() - 1  # 63 - clz
    if h < 63:
        ev.add("geq_below63")
    if h < 32:
        ev.add("geq_below32")
    if h == 32:
        ev.add("geq_limb32")
    if h < 31:
        ev.add("geq_below31")
    if h < 16:
        ev.add("geq_below16")
    return a[h] > n[h]


def sub_n(a, n, ev=_NULL) -> list[int]:
    """(a - n) mod 2^2048 by borrow-lookahead."""
    G = ballot(x < y for x, y in zip(a, n))
    P = ballot(x == y for x, y in zip(a, n))
    B, _ = carry_in(G, P)
    if B & P:
        ev.add("sub_borrow_equal")
    return [(a[j] - n[j] - ((B >> j) & 1)) & M32 for j in range(LANES)]


def mont_finish(t, c, n, ev=_NULL) -> list[int]:
    """value = t + sum_j c_j 2^32(j+1) < 2n  ->  value mod n."""
    top = c[63]
    t, co = resolve([t[j] + (c[j - 1] if j else 0) for j in range(LANES)], ev)
    top += co
    if geq(t, n, top, ev):
        ev.add("final_subtract")
        t = sub_n(t, n, ev)
    else:
        ev.add("no_subtract")
    return t


# ---- Montgomery product: the hand-scheduled rows (SEC_BN_MM == 3) ---------------------------

def mont_rows(a, b, n, n0inv: int, rows: int, ev=_NULL) -> tuple[list[int], int, int]:
    """The `rows` row steps in the asm's carry representation: returns (t, k1, k2) with k1
    (vcc) and k2 (s[48:49]) the lane masks of the two add chains' carry-outs, lane 63's p2
    carry-out K merged into k2's bit 63."""
    assert rows in (64, 32)
    t = [0] * LANES
    k1 = k2 = K = 0
    for i in range(rows):
        ai = a[i]  # v_readlane s40
        p1 = [ai * b[j] + t[j] for j in range(LANES)]  # mad1: never carries out of 64 bits
        assert all(x <= M64 for x in p1)
        assert not (k2 & K & BIT63)
        k2 |= K & BIT63  # lane 63's K of the row before, ahead of k2's next read
        m = ((p1[0] & M32) * n0inv) & M32  # v_readlane s41, s_mul_i32
        p2 = [m * n[j] + p1[j] for j in range(LANES)]  # mad2, carry-outs to K
        K = ballot(x >> 64 for x in p2)
        if K:
            ev.add("p2_carry64")
        Ks = (K << 1) & M64  # s_lshl_b64: lane j takes lane j-1's bit, lane 63's is dropped here
        nk1 = nk2 = 0
        for j in range(LANES):
            lo_next = p2[j + 1] & M32 if j < 63 else 0  # DPP wave_shl:1, bound_ctrl
            s = lo_next + ((p2[j] >> 32) & M32) + ((k1 >> j) & 1)
            nk1 |= (s >> 32) << j
            s = (s & M32) + ((Ks >> j) & 1) + ((k2 >> j) & 1)
            nk2 |= (s >> 32) << j
            t[j] = s & M32
        k1, k2 = nk1, nk2
        pos64 = (k1 >> 63) + (k2 >> 63) + (K >> 63)
        assert pos64 <= 1, "position-64 invariant: the value stays < 2n < 2^2049"
        if pos64:
            ev.add("pos64_bit")
    assert not (k2 & K & BIT63)
    k2 |= K & BIT63
    return t, k1, k2


def mont_mul(a, b, n, n0inv: int, rows: int = 64, ev=_NULL) -> list[int]:
    """a*b*R^-1 mod n, R = 2^(32*rows), for a < R, b < n."""
    with ev.op("mont%d" % rows):
        t, k1, k2 = mont_rows(a, b, n, n0inv, rows, ev)
        c = [((k1 >> j) & 1) + ((k2 >> j) & 1) for j in range(LANES)]
        if 2 in c:
            ev.add("carry_two")
        assert value(t) + sum(cj << (32 * (j + 1)) for j, cj in enumerate(c)) < 2 * value(n)
        return mont_finish(t, c, n, ev)


def add_mod(a, x, n, ev=_NULL) -> list[int]:
    """(a + x) mod n for a < n, x < 2^2048: up to two subtractions."""
    with ev.op("add_mod"):
        t, top = resolve([p + q for p, q in zip(a, x)], ev)
        subs = 0
        for _ in range(2):
            if geq(t, n, top, ev):
                t = sub_n(t, n, ev)
                top = 0
                subs += 1
        ev.add(("add_mod_no_subtract", "add_mod_one_subtract", "add_mod_two_subtracts")[subs])
        return t


# ---- moduli -----------------------------------------------------------------------------

Mod = namedtuple("Mod", "n r2 one n0inv bits")


def neg_inv32(n0: int) -> int:
    """-n^-1 mod 2^32 from n's low limb (api.cpp neg_inv32: Newton steps from x = n0)."""
    x = n0
    for _ in range(4):
        x = (x * (2 - n0 * x)) & M32
    return (-x) & M32


def setup(n_int: int, bits: int = 2048, ev=_NULL) -> Mod:
    """sec_bn_setup_kernel: one = 2^bits - n by borrow-lookahead, R^2 mod n by `bits` modular
    doublings."""
    assert bits in (2048, 1024) and n_int.bit_length() == bits and n_int & 1
    n = limbs(n_int)
    G = ballot(0 < x for x in n)
    P = ballot(x == 0 for x in n)
    B, _ = carry_in(G, P)
    one = [(0 - n[j] - ((B >> j) & 1)) & M32 if 32 * j < bits else 0 for j in range(LANES)]
    r2 = one
    for _ in range(bits):
        r2 = add_mod(r2, r2, n, ev)
    return Mod(n, r2, one, neg_inv32(n[0]), bits)


def make_mod(n_int: int, bits: int = 2048) -> Mod:
    """The same constants from Python ints (quick; for tests that do not study setup)."""
    R = 1 << bits
    return Mod(limbs(n_int), limbs(R * R % n_int), limbs(R % n_int), (-pow(n_int, -1, 1 << 32)) & M32, bits)


def mmul(M: Mod, a, b, rows: int = 64, ev=_NULL) -> list[int]:
    return mont_mul(a, b, M.n, M.n0inv, rows, ev)


ONE_PLAIN = [1] + [0] * 63  # the `l == 0 ? 1 : 0` operand that leaves Montgomery form


def mulmod(M: Mod, a, b, ev=_NULL) -> list[int]:
    """sec_bn_mulmod_kernel: am = mont(a, R^2), out = mont(b, am)."""
    return mmul(M, b, mmul(M, a, M.r2, 64, ev), 64, ev)


# ---- exponentiation schedules -----------------------------------------------------------

def mont_pow_schedule(nnib: int, nib) -> list[tuple]:
    """The products mont_pow performs for an exponent of `nnib` nibbles (nib(i), i counted
    from the least significant): ("table", w) for w = 2..15, then ("load", v) or
    ("load_one",) for the leading digit, then ("square",) x4 and ("times", v) per digit."""
    ops = [("table", w) for w in range(2, 16)]
    i = nnib
    started = False
    while i > 0:
        i -= 1
        v = nib(i)
        if v:
            ops.append(("load", v))
            started = True
            break
    if not started:
        ops.append(("load_one",))
    while i > 0:
        v = nib(i - 1)
        ops += [("square",)] * 4
        if v:
            ops.append(("times", v))
        i -= 1
    return ops


def exp_nibbles(e: int, exp_bytes: int):
    """nib(k) of a big-endian exponent of exp_bytes bytes, as the modexp kernels read it."""
    be = e.to_bytes(exp_bytes, "big")

    def nib(k):
        byte = be[exp_bytes - 1 - k // 2]
        return byte >> 4 if k & 1 else byte & 15

    return nib


def mont_pow(M: Mod, base_m, nnib: int, nib, rows: int = 64, ev=_NULL) -> list[int]:
    """4-bit fixed window in Montgomery form, product for product as mont_pow in bignum.hip."""
    tab = [M.one, base_m]
    x = base_m
    for _ in range(2, 16):
        x = mmul(M, x, base_m, rows, ev)
        tab.append(x)
    r = M.one
    for op in mont_pow_schedule(nnib, nib)[14:]:
        if op[0] == "load":
            r = tab[op[1]]
        elif op[0] == "square":
            r = mmul(M, r, r, rows, ev)
        elif op[0] == "times":
            r = mmul(M, r, tab[op[1]], rows, ev)
    return r


def modexp(M: Mod, base, e: int, exp_bytes: int, ev=_NULL) -> list[int]:
    """sec_bn_modexp_kernel (keep e short: every product is a few milliseconds here)."""
    bm = mmul(M, base, M.r2, 64, ev)
    r = mont_pow(M, bm, 2 * exp_bytes, exp_nibbles(e, exp_bytes), 64, ev)
    return mmul(M, r, ONE_PLAIN, 64, ev)


def fixed_pow_schedule(nbytes: int, byte, k0: int = 0, k1: int | None = None) -> list[tuple]:
    """Table entries (k, v) fixed_pow touches for bytes [k0, k1) of the exponent (byte(k), k
    from the least significant): the first is loaded, each later one is one product.  An
    empty list means the result is Montgomery 1 and no product runs."""
    k1 = nbytes if k1 is None else min(k1, nbytes)
    return [(k, byte(k)) for k in range(k0, k1) if byte(k)]


# ---- reductions ---------------------------------------------------------------------------

def chunk_limbs(msg: bytes, start: int, length: int, avail: int) -> list[int]:
    """chunk_limb for every lane: bytes [start, start+length) of msg as a big-endian integer,
    bytes at or beyond `avail` reading as zero."""
    out = []
    for l in range(LANES):
        end = start + length - 4 * l
        v = 0
        for b in range(4):
            pos = end - 4 + b
            v = (v << 8) | (msg[pos] if start <= pos < avail else 0)
        out.append(v)
    return out


def horner_step(M: Mod, r, x, first: bool, ev=_NULL) -> list[int]:
    """r <- r * 2^2048 + x mod n: mont(r, R^2) then add_mod (the product is skipped for the
    first chunk)."""
    if not first:
        r = mmul(M, r, M.r2, 64, ev)
    return add_mod(r, x, M.n, ev)


def reduce_msg(M: Mod, msg: bytes, avail: int | None = None, ev=_NULL) -> list[int]:
    """int.from_bytes(msg, "big") mod n by Horner over 256-byte chunks (one segment)."""
    avail = len(msg) if avail is None else avail
    r = [0] * LANES
    if not msg:
        return r
    nch = (len(msg) + 255) // 256
    first = len(msg) - 256 * (nch - 1)
    off = 0
    for c in range(nch):
        clen = first if c == 0 else 256
        r = horner_step(M, r, chunk_limbs(msg, off, clen, avail), c == 0, ev)
        off += clen
    return r


def reduce_segmented(M: Mod, msg: bytes, avail: int | None = None, ev=_NULL) -> list[int]:
    """sec_bn_reduce_seg_kernel + sec_bn_reduce_sum_kernel: 8 KiB segments from the least
    significant end, each times R^(32 j) (taken from Python ints here; the kernel raises it
    with mont_pow), summed with add_mod."""
    avail = len(msg) if avail is None else avail
    n_int = value(M.n)
    seg = SEG_CHUNKS * 256
    nseg = max(1, (len(msg) + seg - 1) // seg)
    acc = [0] * LANES
    for j in range(nseg):
        end = len(msg) - j * seg
        start = max(0, end - seg)
        r = reduce_msg(M, msg[start:end], max(0, min(avail - start, end - start)), ev)
        if j:
            r = mmul(M, r, limbs(pow(1 << 2048, SEG_CHUNKS * j + 1, n_int)), 64, ev)
        acc = add_mod(acc, r, M.n, ev)
    return acc


# ---- CRT halves -----------------------------------------------------------------------------

def high_half(x) -> list[int]:
    return [x[j + 32] if j < 32 else 0 for j in range(LANES)]


def low_half(x) -> list[int]:
    return [x[j] if j < 32 else 0 for j in range(LANES)]


def to_half_m(H: Mod, x, ev=_NULL) -> list[int]:
    """x (< 2^2048, plain) mod a 1024-bit half, in the half's Montgomery form."""
    r = add_mod(mmul(H, high_half(x), H.r2, 32, ev), low_half(x), H.n, ev)
    return mmul(H, r, H.r2, 32, ev)


def crt_half(N: Mod, H: Mod, weight_m, x, nnib: int, nib, ev=_NULL) -> list[int]:
    """(x mod h)^e_h times the half's CRT weight (cp or cq, Montgomery form mod n)."""
    rm = mont_pow(H, to_half_m(H, x, ev), nnib, nib, 32, ev)
    t = mmul(H, rm, ONE_PLAIN, 32, ev)
    return mmul(N, t, weight_m, 64, ev)
