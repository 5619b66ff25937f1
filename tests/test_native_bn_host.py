"""CPU: bn_host.hpp (the host bignum that derives sec_apdp_verify_batch's exponents) under
sanitizers, as a stand-alone program: g++ -fsanitize=address,undefined of
tests/native/test_bn_host.cpp, run directly on a file of operands and expected results that this
test writes from Python ints.

The division vectors are built to take each branch of Knuth's Algorithm D with divisors whose top
limb is 0x80000000 and 0xFFFFFFFF: `knuth_branches` below is the algorithm over Python ints, used
only to count which branches a vector takes, so that the test can say on this side that its
vectors reach them; the program asserts that it took them too."""

import os
import random
import shutil
import subprocess

import pytest

from oracle import apdp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_bn_host.cpp")
CSRC = os.path.join(ROOT, "storb_amd", "csrc")
B = 1 << 32


def knuth_branches(u: int, v: int) -> tuple[int, int, int]:
    """(estimates that reached the base, corrections by the second divisor limb, add-backs) of
    Algorithm D dividing u by v in base 2^32; asserts its own remainder."""
    if u < v or v < B:
        return 0, 0, 0
    s = 32 - v.bit_length() % 32 if v.bit_length() % 32 else 0
    n = (v.bit_length() + 31) // 32
    m = (u.bit_length() + 31) // 32
    vn = [((v << s) >> (32 * i)) & (B - 1) for i in range(n)]
    un = [((u << s) >> (32 * i)) & (B - 1) for i in range(m + 1)]
    over = fix = back = 0
    for j in range(m - n, -1, -1):
        num = un[j + n] * B + un[j + n - 1]
        qhat, rhat = divmod(num, vn[n - 1])
        over += qhat >= B
        while qhat >= B or qhat * vn[n - 2] > rhat * B + un[j + n - 2]:
            fix += qhat < B
            qhat -= 1
            rhat += vn[n - 1]
            if rhat >= B:
                break
        part = sum(x << (32 * i) for i, x in enumerate(un[j:j + n + 1])) - qhat * (v << s)
        if part < 0:
            back += 1
            part += v << s
        assert 0 <= part < (v << s)
        for i in range(n + 1):
            un[j + i] = (part >> (32 * i)) & (B - 1)
    assert sum(x << (32 * i) for i, x in enumerate(un)) >> s == u % v
    return over, fix, back


def division_vectors(rng):
    """(u, v) pairs; per top limb of the divisor, ones built for each branch."""
    out = []
    for top in (0x80000000, 0xFFFFFFFF):
        for n in (3, 5, 32):
            # add-back: the estimate 3 fits the divisor's two top limbs (the second is zero), and
            # the low limbs push 3 * v past u
            v = top * B ** (n - 1) + rng.randrange(1, B ** (n - 2))
            for j in (0, 1, 7):
                out.append((3 * top * B ** (n - 1 + j), v))
            # the estimate reaches the base: u's leading limb equals the divisor's
            v2 = top * B ** (n - 1) + (B - 1) * B ** (n - 2) + rng.randrange(B ** (n - 2))
            out.append((top * B ** n + rng.randrange(B ** (n - 2)), v2))
            # corrections by the second limb: common with a small top limb and a large second one
            for _ in range(6):
                out.append((rng.randrange(B ** (2 * n)), v2))
                out.append((rng.randrange(B ** (n + 2)), top * B ** (n - 1) + rng.randrange(B ** (n - 1))))
    return out


def h(x: int) -> str:
    return format(x, "x")


def test_knuth_model_counts_its_branches():
    assert knuth_branches(3 * 0x80000000 * B ** 2, 0x80000000 * B ** 2 + B - 1) == (0, 0, 1)
    assert knuth_branches(5, 7) == (0, 0, 0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_native_bn_host_sanitized(tmp_path):
    rng = random.Random(20)
    n, e, d, p, q = apdp_ref.test_key(11)
    lines = []

    # multiply, subtract, compare
    for wa, wb in [(0, 64), (1, 1), (32, 32), (256, 2048), (2048, 2048), (2048, 256), (33, 95)]:
        a, b = rng.getrandbits(wa), rng.getrandbits(wb)
        lines.append(f"mul {h(a)} {h(b)} {h(a * b)}")
    lines.append(f"mul {h(B ** 64 - 1)} {h(B ** 8 - 1)} {h((B ** 64 - 1) * (B ** 8 - 1))}")
    for a, b in [(B ** 3, 1), (B ** 3 + 5, B ** 3 + 5), (p, 1), (q, 1), (rng.getrandbits(900) + B ** 30, B ** 30)]:
        lines.append(f"sub {h(a)} {h(b)} {h(a - b)}")
    for a, b in [(0, 0), (0, 1), (B, B - 1), (p, q), (q, p), (p, p), (B ** 5, B ** 5 + 1)]:
        lines.append(f"cmp {h(a)} {h(b)} {(a > b) - (a < b) + 1}")

    # remainder: the built branches, per top limb
    reached = {0x80000000: [0, 0, 0], 0xFFFFFFFF: [0, 0, 0]}
    for u, v in division_vectors(rng):
        br = knuth_branches(u, v)
        top = v >> (32 * ((v.bit_length() - 1) // 32))
        reached[top] = [x + y for x, y in zip(reached[top], br)]
        lines.append(f"mod {h(u)} {h(v)} {h(u % v)} {br[0]} {br[1]} {br[2]}")
    for top, counts in reached.items():
        assert all(c > 0 for c in counts), (hex(top), counts)  # every branch, for either top limb
    # even moduli p - 1 / q - 1 (top limb neither of the above: the shift is exercised), a dividend
    # below the divisor, a one-limb divisor, exact multiples, zero
    for m in (p - 1, q - 1):
        for u in (rng.getrandbits(4096), rng.getrandbits(2304), rng.getrandbits(1024) % m, m, m - 1, m + 1,
                  m * rng.getrandbits(900), 0, 1):
            br = knuth_branches(u, m)
            lines.append(f"mod {h(u)} {h(m)} {h(u % m)} {br[0]} {br[1]} {br[2]}")
    for u, v in [(rng.getrandbits(500), 7), (rng.getrandbits(500), B - 1), (p * rng.getrandbits(1000), p),
                 (q * rng.getrandbits(1000) + 1, q), (12345, B ** 4)]:
        br = knuth_branches(u, v)
        lines.append(f"mod {h(u)} {h(v)} {h(u % v)} {br[0]} {br[1]} {br[2]}")

    # the two derivations, against Python for the key: a_h = 0 if t == 0 else (t - 1) % (h - 1) + 1
    # for t = e * s; b_h = (-t) % (h - 1) for t = c * s
    for hh in (p, q):
        m = hh - 1
        ss = [rng.randrange(2, n) for _ in range(6)] + [0, 1, m, 2 * m, (p - 1) * (q - 1), (1 << 2048) - 1]
        for s in ss:
            for ee in (e, 0, 3, (1 << 2048) - 1):
                t = ee * s
                lines.append(f"pos {h(t)} {h(m)} {h(0 if t == 0 else (t - 1) % m + 1)}")
            for c in (rng.getrandbits(256), 0, 1, (1 << 256) - 1, m):
                t = c * s
                lines.append(f"neg {h(t)} {h(m)} {h(-t % m)}")

    # big-endian load / store
    for nbytes, a in [(1, 0), (1, 255), (3, 0x10203), (4, 0x80000000), (5, 0x1122334455), (128, p), (256, n),
                      (256, 1), (288, (1 << 2304) - 1), (32, rng.getrandbits(250))]:
        lines.append(f"be {nbytes} {h(a)}")

    vec = tmp_path / "vectors.txt"
    vec.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "test_bn_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    f"-I{CSRC}", SRC, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "native bn_host tests ok" in r.stdout
