// bn_host.hpp — a small host bignum for the exponent arithmetic of sec_apdp_verify_batch: what
// a caller used to derive itself before the CRT calls (exponents reduced per factor, the
// invertibility of F mod p and q).  Non-negative integers as little-endian 32-bit limbs without
// leading zero limbs (zero is the empty vector).  Header-only, <cstdint> and <vector> alone, so
// it also compiles into a stand-alone test program (tests/native/test_bn_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sec {
namespace bnh {

using Limbs = std::vector<uint32_t>;

inline void trim(Limbs &a)
{
    while (!a.empty() && a.back() == 0)
        a.pop_back();
}

inline bool is_zero(const Limbs &a) { return a.empty(); }

// big-endian bytes -> limbs (any length)
inline Limbs load_be(const uint8_t *be, size_t nbytes)
{
    Limbs a((nbytes + 3) / 4, 0u);
    for (size_t i = 0; i < nbytes; ++i)
        a[i / 4] |= (uint32_t)be[nbytes - 1 - i] << (8 * (i % 4));
    trim(a);
    return a;
}

// limbs -> nbytes big-endian bytes, zero-padded; false (nothing written) when a does not fit
inline bool store_be(const Limbs &a, uint8_t *be, size_t nbytes)
{
    for (size_t i = 0; i < a.size(); ++i)
        for (size_t b = 0; b < 4; ++b)
            if (4 * i + b >= nbytes && ((a[i] >> (8 * b)) & 0xFFu))
                return false;
    for (size_t i = 0; i < nbytes; ++i)
        be[nbytes - 1 - i] = i / 4 < a.size() ? (uint8_t)(a[i / 4] >> (8 * (i % 4))) : (uint8_t)0;
    return true;
}

// -1, 0, 1 for a < b, a == b, a > b (both trimmed)
inline int cmp(const Limbs &a, const Limbs &b)
{
    if (a.size() != b.size())
        return a.size() < b.size() ? -1 : 1;
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i])
            return a[i] < b[i] ? -1 : 1;
    return 0;
}

// a - b for a >= b
inline Limbs sub(const Limbs &a, const Limbs &b)
{
    Limbs r(a.size());
    uint64_t borrow = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        const uint64_t d = (uint64_t)a[i] - (i < b.size() ? b[i] : 0u) - borrow;
        r[i] = (uint32_t)d;
        borrow = d >> 63;
    }
    trim(r);
    return r;
}

inline Limbs mul(const Limbs &a, const Limbs &b)
{
    if (a.empty() || b.empty())
        return Limbs();
    Limbs r(a.size() + b.size(), 0u);
    for (size_t i = 0; i < a.size(); ++i) {
        uint64_t carry = 0;
        for (size_t j = 0; j < b.size(); ++j) {
            const uint64_t t = (uint64_t)a[i] * b[j] + r[i + j] + carry;
            r[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        r[i + b.size()] = (uint32_t)carry;
    }
    trim(r);
    return r;
}

// Which of Knuth's division branches a call of mod() took (for the tests)
struct DivStats {
    uint64_t qhat_overflow = 0;  // the estimate reached the base (top limbs equal)
    uint64_t qhat_fix = 0;       // corrections by the second divisor limb
    uint64_t add_back = 0;       // the rare step D6: the estimate was still one too large
};

// u mod v for v != 0 (v == 0 returns u): Knuth's Algorithm D (TAOCP 4.3.1) without the quotient.
inline Limbs mod(Limbs u, Limbs v, DivStats *st = nullptr)
{
    trim(u);
    trim(v);
    if (v.empty() || cmp(u, v) < 0)
        return u;
    const size_t n = v.size(), m = u.size();
    if (n == 1) {
        uint64_t r = 0;
        for (size_t i = m; i-- > 0;)
            r = ((r << 32) | u[i]) % v[0];
        Limbs out(1, (uint32_t)r);
        trim(out);
        return out;
    }
    int s = 0;  // D1: shift so that the divisor's top bit is set
    while (!((v[n - 1] << s) & 0x80000000u))
        ++s;
    Limbs vn(n), un(m + 1);
    for (size_t i = n; i-- > 0;)
        vn[i] = (v[i] << s) | (s && i ? (uint32_t)((uint64_t)v[i - 1] >> (32 - s)) : 0u);
    un[m] = s ? (uint32_t)((uint64_t)u[m - 1] >> (32 - s)) : 0u;
    for (size_t i = m; i-- > 0;)
        un[i] = (u[i] << s) | (s && i ? (uint32_t)((uint64_t)u[i - 1] >> (32 - s)) : 0u);
    const uint64_t B = (uint64_t)1 << 32;
    for (size_t j = m - n + 1; j-- > 0;) {
        // D3: estimate the quotient digit from the top two limbs, correct it by the third
        const uint64_t num = ((uint64_t)un[j + n] << 32) | un[j + n - 1];
        uint64_t qhat = num / vn[n - 1], rhat = num % vn[n - 1];
        if (st && qhat >= B)
            ++st->qhat_overflow;
        while (qhat >= B || qhat * vn[n - 2] > ((rhat << 32) | un[j + n - 2])) {
            if (st && qhat < B)
                ++st->qhat_fix;
            --qhat;
            rhat += vn[n - 1];
            if (rhat >= B)
                break;
        }
        // D4: multiply and subtract
        uint64_t carry = 0, borrow = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t p = qhat * vn[i] + carry;
            carry = p >> 32;
            const uint64_t d = (uint64_t)un[i + j] - (uint32_t)p - borrow;
            un[i + j] = (uint32_t)d;
            borrow = d >> 63;
        }
        const uint64_t d = (uint64_t)un[j + n] - carry - borrow;
        un[j + n] = (uint32_t)d;
        if (d >> 63) {  // D6: add the divisor back
            if (st)
                ++st->add_back;
            uint64_t c = 0;
            for (size_t i = 0; i < n; ++i) {
                const uint64_t t = (uint64_t)un[i + j] + vn[i] + c;
                un[i + j] = (uint32_t)t;
                c = t >> 32;
            }
            un[j + n] += (uint32_t)c;
        }
    }
    Limbs r(n);  // D8: undo the shift
    for (size_t i = 0; i < n; ++i)
        r[i] = (un[i] >> s) | (s ? (uint32_t)((uint64_t)un[i + 1] << (32 - s)) : 0u);
    trim(r);
    return r;
}

// The exponents sec_apdp_verify_batch derives for a prime factor h of n, from hm1 = h - 1:
//
// x^t mod h for every x, multiples of h included: 0 when t is 0, else the value in [1, h - 1]
// congruent to t mod h - 1, that is (t - 1) mod (h - 1) + 1
inline Limbs pos_exp(const Limbs &t, const Limbs &hm1)
{
    if (is_zero(t))
        return Limbs();
    const Limbs r = mod(t, hm1);
    return is_zero(r) ? hm1 : r;
}

// x^(-t) mod h for x invertible mod h: (-t) mod (h - 1)
inline Limbs neg_exp(const Limbs &t, const Limbs &hm1)
{
    const Limbs r = mod(t, hm1);
    return is_zero(r) ? r : sub(hm1, r);
}

}  // namespace bnh
}  // namespace sec
