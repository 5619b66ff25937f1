// gf_host.hpp — host-side GF(2^8) matrix arithmetic for the C ABI.
//
// O(k^3) set-up work only (the byte streams never touch the CPU):
//   * the systematic encode matrix zfec's fec_new builds (zfec 1.6.0.0, called
//     via easyfec.Encoder at /root/reference/storb/util/piece.py:129): seed
//     rows tmp[0] = [1,0..0], tmp[r][c] = alpha^((r-1)c mod 255), then
//     enc[k..m-1] = tmp[k..m-1] * inv(tmp[0..k-1])
//   * the decode matrix zfec's fec_decode inverts (easyfec.Decoder at
//     piece.py:196): row i = e_i for a primary in its own slot, enc[idx[i]]
//     for a secondary.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace sec {

struct Gf {
    uint8_t exp[510];
    int log[256];
    uint8_t inv[256];
    Gf()
    {
        unsigned v = 1;
        for (int e = 0; e < 255; ++e) {
            exp[e] = exp[e + 255] = (uint8_t)v;
            log[v] = e;
            v <<= 1;
            if (v & 0x100)
                v ^= 0x11D;
        }
        log[0] = -1;
        inv[0] = 0;
        for (int a = 1; a < 256; ++a)
            inv[a] = exp[255 - log[a]];
    }
    uint8_t mul(uint8_t a, uint8_t b) const { return (a && b) ? exp[log[a] + log[b]] : 0; }
};

inline const Gf &gf()
{
    static const Gf g;
    return g;
}

// In-place inverse of a k x k row-major matrix; false if singular.
inline bool gf_invert(std::vector<uint8_t> &a, int k)
{
    const Gf &g = gf();
    std::vector<uint8_t> inv((size_t)k * k, 0);
    for (int i = 0; i < k; ++i)
        inv[(size_t)i * k + i] = 1;
    for (int c = 0; c < k; ++c) {
        int piv = c;
        while (piv < k && a[(size_t)piv * k + c] == 0)
            ++piv;
        if (piv == k)
            return false;
        if (piv != c)
            for (int t = 0; t < k; ++t) {
                std::swap(a[(size_t)piv * k + t], a[(size_t)c * k + t]);
                std::swap(inv[(size_t)piv * k + t], inv[(size_t)c * k + t]);
            }
        const uint8_t s = g.inv[a[(size_t)c * k + c]];
        for (int t = 0; t < k; ++t) {
            a[(size_t)c * k + t] = g.mul(a[(size_t)c * k + t], s);
            inv[(size_t)c * k + t] = g.mul(inv[(size_t)c * k + t], s);
        }
        for (int r = 0; r < k; ++r) {
            const uint8_t f = a[(size_t)r * k + c];
            if (r == c || f == 0)
                continue;
            for (int t = 0; t < k; ++t) {
                a[(size_t)r * k + t] ^= g.mul(f, a[(size_t)c * k + t]);
                inv[(size_t)r * k + t] ^= g.mul(f, inv[(size_t)c * k + t]);
            }
        }
    }
    a.swap(inv);
    return true;
}

// Full m x k encode matrix (identity on top).
inline std::vector<uint8_t> encode_matrix(int k, int m)
{
    const Gf &g = gf();
    std::vector<uint8_t> seed((size_t)m * k, 0), enc((size_t)m * k, 0);
    seed[0] = 1;
    for (int r = 1; r < m; ++r)
        for (int c = 0; c < k; ++c)
            seed[(size_t)r * k + c] = g.exp[((r - 1) * c) % 255];
    std::vector<uint8_t> top(seed.begin(), seed.begin() + (size_t)k * k);
    gf_invert(top, k);  // Vandermonde on distinct points: never singular
    for (int i = 0; i < k; ++i)
        enc[(size_t)i * k + i] = 1;
    for (int r = k; r < m; ++r)
        for (int c = 0; c < k; ++c) {
            uint8_t s = 0;
            for (int t = 0; t < k; ++t)
                s ^= g.mul(seed[(size_t)r * k + t], top[(size_t)t * k + c]);
            enc[(size_t)r * k + c] = s;
        }
    return enc;
}

// zfec _fecmodule.c normalisation: each primary moved into its own slot.
// perm[i] = caller's position of the block now in slot i.
inline void normalise_slots(int k, std::vector<int> &idx, std::vector<int> &perm)
{
    perm.resize(k);
    for (int i = 0; i < k; ++i)
        perm[i] = i;
    int i = 0;
    while (i < k) {
        if (idx[i] >= k || idx[i] == i) {
            ++i;
        } else {
            const int c = idx[i];
            std::swap(idx[i], idx[c]);
            std::swap(perm[i], perm[c]);
        }
    }
}

// zfec's evaluation points: p_0 = 0, p_i = alpha^(i-1) (the seed rows above)
inline uint8_t point(int i) { return i == 0 ? 0 : gf().exp[(i - 1) % 255]; }

// Scalings of the syndrome decode's Cauchy solve (kernels_bs.hip).  zfec's parity row r is the
// Lagrange basis at x_r = p_{k+r}: c[r][j] = a_r b_j / (x_r + y_j) with y_j = p_j,
// a_r = prod_{i<k} (x_r + y_i), b_j = 1 / prod_{i<k, i!=j} (y_j + y_i).  For the present parity
// rows S (ascending) and the lost data rows L (ascending), |S| = |L| = e, the e x e system
// A = c[S][L] = D_a C D_b has C a Cauchy matrix, whose inverse is again one up to diagonals, so
//     A^-1[l][r] = z_l c[r][l] w_r,
//     w_r = prod_{l in L} (x_r + y_l) / prod_{r' in S, r' != r} (x_r + x_r') / a_r^2,
//     z_l = prod_{r in S} (x_r + y_l) / prod_{l' in L, l' != l} (y_l + y_l') / b_l^2.
// Checked against a Gauss-Jordan inverse for every shape (tests/test_cauchy.py restates it).
inline void cauchy_scales(int k, const std::vector<int> &S, const std::vector<int> &Lost, std::vector<uint8_t> &w,
                          std::vector<uint8_t> &z)
{
    const Gf &g = gf();
    auto div = [&](uint8_t a, uint8_t b) { return g.mul(a, g.inv[b]); };
    const size_t e = S.size();
    w.assign(e, 0);
    z.assign(e, 0);
    for (size_t q = 0; q < e; ++q) {
        const uint8_t x = point(k + S[q]);
        uint8_t num = 1, den = 1, a = 1;
        for (int l : Lost)
            num = g.mul(num, x ^ point(l));
        for (size_t q2 = 0; q2 < e; ++q2)
            if (q2 != q)
                den = g.mul(den, x ^ point(k + S[q2]));
        for (int i = 0; i < k; ++i)
            a = g.mul(a, x ^ point(i));
        w[q] = div(div(num, den), g.mul(a, a));
    }
    for (size_t t = 0; t < e; ++t) {
        const uint8_t y = point(Lost[t]);
        uint8_t num = 1, den = 1, binv = 1;  // binv = 1 / b_l
        for (int r : S)
            num = g.mul(num, point(k + r) ^ y);
        for (size_t t2 = 0; t2 < e; ++t2)
            if (t2 != t)
                den = g.mul(den, y ^ point(Lost[t2]));
        for (int i = 0; i < k; ++i)
            if (i != Lost[t])
                binv = g.mul(binv, y ^ point(i));
        z[t] = g.mul(div(num, den), g.mul(binv, binv));
    }
}

// Multiplication by c on bit planes (kernels_bs.hip scale_planes): byte s = c * alpha^s, so
// plane t of c * x is the XOR of the planes s of x whose byte s has bit t set.
inline uint64_t scale_mask(uint8_t c)
{
    uint64_t m = 0;
    for (int s = 0; s < 8; ++s)
        m |= (uint64_t)gf().mul(c, (uint8_t)(1u << s)) << (8 * s);
    return m;
}

// Inverse of zfec's decode matrix for normalised slot indices.
inline bool decode_matrix(int k, int m, const std::vector<int> &idx, std::vector<uint8_t> &minv)
{
    const std::vector<uint8_t> enc = encode_matrix(k, m);
    minv.assign((size_t)k * k, 0);
    for (int i = 0; i < k; ++i) {
        if (idx[i] < k)
            minv[(size_t)i * k + i] = 1;
        else
            memcpy(&minv[(size_t)i * k], &enc[(size_t)idx[i] * k], k);
    }
    return gf_invert(minv, k);
}

// Repair matrix: block `targets[r]` of the code word as a combination of the k source blocks in
// normalised slot order (idx after normalise_slots).  Row r = E[t] * Minv with E[t] the unit row t
// for a data block (so the row is Minv's own row t) and zfec's parity row for t >= k.
// out: targets.size() x k, row-major; false if the sources' decode matrix is singular.
inline bool repair_matrix(int k, int m, const std::vector<int> &idx, const std::vector<int> &targets,
                          std::vector<uint8_t> &out)
{
    const Gf &g = gf();
    std::vector<uint8_t> minv;
    if (!decode_matrix(k, m, idx, minv))
        return false;
    const std::vector<uint8_t> enc = encode_matrix(k, m);
    out.assign(targets.size() * (size_t)k, 0);
    for (size_t r = 0; r < targets.size(); ++r) {
        const int t = targets[r];
        uint8_t *row = &out[r * (size_t)k];
        if (t < k) {
            memcpy(row, &minv[(size_t)t * k], k);
            continue;
        }
        for (int j = 0; j < k; ++j) {
            const uint8_t e = enc[(size_t)t * k + j];
            if (e)
                for (int c = 0; c < k; ++c)
                    row[c] ^= g.mul(e, minv[(size_t)j * k + c]);
        }
    }
    return true;
}

// Which single entry explains an inconsistent column of a check (sec_check_locate).  sharenums:
// the n held blocks in the caller's order, the first k the basis; column: their n bytes at one
// position.  With d_j = (check row j as predicted from the basis) ^ (its stored byte):
//   every d_j zero                      -1: the column is a code word
//   fewer than two check rows           -2: one row cannot tell itself from the basis
//   exactly one d_j nonzero             k + j: a basis error would reach every row (R[j][s] != 0, MDS)
//   every d_j = R[j][s] * e for one s   the caller's position of basis slot s (error value e)
//   else                                -2: no single entry explains it
// false if the basis' decode matrix is singular (never, for distinct sharenums of this code).
inline bool check_locate(int k, int m, const std::vector<int> &sharenums, const uint8_t *column, int *culprit)
{
    const Gf &g = gf();
    const int n = (int)sharenums.size(), r = n - k;
    std::vector<int> idx(sharenums.begin(), sharenums.begin() + k), perm;
    normalise_slots(k, idx, perm);
    std::vector<uint8_t> rm;
    if (!repair_matrix(k, m, idx, std::vector<int>(sharenums.begin() + k, sharenums.end()), rm))
        return false;
    std::vector<uint8_t> d((size_t)r, 0);
    int nonzero = 0, last = -1;
    for (int j = 0; j < r; ++j) {
        uint8_t p = column[k + j];
        for (int s = 0; s < k; ++s)
            p ^= g.mul(rm[(size_t)j * k + s], column[perm[s]]);
        d[j] = p;
        if (p) {
            ++nonzero;
            last = j;
        }
    }
    *culprit = -2;
    if (nonzero == 0)
        *culprit = -1;
    else if (r >= 2 && nonzero == 1)
        *culprit = k + last;
    else if (r >= 2 && nonzero == r)
        for (int s = 0; s < k && *culprit == -2; ++s) {
            if (!rm[s])
                continue;
            const uint8_t e = g.mul(d[0], g.inv[rm[s]]);
            bool all = true;
            for (int j = 1; j < r && all; ++j)
                all = g.mul(rm[(size_t)j * k + s], e) == d[j];
            if (all)
                *culprit = perm[s];
        }
    return true;
}

// ---- bounded-distance correction of one column (sec_check_correct) ---------------------------
// zfec's code is an evaluation code: block i of a column is f(p_i), deg f < k, p_i = point(i).  So
// any n held blocks with points x_j are a Reed-Solomon code of distance r + 1, r = n - k, and with
//     u_j = 1 / prod_{i != j} (x_j + x_i)
// the syndromes S_l = sum_j u_j x_j^l y_j, l < r (0^0 = 1), vanish exactly on code words.
constexpr int kMaxErrors = 16;  // the kernels' state per position holds no more

// t = min(max_errors, floor(r / 2), kMaxErrors); max_errors = 0: the code's limit
inline int error_bound(int r, int max_errors)
{
    int t = r / 2 < kMaxErrors ? r / 2 : kMaxErrors;
    if (max_errors > 0 && max_errors < t)
        t = max_errors;
    return t < 0 ? 0 : t;
}

// x_j and u_j of the held blocks `nums` (distinct)
inline void held_weights(const std::vector<int> &nums, std::vector<uint8_t> &x, std::vector<uint8_t> &u)
{
    const Gf &g = gf();
    const size_t n = nums.size();
    x.resize(n);
    u.resize(n);
    for (size_t j = 0; j < n; ++j)
        x[j] = point(nums[j]);
    for (size_t j = 0; j < n; ++j) {
        uint8_t p = 1;
        for (size_t i = 0; i < n; ++i)
            if (i != j)
                p = g.mul(p, x[j] ^ x[i]);
        u[j] = g.inv[p];
    }
}

// The code word within t = error_bound(n - k, max_errors) entries of `column`, if there is one (it is
// unique: 2t <= r).  fixed: the n corrected bytes; *nchanged: 0 for a code word, 1 .. t the entries
// changed, -2 open (fixed = column).  The kernels' judge (kernels.hip corx_judge) step for step:
//   * the check deltas d_j, as check_locate's.  The column less the code word its basis spans is zero
//     on the basis and d_j on check row j, and syndromes are linear, so S_l = sum_j u_j x_j^l d_j
//     over the r check rows alone, l < 2t;
//   * Berlekamp-Massey, exactly 2t steps: the shortest recurrence S_i = sum_{1..L} C_q S_{i-q}; with
//     errors on a set E of at most t entries L = |E| and C(z) = prod_E (1 + x_j z).  L > t: open;
//   * the roots among the n held points of R(z) = sum_q C_q z^(L-q) = prod_E (z + x_j), L Horner steps
//     each.  Block 0's point is 0, a factor 1 of C: its error shows as deg C = L - 1, which makes 0 a
//     root of R like any other point.  Other than L roots: open;
//   * the values: with Q(z) = R(z) / (z + x_j) = sum_l q_l z^l (synthetic division),
//     sum_l q_l S_l = u_j e_j Q(x_j), so e_j = sum_l q_l S_l / (Q(x_j) u_j); a zero value: open;
//   * the check rows once more on the changed column: any nonzero delta, open.  This makes the
//     verdict exact whatever the steps before it did.
// More than t and at most r - t wrong entries are therefore always open; beyond r - t the column may
// lie within t of another code word and is corrected to that.  false: singular basis (never).
inline bool check_correct(int k, int m, const std::vector<int> &sharenums, const uint8_t *column, int max_errors,
                          uint8_t *fixed, int *nchanged)
{
    const Gf &g = gf();
    const int n = (int)sharenums.size(), r = n - k, t = error_bound(r, max_errors);
    std::vector<int> idx(sharenums.begin(), sharenums.begin() + k), perm;
    normalise_slots(k, idx, perm);
    std::vector<uint8_t> rm;
    if (!repair_matrix(k, m, idx, std::vector<int>(sharenums.begin() + k, sharenums.end()), rm))
        return false;
    auto deltas = [&](const uint8_t *col, std::vector<uint8_t> &d) {
        bool any = false;
        d.assign((size_t)r, 0);
        for (int j = 0; j < r; ++j) {
            uint8_t p = col[k + j];
            for (int s = 0; s < k; ++s)
                p ^= g.mul(rm[(size_t)j * k + s], col[perm[s]]);
            d[j] = p;
            any |= p != 0;
        }
        return any;
    };
    memcpy(fixed, column, (size_t)n);
    std::vector<uint8_t> d;
    if (!deltas(column, d)) {
        *nchanged = 0;
        return true;
    }
    *nchanged = -2;
    if (t == 0)
        return true;
    std::vector<uint8_t> x, u;
    held_weights(sharenums, x, u);
    uint8_t S[2 * kMaxErrors] = {0}, C[kMaxErrors + 1] = {1}, Bp[kMaxErrors + 1] = {1};
    for (int j = 0; j < r; ++j) {
        uint8_t term = g.mul(u[k + j], d[j]);
        for (int l = 0; l < 2 * t; ++l) {
            S[l] ^= term;
            term = g.mul(term, x[k + j]);
        }
    }
    int L = 0, sh = 1;
    uint8_t b = 1;
    for (int i = 0; i < 2 * t; ++i) {
        uint8_t dd = S[i];
        for (int q = 1; q <= kMaxErrors; ++q)
            if (q <= L && q <= i)
                dd ^= g.mul(C[q], S[i - q]);
        if (dd == 0) {
            ++sh;
            continue;
        }
        const uint8_t f = g.mul(dd, g.inv[b]);
        const bool grow = 2 * L <= i;
        for (int q = kMaxErrors; q >= 0; --q) {  // C += f z^sh B, and B = the old C where L grows, in place
            const uint8_t c = C[q];
            if (q >= sh)
                C[q] = c ^ g.mul(f, Bp[q - sh]);
            if (grow)
                Bp[q] = c;
        }
        if (grow) {
            L = i + 1 - L;
            b = dd;
            sh = 1;
        } else {
            ++sh;
        }
    }
    if (L > t)
        return true;
    int loc[kMaxErrors], nloc = 0;
    for (int j = 0; j < n; ++j) {
        uint8_t v = 0;
        for (int q = 0; q <= L; ++q)
            v = g.mul(v, x[j]) ^ C[q];
        if (v == 0) {
            if (nloc == L)
                return true;
            loc[nloc++] = j;
        }
    }
    if (nloc != L)
        return true;
    for (int a = 0; a < L; ++a) {
        const int j = loc[a];
        uint8_t q = 0, num = 0, den = 0;
        for (int l = L - 1; l >= 0; --l) {
            q = C[L - 1 - l] ^ g.mul(x[j], q);
            num ^= g.mul(q, S[l]);
            den = g.mul(den, x[j]) ^ q;
        }
        const uint8_t e = g.mul(g.mul(num, g.inv[den]), g.inv[u[j]]);
        if (den == 0 || e == 0) {
            memcpy(fixed, column, (size_t)n);
            return true;
        }
        fixed[j] ^= e;
    }
    if (deltas(fixed, d)) {
        memcpy(fixed, column, (size_t)n);
        return true;
    }
    *nchanged = L;
    return true;
}

}  // namespace sec
