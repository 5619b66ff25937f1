// Stand-alone check of gf_host.hpp's check_correct (sec_check_correct's arithmetic, the model of the
// kernels' judge), built with -fsanitize=address,undefined by tests/test_native_correct_multi.py:
// inject at most t errors and get them back, up to t = 16 on zfec(64,96) with 96 held; more than t
// and at most r - t are open; max_errors = 1 is check_locate.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "gf_host.hpp"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static unsigned g_seed = 12345;
static unsigned rnd() { return (g_seed = g_seed * 1103515245u + 12345u) >> 16; }

// a code word's bytes at the blocks `sn`
static std::vector<uint8_t> word(int k, int m, const std::vector<int> &sn)
{
    static std::vector<uint8_t> enc;
    static int ek = 0, em = 0;
    if (ek != k || em != m) {
        enc = sec::encode_matrix(k, m);
        ek = k;
        em = m;
    }
    std::vector<uint8_t> d((size_t)k), col(sn.size());
    for (auto &v : d)
        v = (uint8_t)rnd();
    for (size_t i = 0; i < sn.size(); ++i) {
        uint8_t v = 0;
        for (int j = 0; j < k; ++j)
            v ^= sec::gf().mul(enc[(size_t)sn[i] * k + j], d[j]);
        col[i] = v;
    }
    return col;
}

// `ne` distinct entries of `col` changed, entry `must` (if >= 0) among them
static std::vector<uint8_t> damaged(const std::vector<uint8_t> &col, int ne, int must)
{
    std::vector<int> at(col.size());
    for (size_t i = 0; i < at.size(); ++i)
        at[i] = (int)i;
    for (size_t i = at.size() - 1; i > 0; --i)
        std::swap(at[i], at[rnd() % (i + 1)]);
    if (must >= 0 && ne > 0)
        std::swap(at[0], *std::find(at.begin(), at.end(), must));
    std::vector<uint8_t> bad = col;
    for (int i = 0; i < ne; ++i)
        bad[(size_t)at[i]] ^= (uint8_t)(1 + rnd() % 255);
    return bad;
}

static void shape(int k, int m, std::vector<int> sn, int max_errors, int trials)
{
    const int n = (int)sn.size(), r = n - k, t = sec::error_bound(r, max_errors);
    int zero = -1;
    for (int i = 0; i < n; ++i)
        if (sn[i] == 0)
            zero = i;
    std::vector<uint8_t> fixed((size_t)n);
    for (int trial = 0; trial < trials; ++trial) {
        const std::vector<uint8_t> col = word(k, m, sn);
        for (int ne = 0; ne <= r - t; ++ne) {
            const std::vector<uint8_t> bad = damaged(col, ne, trial % 2 ? zero : -1);
            int changed = 99;
            REQUIRE(sec::check_correct(k, m, sn, bad.data(), max_errors, fixed.data(), &changed));
            if (ne <= t) {
                REQUIRE(changed == ne);
                REQUIRE(fixed == col);
            } else {
                REQUIRE(changed == -2);
                REQUIRE(fixed == bad);
            }
            if (max_errors == 1) {
                int who = 99;
                REQUIRE(sec::check_locate(k, m, sn, bad.data(), &who));
                REQUIRE(changed == (who == -1 ? 0 : who == -2 ? -2 : 1));
                for (int j = 0; j < n; ++j)
                    REQUIRE((fixed[(size_t)j] != bad[(size_t)j]) == (j == who));
            }
        }
        // noise: whatever the verdict, `fixed` is the column or differs from it in `changed` entries
        std::vector<uint8_t> noise((size_t)n);
        for (auto &v : noise)
            v = (uint8_t)rnd();
        int changed = 99, differs = 0;
        REQUIRE(sec::check_correct(k, m, sn, noise.data(), max_errors, fixed.data(), &changed));
        for (int j = 0; j < n; ++j)
            differs += fixed[(size_t)j] != noise[(size_t)j];
        REQUIRE(changed == -2 ? differs == 0 : (changed == differs && changed <= t));
    }
}

static std::vector<int> iota(int from, int to)
{
    std::vector<int> v;
    for (int i = from; i < to; ++i)
        v.push_back(i);
    return v;
}

int main()
{
    REQUIRE(sec::error_bound(32, 0) == 16 && sec::error_bound(40, 0) == 16 && sec::error_bound(32, 3) == 3);
    REQUIRE(sec::error_bound(7, 0) == 3 && sec::error_bound(1, 0) == 0 && sec::error_bound(0, 5) == 0);
    for (int T : {0, 1, 2}) {
        shape(4, 6, {5, 0, 3, 2, 4, 1}, T, 40);
        shape(4, 6, {5, 0, 3, 2, 1}, T, 10);  // one check row: nothing is corrected
        shape(4, 6, {0, 5, 2, 4}, T, 4);      // n == k: every column is a code word
        shape(8, 11, {10, 1, 2, 3, 4, 5, 6, 7, 0, 8, 9}, T, 40);
        shape(10, 14, {13, 0, 2, 3, 11, 5, 6, 12, 8, 9, 1, 4, 7, 10}, T, 40);
        shape(10, 14, {13, 12, 2, 3, 11, 5, 6, 1, 8, 9, 10, 4, 7}, T, 40);  // piece 0 not held, r = 3
        shape(16, 24, iota(0, 24), T, 20);
    }
    {
        std::vector<int> all = iota(0, 96), rev = all, most = iota(1, 96);
        std::reverse(rev.begin(), rev.end());  // piece 0 the last check row
        shape(64, 96, all, 0, 6);              // t = 16
        shape(64, 96, rev, 0, 6);
        shape(64, 96, most, 0, 4);             // r = 31, t = 15
        shape(64, 96, all, 5, 3);
        shape(32, 48, iota(0, 48), 0, 6);
    }
    puts("native correct_multi tests ok");
    return 0;
}
