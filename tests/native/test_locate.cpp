// Stand-alone check of gf_host.hpp's check_locate (sec_check_locate's arithmetic), built with
// -fsanitize=address,undefined by tests/test_native_locate.py: the exhaustive RS(4,6) case (every
// entry, every nonzero error value, two basis orders) and the short cases around it.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gf_host.hpp"

#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

// byte of block s of the code word whose data column is d[0..k)
static uint8_t word_byte(int k, const std::vector<uint8_t> &enc, const uint8_t *d, int s)
{
    uint8_t v = 0;
    for (int j = 0; j < k; ++j)
        v ^= sec::gf().mul(enc[(size_t)s * k + j], d[j]);
    return v;
}

static int locate(int k, int m, const std::vector<int> &sn, const std::vector<uint8_t> &col)
{
    int who = 99;
    REQUIRE(sec::check_locate(k, m, sn, col.data(), &who));
    return who;
}

static void exhaustive(int k, int m, const std::vector<int> &sn, unsigned seed)
{
    const std::vector<uint8_t> enc = sec::encode_matrix(k, m);
    std::vector<uint8_t> d((size_t)k);
    for (int j = 0; j < k; ++j)
        d[j] = (uint8_t)((seed = seed * 1103515245u + 12345u) >> 16);
    std::vector<uint8_t> col(sn.size());
    for (size_t i = 0; i < sn.size(); ++i)
        col[i] = word_byte(k, enc, d.data(), sn[i]);
    REQUIRE(locate(k, m, sn, col) == -1);
    const int r = (int)sn.size() - k;
    for (size_t i = 0; i < sn.size(); ++i)
        for (int e = 1; e < 256; ++e) {
            std::vector<uint8_t> bad = col;
            bad[i] ^= (uint8_t)e;
            REQUIRE(locate(k, m, sn, bad) == (r >= 2 ? (int)i : -2));
        }
}

int main()
{
    exhaustive(4, 6, {0, 1, 2, 3, 4, 5}, 1);
    exhaustive(4, 6, {5, 0, 3, 2, 4, 1}, 2);
    exhaustive(4, 6, {4, 5, 1, 0, 2, 3}, 3);
    exhaustive(4, 6, {5, 0, 3, 2, 1}, 4);  // one check row: never located
    exhaustive(1, 3, {2, 0, 1}, 5);
    exhaustive(10, 14, {13, 0, 2, 3, 11, 5, 6, 12, 8, 9, 1, 4, 7, 10}, 6);
    {  // n == k: nothing to check
        std::vector<uint8_t> col = {1, 2, 3, 4};
        REQUIRE(locate(4, 6, {0, 5, 2, 4}, col) == -1);
    }
    {  // two errors, three check rows: no single entry explains them
        const std::vector<uint8_t> enc = sec::encode_matrix(4, 7);
        const uint8_t d[4] = {9, 200, 31, 77};
        const std::vector<int> sn = {6, 1, 2, 3, 0, 4, 5};
        std::vector<uint8_t> col(7);
        for (int i = 0; i < 7; ++i)
            col[i] = word_byte(4, enc, d, sn[i]);
        for (int a = 0; a < 7; ++a)
            for (int b = a + 1; b < 7; ++b) {
                std::vector<uint8_t> bad = col;
                bad[a] ^= 0x11;
                bad[b] ^= 0xE0;
                REQUIRE(locate(4, 7, sn, bad) == -2);
            }
    }
    puts("native locate tests ok");
    return 0;
}
