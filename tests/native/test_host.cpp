// Host-side unit test of libstorbec's C++ helpers (no HIP): GF matrices, the staging copy
// pool, the task pool + SHA-1 of sec_encode_pieces, and the bit-sliced kernels' host planning
// (bs_plan.hpp).  Built by tests/test_native_host.py with g++ under AddressSanitizer + UBSan and,
// separately, ThreadSanitizer (the pools' threads).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "bs_plan.hpp"
#include "gf_host.hpp"
#include "task_pool.hpp"

static int fails = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                     \
        }                                                                \
    } while (0)

static void test_matrices()
{
    const sec::Gf &g = sec::gf();
    const std::vector<uint8_t> e = sec::encode_matrix(4, 6);
    const uint8_t want[8] = {0x77, 0x40, 0x38, 0x0e, 0xc7, 0xa7, 0x0d, 0x6c};
    EXPECT(memcmp(e.data() + 16, want, 8) == 0);
    for (int k : {1, 2, 5, 10, 32, 64}) {
        const int m = std::min(256, k + k / 2 + 1);
        const std::vector<uint8_t> enc = sec::encode_matrix(k, m);
        // any k rows (here: the last k) form an invertible matrix whose inverse is exact
        std::vector<int> idx;
        for (int i = 0; i < k; ++i)
            idx.push_back(m - k + i);
        std::vector<int> perm;
        sec::normalise_slots(k, idx, perm);
        for (int i = 0; i < k; ++i)
            EXPECT(idx[i] >= k || idx[i] == i);
        std::vector<uint8_t> minv;
        EXPECT(sec::decode_matrix(k, m, idx, minv));
        for (int r = 0; r < k; ++r)
            for (int c = 0; c < k; ++c) {
                uint8_t s = 0;
                for (int t = 0; t < k; ++t) {
                    const uint8_t a = idx[r] < k ? (uint8_t)(t == r) : enc[(size_t)idx[r] * k + t];
                    s ^= g.mul(a, minv[(size_t)t * k + c]);
                }
                EXPECT(s == (r == c ? 1 : 0));
            }
    }
}

static void test_copy_pool()
{
    std::mt19937_64 rng(7);
    sec::TaskPool pool(5);
    for (int round = 0; round < 40; ++round) {
        const int njobs = 1 + (int)(rng() % 40);
        std::vector<std::vector<char>> src(njobs), dst(njobs);
        std::vector<sec::CopyJob> jobs;
        for (int j = 0; j < njobs; ++j) {
            const size_t n = rng() % (round % 3 == 0 ? 64 : (3 << 20));
            src[j].resize(n);
            dst[j].assign(n, 0);
            for (size_t i = 0; i < n; i += 4096)
                src[j][i] = (char)rng();
            jobs.push_back(sec::CopyJob{dst[j].data(), src[j].data(), n});
        }
        pool.run_copies(jobs);
        for (int j = 0; j < njobs; ++j)
            EXPECT(src[j] == dst[j]);
    }
}

// copies from several threads at once through one shared pool (contexts of one process share it)
static void test_shared_pool_concurrent()
{
    std::shared_ptr<sec::TaskPool> a = sec::shared_pool(4), b = sec::shared_pool(4);
    EXPECT(a.get() == b.get());
    EXPECT(sec::shared_pool(3).get() != a.get());
    EXPECT(sec::usable_cpus() >= 1);
    EXPECT(sec::default_pool_threads() >= 1 && sec::default_pool_threads() <= 7 &&
           sec::default_pool_threads() <= std::max(1, sec::usable_cpus() / 2));
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int t = 0; t < 6; ++t)
        th.emplace_back([&, t] {
            std::mt19937_64 rng(100 + t);
            for (int round = 0; round < 6; ++round) {
                const size_t n = (5u << 20) + rng() % (3u << 20);
                std::vector<char> src(n), dst(n, 0), zero(n, 1);
                for (size_t i = 0; i < n; i += 512)
                    src[i] = (char)rng();
                a->run_copies({sec::CopyJob{dst.data(), src.data(), n}, sec::CopyJob{zero.data(), nullptr, n}});
                if (dst != src || zero != std::vector<char>(n, 0))
                    ++bad;
            }
        });
    for (auto &x : th)
        x.join();
    EXPECT(bad.load() == 0);
}

static void test_task_pool_sha1()
{
    // known answers (FIPS 180-1): "abc", and the empty message
    uint8_t d[20];
    const uint8_t abc[20] = {0xa9, 0x99, 0x3e, 0x36, 0x47, 0x06, 0x81, 0x6a, 0xba, 0x3e,
                             0x25, 0x71, 0x78, 0x50, 0xc2, 0x6c, 0x9c, 0xd0, 0xd8, 0x9d};
    EXPECT(sec::sha1_padded((const uint8_t *)"abc", 3, 3, d) && memcmp(d, abc, 20) == 0);
    const uint8_t empty[20] = {0xda, 0x39, 0xa3, 0xee, 0x5e, 0x6b, 0x4b, 0x0d, 0x32, 0x55,
                               0xbf, 0xef, 0x95, 0x60, 0x18, 0x90, 0xaf, 0xd8, 0x07, 0x09};
    EXPECT(sec::sha1_padded(nullptr, 0, 0, d) && memcmp(d, empty, 20) == 0);
    // the padded form equals the hash of the explicitly zero-padded bytes, from many threads
    std::mt19937_64 rng(11);
    sec::TaskPool pool(6);
    for (int round = 0; round < 8; ++round) {
        const int n = 1 + (int)(rng() % 64);
        std::vector<std::vector<uint8_t>> msg(n);
        std::vector<size_t> avail(n);
        std::vector<uint8_t> got((size_t)n * 20), want((size_t)n * 20);
        for (int i = 0; i < n; ++i) {
            const size_t len = rng() % (round % 2 ? 70000 : 300);
            avail[i] = len ? rng() % (len + 1) : 0;
            msg[i].assign(len, 0);
            for (size_t b = 0; b < avail[i]; ++b)
                msg[i][b] = (uint8_t)rng();
            EXPECT(sec::sha1_padded(msg[i].data(), len, len, &want[(size_t)i * 20]));
        }
        sec::TaskPool::Group g1, g2;
        for (int i = 0; i < n; ++i) {
            sec::TaskPool::Group &g = i % 2 ? g1 : g2;
            const uint8_t *p = msg[i].data();
            const size_t av = avail[i], len = msg[i].size();
            uint8_t *o = &got[(size_t)i * 20];
            pool.submit(g, [=] { return sec::sha1_padded(p, av, len, o); });
        }
        EXPECT(pool.wait(g1));
        EXPECT(pool.wait(g2));
        EXPECT(got == want);
    }
    sec::TaskPool::Group gf;  // a failing task is reported, the rest still run
    std::atomic<int> ran{0};
    for (int i = 0; i < 20; ++i)
        pool.submit(gf, [&ran, i] { ++ran; return i != 7; });
    EXPECT(!pool.wait(gf));
    EXPECT(ran.load() == 20);
}

// bs_plan.hpp: the host planning of the bit-sliced check, repair and syndrome decode
static void test_bs_plan()
{
    // layout: k = 4, m = 7; the basis holds blocks {2, 0, 3, 1}, check rows {6, 4}; block 3 is short
    {
        const int k = 4, m = 7, sn[6] = {2, 0, 3, 1, 6, 4};
        const uint64_t eoff[6] = {1200, 1000, 1300, 1100, 1600, 1400};  // block b at 1000 + 100 b
        const uint32_t eavail[6] = {64, 64, 17, 64, 64, 64};
        std::vector<uint64_t> off;
        std::vector<uint32_t> avail, rmap;
        for (uint32_t chunk = 0; chunk < 2; ++chunk) {  // the second appended after the first
            const sec::BsLayout l = sec::bs_layout(k, m, sn, eoff, eavail, 6, k, off, avail, &rmap);
            EXPECT(l.slot0 == chunk * 7 && l.rmap0 == chunk * 3);
            EXPECT(off.size() == (chunk + 1) * 7 && avail.size() == off.size() && rmap.size() == (chunk + 1) * 3);
            EXPECT(l.dmask == 0xF && l.pmask == 0b101);
            for (int e = 0; e < 6; ++e) {
                EXPECT(off[l.slot0 + sn[e]] == 1000 + 100 * (uint64_t)sn[e]);
                EXPECT(avail[l.slot0 + sn[e]] == (sn[e] == 3 ? 17u : 64u));
            }
            EXPECT(off[l.slot0 + 5] == 0 && avail[l.slot0 + 5] == 0);  // parity row 1 is not held
            EXPECT(rmap[l.rmap0 + 2] == 0 && rmap[l.rmap0 + 0] == 1 && rmap[l.rmap0 + 1] == 0);
        }
        // a decode's basis that holds parity (normalised): no check rows, no rmap
        const int idx[4] = {0, 5, 2, 4};
        const sec::BsLayout l = sec::bs_layout(k, m, idx, eoff, eavail, k, k, off, avail);
        EXPECT(l.slot0 == 14 && off.size() == 21 && rmap.size() == 6);
        EXPECT(l.dmask == 0b0101 && l.pmask == 0b011);
        EXPECT(off[14 + 0] == 1200 && off[14 + 5] == 1000 && off[14 + 2] == 1300 && off[14 + 4] == 1100);
        EXPECT(avail[14 + 2] == 17 && avail[14 + 4] == 64);
        for (int j : {1, 3, 6})  // neither held: untouched
            EXPECT(off[14 + j] == 0 && avail[14 + j] == 0);
    }
    // touched_groups (no shape has 64-row groups: that shift is pinned here, under UBSan)
    using G = std::vector<int>;
    EXPECT(sec::touched_groups(1, 32, 16) == G({0}));
    EXPECT(sec::touched_groups(1ull << 16, 32, 16) == G({1}));
    EXPECT(sec::touched_groups(1 | 1ull << 31, 32, 16) == G({0, 1}));
    EXPECT(sec::touched_groups(0, 32, 16) == G());
    EXPECT(sec::touched_groups(0b1000, 4, 4) == G({0}));
    EXPECT(sec::touched_groups(~0ull, 64, 64) == G({0}));
    // add_group_run_tiles: runs of 8 tiles of each group, then the ragged last span of each
    for (bool copy_first : {true, false}) {
        std::vector<sec::Tile> t;
        sec::add_group_run_tiles(t, 5, 8 * 2048 + 1, 2048, {0, 1}, 16, copy_first);
        EXPECT(t.size() == 18);
        for (size_t i = 0; i < t.size(); ++i) {
            const uint32_t g = i < 16 ? (uint32_t)i / 8 : (uint32_t)i - 16;
            EXPECT(t[i].chunk == 5 && t[i].r0 == 16 * g);
            EXPECT(t[i].t0 == (i < 16 ? (i % 8) * 2048 : 16384));
            EXPECT(t[i].ntail == (copy_first && g == 0 ? 1u : 0u));
        }
    }
    // eligibility: the basis is the chunk's k data blocks
    {
        const int k = 4;
        const int32_t sn[6] = {2, 0, 3, 1, 6, 4}, par[6] = {2, 0, 4, 1, 6, 3};
        const uint64_t B = 16, full[6] = {16, 16, 16, 16, 16, 16}, last_short[6] = {16, 16, 5, 16, 16, 16},
                       data_short[6] = {16, 15, 16, 16, 16, 16}, parity_short[6] = {16, 16, 16, 16, 15, 16};
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, B, nullptr) == 0);
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, B, full) == 0);
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, B, last_short) == 0);  // only block k-1 short
        EXPECT(sec::bs_data_basis_shape(-1, k, sn, 6, B, full) == -1);
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, 15, nullptr) == -1);
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, sec::kBsMaxB, nullptr) == 0);
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, sec::kBsMaxB + 1, nullptr) == -1);
        EXPECT(sec::bs_data_basis_shape(0, k, par, 6, B, full) == -1);  // a basis entry >= k
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, B, data_short) == -1);
        EXPECT(sec::bs_data_basis_shape(0, k, sn, 6, B, parity_short) == -1);
        // the check's own conditions: a check row, padlen < B
        EXPECT(sec::check_bs_shape(0, k, sn, 6, B, last_short, 3) == 0);
        EXPECT(sec::check_bs_shape(-1, k, sn, 6, B, full, 3) == -1);
        EXPECT(sec::check_bs_shape(0, k, sn, 6, 15, nullptr, 3) == -1);
        EXPECT(sec::check_bs_shape(0, k, par, 6, B, full, 3) == -1);
        EXPECT(sec::check_bs_shape(0, k, sn, 6, B, data_short, 3) == -1);
        EXPECT(sec::check_bs_shape(0, k, sn, 6, B, parity_short, 3) == -1);
        EXPECT(sec::check_bs_shape(0, k, sn, k, B, full, 3) == -1);
        EXPECT(sec::check_bs_shape(0, k, sn, 6, B, full, B) == -1);
        EXPECT(sec::check_bs_shape(0, k, sn, 6, B, full, B - 1) == 0);
        // the repair's: a target or a check row
        EXPECT(sec::repair_bs_shape(0, k, sn, k, 0, B, full) == -1);
        EXPECT(sec::repair_bs_shape(0, k, sn, k, 1, B, full) == 0);
        EXPECT(sec::repair_bs_shape(0, k, sn, k + 1, 0, B, full) == 0);
        EXPECT(sec::repair_bs_shape(0, k, sn, k, 1, B, last_short) == 0);
        EXPECT(sec::repair_bs_shape(-1, k, sn, k, 1, B, full) == -1);
        EXPECT(sec::repair_bs_shape(0, k, sn, k, 1, 15, nullptr) == -1);
        EXPECT(sec::repair_bs_shape(0, k, par, k, 1, B, full) == -1);
        EXPECT(sec::repair_bs_shape(0, k, sn, 6, 1, B, data_short) == -1);
        EXPECT(sec::repair_bs_shape(0, k, sn, 6, 1, B, parity_short) == -1);
    }
}

// bs_plan.hpp xcd_order: a permutation for every count (n % 8 != 0 included), the identity below 16
// tiles; entry b is a tile of the contiguous eighth of XCD b % 8 (the first n % 8 eighths one tile
// longer, their bounds summed up here, not taken from the function's formula), and each eighth is
// walked upwards without a gap.
static void test_xcd_order()
{
    std::vector<size_t> counts;
    for (size_t n = 0; n <= 4200; ++n)
        counts.push_back(n);
    for (size_t n : {2048, 2022, 1540, 65536 + 5})
        counts.push_back(n);
    for (size_t n : counts) {
        std::vector<sec::Tile> t(n);
        for (size_t i = 0; i < n; ++i)
            t[i] = sec::Tile{(uint32_t)(i * 7 + 3), (uint32_t)i, (uint32_t)(i % 5), (uint32_t)(i % 3)};
        const std::vector<sec::Tile> in = t;
        sec::xcd_order(t);
        bool ok = t.size() == n;
        size_t lo[9] = {0};
        for (size_t x = 0; x < 8; ++x)
            lo[x + 1] = lo[x] + n / 8 + (x < n % 8 ? 1 : 0);
        ok = ok && lo[8] == n;
        std::vector<uint8_t> seen(n, 0);
        size_t next[8];
        for (size_t x = 0; x < 8; ++x)
            next[x] = lo[x];
        for (size_t b = 0; ok && b < n; ++b) {
            const size_t i = t[b].t0, x = b % 8;
            ok = i < n && !seen[i] && memcmp(&t[b], &in[i], sizeof(sec::Tile)) == 0;  // a whole input tile, once
            if (!ok)
                break;
            seen[i] = 1;
            if (n < 16) {
                ok = i == b;
            } else {
                ok = lo[x] <= i && i < lo[x + 1] && i == next[x];  // its XCD's eighth, ascending
                ++next[x];
            }
        }
        for (size_t x = 0; ok && n >= 16 && x < 8; ++x)
            ok = next[x] == lo[x + 1];
        if (!ok) {
            fprintf(stderr, "FAIL xcd_order: n = %zu\n", n);
            ++fails;
        }
    }
}

int main()
{
    test_xcd_order();
    test_matrices();
    test_copy_pool();
    test_shared_pool_concurrent();
    test_task_pool_sha1();
    test_bs_plan();
    if (fails)
        return 1;
    printf("native host tests ok\n");
    return 0;
}
