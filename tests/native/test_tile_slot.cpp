// Host-side unit test of the tile maps' XCD-major placement (kernels.hpp tile_slot, bs_plan.hpp
// append_placed; no HIP).  Built by tests/test_native_tile_slot.py with g++ under AddressSanitizer
// + UBSan.  What a run of the map belongs to is summed up here from the counts, not taken from the
// function's formula.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bs_plan.hpp"

static int fails = 0;

static void fail(const char *what, uint32_t nt)
{
    fprintf(stderr, "FAIL %s: nt = %u\n", what, nt);
    ++fails;
}

static void test_count(uint32_t nt)
{
    // a bijection of [0, nt) onto itself; the identity below 16
    std::vector<uint32_t> owner(nt, UINT32_MAX);  // slot -> the workgroup that reads it
    for (uint32_t b = 0; b < nt; ++b) {
        const uint32_t s = sec::tile_slot(b, nt);
        if (s >= nt || owner[s] != UINT32_MAX)
            return fail("bijection", nt);
        if (nt < 16 && s != b)
            return fail("identity below 16", nt);
        owner[s] = b;
    }
    if (nt < 16)
        return;
    // run x (the workgroups b % 8 == x, ascending) is contiguous: lo[x] .. lo[x + 1]
    uint32_t lo[9] = {0};
    for (uint32_t x = 0; x < 8; ++x)
        lo[x + 1] = lo[x] + nt / 8 + (x < nt % 8 ? 1 : 0);
    for (uint32_t b = 0; b < nt; ++b)
        if (sec::tile_slot(b, nt) != lo[b % 8] + b / 8)
            return fail("runs", nt);
    // the 8 entries of an aligned group (one 128-byte line of 16-byte tiles) belong to one residue
    // class b % 8, but for the at most 8 groups that hold a run's boundary
    uint32_t mixed = 0;
    for (uint32_t g = 0; g < nt; g += 8) {
        bool one = true;
        for (uint32_t s = g; s < g + 8 && s < nt; ++s)
            one = one && owner[s] % 8 == owner[g] % 8;
        mixed += one ? 0 : 1;
    }
    if (mixed > 8)
        return fail("lines of one residue class", nt);
}

// The planner's placement read back as the kernels read it: workgroup b finds the tile it was
// given, after a chunk-order launch and after an XCD-ordered one, several launches in one array.
static void test_placed(uint32_t nt)
{
    std::vector<sec::Tile> ident(nt);
    for (uint32_t b = 0; b < nt; ++b)
        ident[b] = sec::Tile{b, b * 7 + 3, b % 5, b % 3};
    std::vector<sec::Tile> ordered = ident;
    sec::xcd_order(ordered);  // workgroup b runs tile ordered[b]
    std::vector<sec::Tile> img(3, sec::Tile{9, 9, 9, 9});  // an earlier launch's entries stay
    sec::append_placed(img, ident);
    sec::append_placed(img, ordered);
    if (img.size() != 3 + 2 * (size_t)nt)
        return fail("placed size", nt);
    for (uint32_t b = 0; b < 3; ++b)
        if (img[b].chunk != 9)
            return fail("placed: earlier entries", nt);
    for (uint32_t b = 0; b < nt; ++b) {
        const uint32_t s = sec::tile_slot(b, nt);
        if (memcmp(&img[3 + s], &ident[b], sizeof(sec::Tile)) != 0 || img[3 + s].chunk != b)
            return fail("placed identity map read back", nt);
        if (memcmp(&img[3 + nt + s], &ordered[b], sizeof(sec::Tile)) != 0)
            return fail("placed XCD-ordered map read back", nt);
    }
    // placement undoes xcd_order's permutation: an XCD-ordered launch's sub-array is in chunk order
    for (uint32_t i = 0; i < nt; ++i)
        if (img[3 + nt + i].chunk != i)
            return fail("placed after xcd_order", nt);
}

int main()
{
    std::vector<uint32_t> counts;
    for (uint32_t nt = 1; nt <= 4096; ++nt)
        counts.push_back(nt);
    for (uint32_t nt : {65536u, 262144u, 262145u, 262146u, 262147u, 262148u, 262149u, 262150u, 262151u})
        counts.push_back(nt);
    for (uint32_t nt : counts) {
        test_count(nt);
        test_placed(nt);
    }
    std::vector<sec::Tile> none;
    sec::append_placed(none, {});
    if (!none.empty())
        fail("empty launch", 0);
    if (fails)
        return 1;
    printf("tile slot tests ok\n");
    return 0;
}
