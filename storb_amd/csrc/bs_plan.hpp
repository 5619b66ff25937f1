// bs_plan.hpp — host planning shared by the bit-sliced check, repair and syndrome decode
// (kernels_bs.hip's phase-1 pipeline): the chunks it can take, a chunk's blocks by block number, the
// row groups it touches and its tiles.  No HIP: tests/native/test_host.cpp runs it under sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "kernels.hpp"

namespace sec {

// Largest block a bit-sliced kernel takes: a tile's positions are 32-bit, and a tile of 256 lanes
// reaches 8192 positions past its t0 before it clamps them to B.
constexpr uint64_t kBsMaxB = 0xFFFFFFFFull - 8192;

struct BsLayout {
    uint32_t slot0, rmap0;
    uint64_t dmask, pmask;  // bit j: data block j held; bit r: parity row r held
};

// A chunk's n held entries (entry e: block sn[e] at eoff[e], eavail[e] readable bytes) by block number:
// appends the chunk's m entries to off / avail, block j (data j < k, parity row r at j = k + r) at
// slot0 + j, those of blocks not held 0.  Entries from `nbasis` on are check rows, entry e check row
// e - nbasis: with `rmap`, appends the chunk's m - k entries, rmap[rmap0 + r] = row r's check row.
inline BsLayout bs_layout(int k, int m, const int *sn, const uint64_t *eoff, const uint32_t *eavail, int n, int nbasis,
                          std::vector<uint64_t> &off, std::vector<uint32_t> &avail,
                          std::vector<uint32_t> *rmap = nullptr)
{
    BsLayout l{(uint32_t)off.size(), rmap ? (uint32_t)rmap->size() : 0u, 0, 0};
    off.resize(off.size() + (size_t)m, 0);
    avail.resize(avail.size() + (size_t)m, 0);
    if (rmap)
        rmap->resize(rmap->size() + (size_t)(m - k), 0);
    for (int e = 0; e < n; ++e) {
        off[l.slot0 + (size_t)sn[e]] = eoff[e];
        avail[l.slot0 + (size_t)sn[e]] = eavail[e];
        (sn[e] < k ? l.dmask : l.pmask) |= 1ull << (sn[e] < k ? sn[e] : sn[e] - k);
        if (rmap && e >= nbasis)
            (*rmap)[l.rmap0 + (size_t)(sn[e] - k)] = (uint32_t)(e - nbasis);
    }
    return l;
}

// The groups of rows_per_group rows, of nrows rows in all, that have a bit set in mask; ascending
inline std::vector<int> touched_groups(uint64_t mask, int nrows, int rows_per_group)
{
    const uint64_t group = rows_per_group >= 64 ? ~0ull : (1ull << rows_per_group) - 1;
    std::vector<int> gs;
    for (int g = 0; g * rows_per_group < nrows; ++g)
        if ((mask >> (g * rows_per_group)) & group)
            gs.push_back(g);
    return gs;
}

// One chunk's tiles for a bit-sliced kernel that runs each row group as a tile of its own, in runs
// of 8 positions per group: workgroup b runs on XCD b % 8, so one XCD's L2 serves a span's second
// read.  `copy_first`: the first group's tiles carry ntail bit 0 (they copy the chunk's blocks).
inline void add_group_run_tiles(std::vector<Tile> &tiles, uint32_t desc_index, uint64_t B, uint64_t step,
                                const std::vector<int> &groups, int rows_per_group, bool copy_first)
{
    for (uint64_t t0 = 0; t0 < B; t0 += 8 * step)
        for (int g : groups)
            for (uint64_t t = t0; t < std::min(B, t0 + 8 * step); t += step)
                tiles.push_back(Tile{desc_index, (uint32_t)t, (uint32_t)(g * rows_per_group),
                                     copy_first && g == groups[0] ? 1u : 0u});
}

// XCD order of one launch's tiles (api.cpp says where it applies and what it measured): workgroup b
// runs on XCD b % 8, so entry b becomes the next tile of the contiguous eighth that belongs to
// XCD b % 8, eighth x starting at x * (n / 8) + min(x, n % 8): the first n % 8 eighths hold one
// tile more.  A permutation for any n; lists of fewer than 16 tiles keep their order.
inline void xcd_order(std::vector<Tile> &t)
{
    const uint32_t n = (uint32_t)t.size();
    if (n < 16)
        return;
    std::vector<Tile> o(n);
    for (uint32_t b = 0; b < n; ++b)
        o[b] = t[tile_slot(b, n)];  // kernels.hpp: the same formula places the map's entries
    t.swap(o);
}

// Appends one launch's tiles, t[b] the tile workgroup b runs (in chunk order or after xcd_order),
// where its kernel reads them: entry b at tile_slot(b, t.size()) of the launch's own sub-array
// (kernels.hpp).  Placement is the inverse view of xcd_order's formula, so an XCD-ordered launch's
// sub-array comes out in chunk order.
inline void append_placed(std::vector<Tile> &tiles, const std::vector<Tile> &t)
{
    const size_t first = tiles.size();
    const uint32_t n = (uint32_t)t.size();
    tiles.resize(first + n);
    for (uint32_t b = 0; b < n; ++b)
        tiles[first + tile_slot(b, n)] = t[b];
}

// Chunks whose basis is their k data blocks, so that every other row, held or wanted, is one of
// zfec's own parity rows, which the bit-sliced kernels hold: `shape` (the (k, m)'s, sec_bs_shape) when
//   * it is one and 16 <= B (below it the tail kernel) <= kBsMaxB;
//   * the first k entries are the data blocks 0 .. k-1 in any order;
//   * every entry's avail is one phase 1's loader honours: it clamps its addresses to B - 16 and
//     reads whole 16-byte pieces, taking the zero-filling byte path for data block k-1 alone (zfec's
//     padded last block read in place): every other entry, data or parity, is readable to B;
// else -1.  sn, avail: the chunk's n entries in the caller's order; avail may be NULL (all B).
inline int bs_data_basis_shape(int shape, int k, const int32_t *sn, int n, uint64_t B, const uint64_t *avail)
{
    if (shape < 0 || B < 16 || B > kBsMaxB)
        return -1;
    for (int j = 0; j < k; ++j)
        if (sn[j] >= k)
            return -1;
    for (int e = 0; avail && e < n; ++e)
        if (sn[e] != k - 1 && avail[e] < B)
            return -1;
    return shape;
}

// Bit-sliced check (sec_check_bs_kernel; check, decode + check): a check row is held, nothing is
// recovered (the basis is data), and only output row k-1 is short, as the syndrome decode asks.
inline int check_bs_shape(int shape, int k, const int32_t *sn, int n, uint64_t B, const uint64_t *avail, uint64_t pad)
{
    return n > k && pad < B ? bs_data_basis_shape(shape, k, sn, n, B, avail) : -1;
}

// Bit-sliced repair (sec_repair_bs_kernel; repair: n == k, repair + check): the chunk has a target or
// a check row.  No target is held, so with the data blocks the basis every target is a parity row.
inline int repair_bs_shape(int shape, int k, const int32_t *sn, int n, int nt, uint64_t B, const uint64_t *avail)
{
    return nt + (n - k) >= 1 ? bs_data_basis_shape(shape, k, sn, n, B, avail) : -1;
}

}  // namespace sec
