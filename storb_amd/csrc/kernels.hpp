// kernels.hpp — device-side descriptors shared by kernels.hip and api.cpp.
//
// Work decomposition.  A "tile" is one workgroup of L lanes over a run of
// L*16*U consecutive byte positions t of ONE chunk's blocks (U = 1: the kernels keep U as a
// template parameter, but only U = 1 is built; L any multiple of 64 up to 1024),
// and a group of up to 8 output rows (parity rows for encode, missing data rows
// for decode).  Each lane owns 16 consecutive positions per u-step, so every
// wave reads one coalesced 1 KiB run from each of the k input blocks and
// writes one 1 KiB run per output row.  Tiles cover [0, valid) of a chunk
// (valid = length of its last, possibly short, data block); the < padlen
// positions in [valid, B) are computed byte by byte by the chunk's last tile
// (Tile::ntail).  Chunks too small for a tile (valid < 16) become "tail items",
// one thread per position, in a separate launch.
#pragma once
#include <stdint.h>

namespace sec {

constexpr int kLanes = 256;         // threads per workgroup
constexpr int kLaneBytes = 16;      // bytes per lane per u-step (dwordx4)
constexpr int kStepBytes = kLanes * kLaneBytes;  // 4 KiB per u-step
constexpr int kMaxRows = 8;         // output rows per tile (accumulator groups)
constexpr int kTabDwords = 5;       // v_perm tables per GF coefficient
constexpr int kBatchVecs = 16;      // 16 B vectors a lane loads per batch (SEC_ENC/DEC_BATCH):
                                    // a tile has U > 1 only if k * U <= kBatchVecs
// Largest workgroup of a tile kernel with `rows` output rows (its launch bound, which also
// caps its VGPRs: 1024 lanes leave 128 per lane).  Groups of more than 4 rows are bound by
// SEC_LB_WIDE_ROWS lanes (A/B knob); the plan clamps its tile widths to this.
#ifndef SEC_LB_WIDE_ROWS
#define SEC_LB_WIDE_ROWS 1024
#endif
constexpr int max_lanes(int rows, int U) { return U != 1 ? kLanes : (rows > 4 ? SEC_LB_WIDE_ROWS : 1024); }

// One encode chunk, device copy (48 B).
struct EncDesc {
    uint64_t in_off;      // chunk start in `in`
    uint64_t par_off;     // first parity block in `parity`
    uint64_t par_stride;  // bytes between parity blocks
    uint32_t B;           // block bytes = ceil(n/k)
    uint32_t k;           // data blocks
    uint32_t p;           // parity blocks (m - k)
    uint32_t tab;         // dword offset of this chunk's tables, layout [j][r][5]
    uint32_t valid;       // n - (k-1)*B: bytes of the last (zero-padded) data block
    uint32_t pad;
};

// One decode chunk, device copy (40 B).
struct DecDesc {
    uint64_t out_off;  // reassembled chunk start in `out`
    uint64_t n;        // bytes to write = k*B - padlen
    uint32_t B;
    uint32_t k;
    uint32_t e;        // missing primaries (rows recovered)
    uint32_t tab;      // dword offset of tables, layout [slot][missing][5]
    uint32_t slot0;    // first entry in slot_off / slot_row / miss_row
    uint32_t valid;    // positions [0, valid) where every output row is writable and every slot
                       // readable: min(last output row's length, every slot's avail), clamped to [0, B)
};

// Per-slot metadata of a decode launch (device arrays).  Slot c of a chunk is entry
// slot0 + c; a chunk's recovered rows are miss[slot0 .. slot0 + e).
struct DecSlots {
    const uint64_t *off;    // block address: blocks + off[slot]
    const uint32_t *row;    // output row a present primary is copied to, or 0xFFFFFFFF
    const uint32_t *miss;   // output row of each recovered (missing) primary
    const uint32_t *avail;  // bytes of the block that exist in memory; the rest read as zero
};

// One repair chunk, device copy (32 B): nt lost blocks (data or parity) recomputed from k source
// blocks, each a full B-byte piece at an address of its own.
struct RepDesc {
    uint32_t B;
    uint32_t k;
    uint32_t nt;     // target rows
    uint32_t tab;    // dword offset of tables, layout [slot][target][5]
    uint32_t slot0;  // first entry in RepSlots::off / avail
    uint32_t tgt0;   // first entry in RepSlots::tgt_off
    uint32_t valid;  // positions [0, valid) where every slot is readable: min(B, every slot's avail)
    uint32_t pad;
};

// Per-slot and per-target metadata of a repair launch (device arrays).  Slot c of a chunk is entry
// slot0 + c (normalised order), its target row r entry tgt0 + r (the caller's order).
struct RepSlots {
    const uint64_t *off;      // block address: blocks + off[slot]
    const uint32_t *avail;    // bytes of the block that exist in memory; the rest read as zero
    const uint64_t *tgt_off;  // target address: out + tgt_off[target], any byte alignment
};

// One check chunk, device copy (40 B): nr check rows predicted from k basis blocks and compared
// with the stored rows.  Its n = k + nr entries in ChkSlots::off / avail / cpos are the basis in
// normalised order, then the check rows in the caller's order.
struct ChkDesc {
    uint32_t B;
    uint32_t k;
    uint32_t nr;      // check rows
    uint32_t tab;     // dword offset of tables, layout [slot][row][5]
    uint32_t slot0;   // first of the n entries in ChkSlots::off / avail / cpos
    uint32_t flag0;   // ChkSlots::flags[flag0]: the chunk's first differing position (atomicMin);
                      // flags[flag0 + 1 + r]: check row r, 0 once it differs (all 0xFFFFFFFF when clean)
    uint32_t valid;   // positions [0, valid) where all n entries are readable: min(B, every avail)
    uint32_t res;     // the chunk's index in the launch's results[]
    uint32_t cslot0;  // the chunk's first entry in the launch's row_bad[] / column[]
    uint32_t pad;
};

struct ChkSlots {
    const uint64_t *off;    // block address: blocks + off[entry]
    const uint32_t *avail;  // bytes of the block that exist in memory; the rest read as zero
    const uint32_t *cpos;   // the entry's position among the chunk's n in the caller's order
    const uint32_t *echunk; // the entry's chunk (descriptor index)
    uint32_t *flags;        // see ChkDesc::flag0
};

// sec_chk_result's device mirror (include/storb_ec.h)
struct ChkResult {
    uint64_t first;
    uint32_t nbad;
    uint32_t pad;
};

// One decode + check chunk, device copy (48 B): e missing primaries recovered from k basis blocks,
// the present primaries copied, and nr check rows predicted from the same basis and compared with
// the stored rows.  Its n = k + nr entries in DChkSlots::off / avail are those of its ChkDesc (the
// same arrays: sec_check_final writes the results), row / miss are indexed from slot0 as well.
struct DChkDesc {
    uint64_t out_off;  // reassembled chunk (recover-only: its e recovered blocks) in `out`
    uint64_t n;        // bytes to write there
    uint32_t B;
    uint32_t k;
    uint32_t e;        // missing primaries: rows 0 .. e-1 of the table, stored
    uint32_t nr;       // check rows: rows e .. e+nr-1 of the table, compared
    uint32_t tab;      // dword offset of tables, layout [slot][row][5]
    uint32_t slot0;    // first of the n entries
    uint32_t flag0;    // as ChkDesc::flag0
    uint32_t valid;    // positions [0, valid) where every output row is writable and all n entries
                       // readable: min(last output row's length unless recover-only, every avail)
};

struct DChkSlots {
    const uint64_t *off;    // block address: blocks + off[entry]
    const uint32_t *avail;  // bytes of the block that exist in memory; the rest read as zero
    const uint32_t *row;    // basis slots: output row a present primary is copied to, or 0xFFFFFFFF
    const uint32_t *miss;   // miss[slot0 + r]: output row of recovered row r
    uint32_t *flags;        // see ChkDesc::flag0
};

// One decode + correct chunk, device copy (64 B): DChkDesc's fields with the same meaning (the table,
// the n entries, row / miss), and the chunk's words in CorSlots::flags.
struct CorDesc {
    uint64_t out_off;
    uint64_t n;
    uint32_t B;
    uint32_t k;
    uint32_t e;
    uint32_t nr;
    uint32_t tab;
    uint32_t slot0;
    uint32_t flag0;   // flags[flag0]: the first position that is no code word, flags[flag0 + 1]: the first
                      // open one (atomicMin; 0xFFFFFFFF when none)
    uint32_t valid;   // as DChkDesc::valid
    uint32_t cnt0;    // flags[cnt0]: positions corrected, flags[cnt0 + 1]: open, flags[cnt0 + 2 + j]: positions
                      // at which entry j (basis slots in normalised order, then check rows) was the one changed
    uint32_t res;     // the chunk's index in the launch's results[]
    uint32_t cslot0;  // the chunk's first entry in the launch's hits[]
    uint32_t tgt0;    // repair + correct: first entry in RCorSlots::tgt_off (decode + correct: 0)
};

struct CorSlots {
    const uint64_t *off;
    const uint32_t *avail;
    const uint32_t *row;
    const uint32_t *miss;
    const uint32_t *cpos;    // as ChkSlots
    const uint32_t *echunk;
    uint32_t *flags;         // the call's words: [0, 2 * chunks) start as 0xFFFFFFFF, the counters behind as 0
};

// One repair + correct chunk is a CorDesc as well: e its nt target rows (rows 0 .. nt-1 of the table,
// each stored whole at out + tgt_off[tgt0 + r], as RChkDesc's), nr, the n entries and the words as
// above; out_off and n are unused (0), valid = min(B, every avail).  A target may be a held entry.
struct RCorSlots {
    const uint64_t *off;
    const uint32_t *avail;
    const uint64_t *tgt_off;  // target address: out + tgt_off[target], any byte alignment
    const uint32_t *cpos;     // as ChkSlots
    const uint32_t *echunk;
    uint32_t *flags;          // as CorSlots::flags
};

// sec_cor_result's device mirror (include/storb_ec.h)
struct CorResult {
    uint64_t first;
    uint64_t first_open;
    uint32_t corrected;
    uint32_t open;
};

// One repair + check chunk, device copy (40 B): nt lost blocks regenerated from k basis blocks, each
// a whole B-byte piece at an address of its own, and nr check rows predicted from the same basis and
// compared with the stored rows.  Its n = k + nr entries in RChkSlots::off / avail are those of its
// ChkDesc (the same arrays: sec_check_final writes the results).
struct RChkDesc {
    uint32_t B;
    uint32_t k;
    uint32_t nt;     // target rows: rows 0 .. nt-1 of the table, stored
    uint32_t nr;     // check rows: rows nt .. nt+nr-1 of the table, compared
    uint32_t tab;    // dword offset of tables, layout [slot][row][5]
    uint32_t slot0;  // first of the n entries
    uint32_t tgt0;   // first entry in RChkSlots::tgt_off
    uint32_t flag0;  // as ChkDesc::flag0
    uint32_t valid;  // positions [0, valid) where all n entries are readable: min(B, every avail)
    uint32_t pad;
};

struct RChkSlots {
    const uint64_t *off;      // block address: blocks + off[entry]
    const uint32_t *avail;    // bytes of the block that exist in memory; the rest read as zero
    const uint64_t *tgt_off;  // target address: out + tgt_off[target], any byte alignment
    uint32_t *flags;          // see ChkDesc::flag0
};

// One chunk of a syndrome decode (kernels_bs.hip sec_syndrome_bs_kernel, sec_decode_bs_kernel; 56 B).  Block j of
// the chunk (data j < k, parity row r at j = k + r) is at blocks + off[slot0 + j] with
// avail[slot0 + j] readable bytes, when its bit in dmask / pmask is set.
struct SynDesc {
    uint64_t out_off;  // reassembled chunk in `out`: present primaries are copied there (tile flag)
    uint64_t syn_off;  // syndrome q (of the q-th present parity row) at syn + syn_off + q * syn_stride(B)
    uint64_t dmask;    // bit j: data block j present (k <= 64)
    uint64_t pmask;    // bit r: parity row r present (m - k <= 64)
    uint32_t B;
    uint32_t last;     // bytes of output row k-1 (n - (k-1)*B): its stores stop there (recover-only: B)
    uint32_t slot0;
    uint32_t wq0;      // masks[wq0 + q]: the scaling w of syndrome q (scale_mask)
    uint32_t zq0;      // fused kernel: masks[zq0 + t], the scaling z of the t-th lost row
    uint32_t flags;    // fused kernel: bit 1 = recover-only (recovered rows by rank)
};

struct SynSlots {
    const uint64_t *off;
    const uint32_t *avail;
    const uint64_t *masks;  // scalings of both phases (scale_mask layout)
};

// One chunk of a syndrome decode, phase 2 (kernels_bs.hip sec_solve_bs_kernel; 48 B): the lost
// data rows from the scaled bit-sliced syndromes.
struct SolveDesc {
    uint64_t out_off;
    uint64_t syn_off;  // as SynDesc
    uint64_t lost;     // bit l: data row l is recovered
    uint64_t pmask;    // bit r: parity row r present (syndrome q = the q-th set bit)
    uint32_t B;
    uint32_t last;     // bytes output row k-1 holds (reassembly; recover-only: B)
    uint32_t zq0;      // masks[zq0 + t]: the scaling z of the t-th recovered row (ascending)
    uint32_t recover;  // 1: recovered row t at out_off + t * B (else row l at out_off + l * B)
};

// One chunk of a bit-sliced check (kernels_bs.hip sec_check_bs_kernel; 40 B): all k data blocks are
// held and are the basis, so check row r is zfec's own parity row.  Block j of the chunk (data
// j < k, parity row r at j = k + r) is at blocks + off[slot0 + j] with avail[slot0 + j] readable
// bytes (parity rows: when their bit in pmask is set); rmap[rmap0 + r] is parity row r's check-row
// index, its flag word flags[flag0 + 1 + that] (ChkDesc::flag0: sec_check_final reads them).
struct CbsDesc {
    uint64_t out_off;  // decode + check: the chunk in `out`, the data blocks copied there (tile flag)
    uint64_t pmask;    // bit r: parity row r held (m - k <= 64)
    uint32_t B;
    uint32_t last;     // bytes of output row k-1 (B - padlen): its stores stop there
    uint32_t slot0;
    uint32_t flag0;
    uint32_t rmap0;
    uint32_t pad;
};

struct CbsSlots {
    const uint64_t *off;
    const uint32_t *avail;
    const uint32_t *rmap;
    uint32_t *flags;
};

// One chunk of a bit-sliced repair or repair + check (kernels_bs.hip sec_repair_bs_kernel; 32 B): all
// k data blocks are held and are the basis, so every target and every check row is zfec's own parity
// row.  Blocks as CbsDesc's (off / avail from slot0; a target row's entry is unused).  Parity row r,
// when its bit in tmask is set, is stored whole at out + tgt_off[tmap[rmap0 + r]] (tmap: the row's
// index in the launch's tgt_off, the caller's target order); when its bit in pmask is set it is
// compared, rmap[rmap0 + r] its check-row index as in CbsDesc.  No row is in both masks.
struct RbsDesc {
    uint64_t pmask;  // bit r: parity row r held (compared)
    uint64_t tmask;  // bit r: parity row r is a target (stored)
    uint32_t B;
    uint32_t slot0;
    uint32_t flag0;  // as ChkDesc::flag0 (unused when pmask is 0)
    uint32_t rmap0;  // first of the chunk's m - k entries in RbsSlots::rmap and ::tmap
};

struct RbsSlots {
    const uint64_t *off;
    const uint32_t *avail;
    const uint32_t *rmap;
    const uint32_t *tmap;
    const uint64_t *tgt_off;  // target address: out + tgt_off[target], any byte alignment
    uint32_t *flags;
};

// Syndromes are stored bit-sliced (a lane's 8 planes where its 32 bytes would be), at the
// lanes' unclamped positions: rows of whole 2048-position wave spans.
constexpr uint64_t kSynSpan = 2048;
constexpr uint64_t syn_stride(uint64_t B) { return (B + kSynSpan - 1) / kSynSpan * kSynSpan; }

struct Tile {
    uint32_t chunk;  // descriptor index
    uint32_t t0;     // first byte position within the block
    uint32_t r0;     // first output row of this tile's row group
    uint32_t ntail;  // on the chunk's last tile of the row group: B - valid, the ragged
                     // positions [valid, B) it also computes byte by byte; else 0
};

// Where a launch of nt tiles keeps the map entry of workgroup b inside its own sub-array:
// XCD-major.  Workgroups are dealt round-robin over the 8 XCDs, so in launch order the 8 entries
// of a 128-byte line went to 8 XCDs and each XCD's L2 fetched every line of the map for one entry;
// here the entries of the workgroups b % 8 == x form one contiguous run, run x starting at
// x * (nt / 8) + min(x, nt % 8) (the first nt % 8 runs hold one entry more).  A bijection of
// [0, nt) for every nt, the identity below 16; the planner (bs_plan.hpp append_placed) and the
// kernels (own_tile) share it, so results do not depend on where a workgroup runs.
#ifdef __HIP__
#define SEC_HOST_DEVICE __host__ __device__
#else
#define SEC_HOST_DEVICE
#endif
SEC_HOST_DEVICE inline uint32_t tile_slot(uint32_t b, uint32_t nt)
{
    if (nt < 16)
        return b;
    const uint32_t x = b % 8, r = nt % 8;
    return x * (nt / 8) + (x < r ? x : r) + b / 8;
}

#ifdef __HIP__
// This workgroup's tile, of a launch of one workgroup per tile (gridDim.x tiles); scalar arithmetic
__device__ __forceinline__ Tile own_tile(const Tile *__restrict__ tiles)
{
    return tiles[tile_slot(blockIdx.x, gridDim.x)];
}
#endif

// One byte position handled by the tail kernels.
struct TailItem {
    uint32_t chunk;
    uint32_t t;
};

// One SHA-1 message (a piece): `len` bytes at bases[base] + off, of which the
// first `avail` exist in memory; the rest read as zero (zfec's padding of the
// last data block, which is part of that piece's bytes).
struct MsgDesc {
    uint64_t off;
    uint64_t len;
    uint64_t avail;
    uint32_t base;  // 0 or 1: which of the launch's two base pointers
    uint32_t pad;
};

}  // namespace sec

// launchers (kernels.hip); all enqueue on `stream` and return hipError_t as int
extern "C++" {
// Timing: the next launch's dispatch records `start`, every launch records `stop` (both
// hipEvent_t, or null), until the next call; returns the launches since the previous call.
int sec_launch_events(void *start, void *stop);
// For launchers in other translation units: the events the next dispatch records (as above),
// counted as a launch; pass them to hipExtLaunchKernelGGL.
void sec_next_launch_events(void **start, void **stop);
int sec_launch_expand(const uint8_t *coef, uint32_t ncoef, uint32_t *tabs, void *stream);
// wide: k > kBatchVecs / U (U must be 1): the kernels that load the blocks in several batches
int sec_launch_encode(int rows, int U, int wide, int lanes, const uint8_t *in, uint8_t *par,
                      const sec::EncDesc *descs, const sec::Tile *tiles, uint32_t ntiles, const uint32_t *tabs,
                      void *stream);
// Bit-sliced compile-time-matrix encode (kernels_bs.hip) for the shapes sec_bs_shape knows
// (else -1; rows = 0: the first kernel of that (k, m), else the one of `rows` rows per group):
// all of [0, B) of chunks with B >= 16: group 0 for the one-group shapes, tiles of `lanes`
// (64..256) lanes over lanes / 64 wave spans of sec_bs_span() positions; group -2 for zfec(64,96)
// (two row groups): both groups of one span per two-wave workgroup, one tile per span, `lanes`
// ignored
int sec_bs_shape(int k, int m, int rows = 0);
int sec_bs_groups(int shape);
int sec_bs_rows(int shape);
uint32_t sec_bs_span();
int sec_launch_encode_bs(int shape, int group, int lanes, const uint8_t *in, uint8_t *par, const sec::EncDesc *descs,
                         const sec::Tile *t, uint32_t ntiles, void *stream);
// Syndrome decode, phase 1, for the shapes sec_syn_shape knows (else -1): tiles as the bit-sliced
// encode's (r0 = the row group's first parity row; ntail bit 0 = this tile also copies the
// present primaries to `out`)
int sec_syn_shape(int k, int m);
int sec_launch_syndrome_bs(int shape, int lanes, const uint8_t *blocks, uint8_t *out, uint8_t *syn,
                           const sec::SynDesc *descs, const sec::Tile *t, uint32_t ntiles, sec::SynSlots sl,
                           void *stream);
// Phase 1 of zfec(64,96) chunks with present parity rows in both groups: one two-wave workgroup per
// span (tile t0; ntail bit 0 = copy the present primaries), wave g group g (sec_syn_pair shapes)
int sec_launch_syndrome_bs_pair(int shape, const uint8_t *blocks, uint8_t *out, uint8_t *syn, const sec::SynDesc *descs,
                                const sec::Tile *t, uint32_t ntiles, sec::SynSlots sl, void *stream);
// Both phases in one kernel (e <= 16 and every present parity row in the tile's row group r0):
// the syndromes stay in registers
int sec_launch_decode_bs(int shape, int lanes, const uint8_t *blocks, uint8_t *out, const sec::SynDesc *descs,
                         const sec::Tile *t, uint32_t ntiles, sec::SynSlots sl, void *stream);
// Bit-sliced check (and the copy half of a decode + check that lost nothing) of chunks whose basis
// is their k data blocks (phase 1's item pipeline with a comparing ending): tiles as phase 1's
// (r0 = the row group's first parity row, one tile per span and row group with a held row; ntail
// bit 0 = this tile also copies the data blocks to `out`)
int sec_launch_check_bs(int shape, int lanes, const uint8_t *blocks, uint8_t *out, const sec::CbsDesc *descs,
                        const sec::Tile *t, uint32_t ntiles, sec::CbsSlots sl, void *stream);
// Bit-sliced repair and repair + check of chunks whose basis is their k data blocks (phase 1's item
// pipeline; target rows stored at their own addresses, held rows compared): tiles as the check's
// (r0 = the row group's first parity row, one tile per span and row group with a target or a held
// row; ntail unused)
int sec_launch_repair_bs(int shape, int lanes, const uint8_t *blocks, uint8_t *out, const sec::RbsDesc *descs,
                         const sec::Tile *t, uint32_t ntiles, sec::RbsSlots sl, void *stream);
// The shapes with the two-wave phase-1 kernel (zfec(64,96): both 16-row parity groups)
int sec_syn_pair(int shape);
// Phase 2: the lost data rows of row group r0 / sec_solve_rows(shape) of each tile's chunk
int sec_solve_rows(int shape);
// Phase 2, one workgroup per span (tile t0): the span's e <= slots syndrome rows staged in LDS once,
// each wave one row group; on the shapes sec_solve_lds accepts (slots: a multiple of 8, <= 32)
int sec_solve_lds(int shape);
int sec_launch_solve_bs_lds(int shape, int slots, const uint8_t *syn, uint8_t *out, const sec::SolveDesc *descs,
                            const sec::Tile *t, uint32_t ntiles, const uint64_t *masks, void *stream);
int sec_launch_solve_bs(int shape, int lanes, const uint8_t *syn, uint8_t *out, const sec::SolveDesc *descs,
                        const sec::Tile *t, uint32_t ntiles, const uint64_t *masks, void *stream);
int sec_launch_encode_tail(const uint8_t *in, uint8_t *par, const sec::EncDesc *descs, const sec::TailItem *items,
                           uint32_t nitems, const uint32_t *tabs, void *stream);
// split: sec_sha1_split_kernel (two waves per 64 messages: schedule and rounds) instead of
// one lane per message
int sec_launch_sha1(const uint8_t *base0, const uint8_t *base1, const sec::MsgDesc *msgs, uint32_t nmsgs,
                    uint8_t *digests, void *stream, int split = 0);
// The U = 1 tile kernels over (blocks, out, descs, tiles, tabs, slots), chosen by the descriptor:
//   DecDesc / DecSlots    sec_decode_kernel        rows 0..8 recovered rows of the tile's group
//   RepDesc / RepSlots    sec_repair_kernel        rows 1..8 target rows, each stored whole at its own address
//   ChkDesc / ChkSlots    sec_check_kernel         rows 1..8 check rows; `out` unused: nothing is stored
//                                                  unless a row differs, then only slots.flags words
//   DChkDesc / DChkSlots  sec_decode_check_kernel  rows 0..8 of the chunk's e + nr rows
//   RChkDesc / RChkSlots  sec_repair_check_kernel  rows 1..8 of the chunk's nt + nr rows
// (the check family's results by sec_launch_check_final).  kb (4): the kernel variant whose load
// batch is kb slots (every chunk of the group has k <= kb; not wide); 0: the default batch.
// sec_launch_rows_tail: the same family's byte-granular tail kernel.
template <class Desc, class Slots>
int sec_launch_rows(int rows, int U, int wide, int lanes, const uint8_t *blocks, uint8_t *out, const Desc *descs,
                    const sec::Tile *tiles, uint32_t ntiles, const uint32_t *tabs, Slots slots, void *stream,
                    int kb = 0);
template <class Desc, class Slots>
int sec_launch_rows_tail(const uint8_t *blocks, uint8_t *out, const Desc *descs, const sec::TailItem *items,
                         uint32_t nitems, const uint32_t *tabs, Slots slots, void *stream);
// One thread per entry of the launch's chunks: slots.flags into results[d.res], row_bad[d.cslot0 + ..]
// and, for an inconsistent chunk, column[d.cslot0 + ..] (row_bad, column nullable)
int sec_launch_check_final(const uint8_t *blocks, const sec::ChkDesc *descs, uint32_t nentries, sec::ChkSlots slots,
                           sec::ChkResult *results, uint8_t *row_bad, uint8_t *column, void *stream);
// Decode + correct: sec_decode_correct_kernel over tiles (chunk, t0) that take all rows of their
// positions in groups of `rows` (2, 4 or 8), its byte-granular tail kernel, and, after both, one
// thread per entry: the chunks' words into results[d.res] and hits[d.cslot0 + ..] (hits nullable)
int sec_launch_correct(int rows, const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::Tile *tiles,
                       uint32_t ntiles, const uint32_t *tabs, sec::CorSlots slots, void *stream, uint32_t tmax = 0);
int sec_launch_correct_tail(const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::TailItem *items,
                            uint32_t nitems, const uint32_t *tabs, sec::CorSlots slots, void *stream,
                            uint32_t tmax = 0);
int sec_launch_correct_final(const sec::CorDesc *descs, uint32_t nentries, sec::CorSlots slots, sec::CorResult *results,
                             uint32_t *hits, void *stream);
// tmax != 0: the _ex kernels instead (several errors per position, a chunk's bound min(tmax, nr / 2);
// its table then carries 3n coefficients more, kernels.hip corx_judge), for both operations
// Repair + correct: sec_repair_correct_kernel and its tail kernel over the same tiles and items, the
// targets stored whole at their own addresses; its results by sec_launch_correct_final (slots: off,
// avail, cpos, echunk and flags of the RCorSlots, row / miss unused)
int sec_launch_correct(int rows, const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::Tile *tiles,
                       uint32_t ntiles, const uint32_t *tabs, sec::RCorSlots slots, void *stream, uint32_t tmax = 0);
int sec_launch_correct_tail(const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::TailItem *items,
                            uint32_t nitems, const uint32_t *tabs, sec::RCorSlots slots, void *stream,
                            uint32_t tmax = 0);
}
