// kernels.hip — CDNA4 (gfx950) kernels for GF(2^8) Reed–Solomon encode / decode.
//
// What they compute is zfec's fec_encode / fec_decode (restated in
// oracle/fec_oracle.c; called from /root/reference/storb/util/piece.py:129-130
// and :196-197 through zfec.easyfec):
//     out_r[t] = XOR_j  c_rj * in_j[t]        over GF(2^8) / 0x11D
//
// How.  The work is byte-wise and HBM-bound (a few VALU ops per byte, no
// matrix shape), so there is no MFMA and no LDS in the hot loop:
//   * multiplication by a constant c is GF(2)-linear in the byte x, so with
//     x = lo3 | mid3 << 3 | hi2 << 6
//         c*x = c*lo3  ^  c*(mid3 << 3)  ^  c*(hi2 << 6)
//     and each term is an 8- (or 4-) entry byte table: exactly what one
//     v_perm_b32 looks up for 4 bytes at once (its 8-byte source = the table,
//     its selector = the 3-bit fields).  So one coefficient costs 3 v_perm +
//     2 XOR per dword, and the 3 selectors of an input dword are shared by all
//     output rows.  The tables (5 dwords per coefficient) are wave-uniform and
//     arrive through scalar loads.
//   * the tables themselves are expanded on the device from the coefficient
//     bytes by sec_expand_tables, which stages the GF(2^8) exp/log tables in
//     LDS and forms every product as exp[log c + log v].
//   * each lane streams 16 B (global_load_dwordx4) per block per u-step, so a
//     wave reads one coalesced 1 KiB run from each of the k blocks; block
//     starts that are not 16 B aligned (B % 16 != 0) use the hardware's
//     unaligned dwordx4 access; the last data block's zero padding is
//     synthesised by the byte-granular tail kernels (at most padlen positions per
//     chunk), never read.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.hpp"

using u8 = uint8_t;
using u32 = uint32_t;
using u64 = uint64_t;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));  // byte-aligned 16 B access

namespace {

struct GfTables {
    u8 exp[512];
    u8 log[256];
};

constexpr GfTables make_gf()
{
    GfTables t{};
    u32 v = 1;
    for (int e = 0; e < 255; ++e) {
        t.exp[e] = (u8)v;
        t.exp[e + 255] = (u8)v;
        t.log[v] = (u8)e;
        v <<= 1;
        if (v & 0x100)
            v ^= 0x11D;
    }
    t.exp[510] = t.exp[0];
    t.exp[511] = t.exp[1];
    t.log[0] = 255;  // sentinel; products with 0 are special-cased
    return t;
}

__constant__ GfTables c_gf = make_gf();

// ---- table expansion: coefficient byte -> 5 v_perm tables ---------------
__global__ __launch_bounds__(256) void sec_expand_tables(const u8 *__restrict__ coef, u32 ncoef,
                                                         u32 *__restrict__ tabs)
{
    __shared__ u8 s_exp[512];
    __shared__ u8 s_log[256];
    for (u32 i = threadIdx.x; i < 512; i += blockDim.x)
        s_exp[i] = c_gf.exp[i];
    for (u32 i = threadIdx.x; i < 256; i += blockDim.x)
        s_log[i] = c_gf.log[i];
    __syncthreads();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncoef)
        return;
    const u32 c = coef[i];
    const u32 lc = s_log[c];
    auto mul = [&](u32 v) -> u32 { return (c && v) ? (u32)s_exp[lc + s_log[v]] : 0u; };
    auto pack = [&](u32 a, u32 b, u32 cc, u32 d) { return mul(a) | mul(b) << 8 | mul(cc) << 16 | mul(d) << 24; };
    u32 *o = tabs + (u64)i * sec::kTabDwords;
    o[0] = pack(0, 1, 2, 3);                      // c * lo3,        lo3 = 0..3
    o[1] = pack(4, 5, 6, 7);                      //                 lo3 = 4..7
    o[2] = pack(0 << 3, 1 << 3, 2 << 3, 3 << 3);  // c * (mid3<<3), mid3 = 0..3
    o[3] = pack(4 << 3, 5 << 3, 6 << 3, 7 << 3);  //                 mid3 = 4..7
    o[4] = pack(0 << 6, 1 << 6, 2 << 6, 3 << 6);  // c * (hi2<<6),   hi2 = 0..3
}

// gfx950's three-input bitwise op (v_bitop3_b32, truth table as the immediate).  The
// compiler does not form it from C: a 4-term XOR took 3 v_xor_b32 (GF accumulation, SHA-1
// message schedule) and SHA-1's Maj 2 ops.  Only symmetric tables are used (0x96 = XOR3,
// 0xE8 = Maj), so the operand order of the table does not matter.
__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c)
{
    u32 r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// Ch(b, c, d) = (b & c) | (~b & d); written as C the compiler folded it into the round's
// additions as 3 ops (sub, and, and_or)
__device__ __forceinline__ u32 bfi(u32 b, u32 c, u32 d)
{
    u32 r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(c), "v"(d));
    return r;
}
__device__ __forceinline__ u32 maj(u32 a, u32 b, u32 c)
{
    u32 r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xe8" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ---- the multiply-accumulate ------------------------------------------------
template <int U>
struct Sel {  // the 3 v_perm selectors of each dword of x: bits 0-2, 3-5, 6-7 of every byte
    u32 s0[U][4], s1[U][4], s2[U][4];
    __device__ __forceinline__ explicit Sel(const u32x4 (&x)[U])
    {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const u32 v = x[u][w];
                s0[u][w] = v & 0x07070707u;
                s1[u][w] = (v >> 3) & 0x07070707u;
                s2[u][w] = (v >> 6) & 0x03030303u;
            }
    }
};
__device__ __forceinline__ u32 perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// SEC_LDS_TAB: v_perm is VOP3, which reads at most one SGPR, so with every table dword in
// SGPRs (scalar loads) one source of perm(c[1], c[0]) and of perm(c[3], c[2]) is first copied
// into a VGPR: 2 v_mov per coefficient and wave, 0.5 per dword and row at U = 1 (8 % of C4's
// encode VALU).  With the knob on, each wave keeps dwords 1 and 3 of its batch's coefficients
// in its own slice of LDS (filled by vector loads at the batch's start; the same wave writes
// and reads it, so no barrier), and the products read them with one ds_read_b64 per
// coefficient instead of the two v_mov.
// SEC_LDS_TAB = 0 off, 1 every tile kernel, 2 (default) the encode kernels of 8-row groups
// only.  Against the SGPR-only build (profiles/r02_ldstab.jsonl, one process per shape):
// encode of 8-row groups zfec(16,24) +4 %, (32,48) +1 %, (64,96) +5 %; but C2 encode -6 %,
// C4 -3 %, C5 -6 %, and the wide decodes -35 % (VGPR spills), so it stays off there.
#ifndef SEC_LDS_TAB
#define SEC_LDS_TAB 2
#endif
template <int R, bool DEC>
__host__ __device__ constexpr bool lds_tab() { return SEC_LDS_TAB == 1 || (SEC_LDS_TAB == 2 && !DEC && R == 8); }
using u32x2 = uint2;

// SEC_PROBE_NOGF (build knob, calibration only; never the product): every GF product replaced by
// the block itself (acc ^= x), so a variant library moves exactly the product kernels' bytes with
// the same tiles and descriptors but no field arithmetic -- the access pattern's own ceiling
// (tools/c5_classes.py --lib).  Its outputs are not Reed-Solomon parity.
#ifndef SEC_PROBE_NOGF
#define SEC_PROBE_NOGF 0
#endif

// acc[r] ^= coefficient(r) * x for one block: 3 v_perm + 2 XOR per dword and row
// (t: the block's first row's 5 table dwords; v: its dwords 1 and 3 in LDS, SEC_LDS_TAB only)
template <int R, int U, bool LT = false>
__device__ __forceinline__ void gf_mac(u32x4 (&acc)[R][U], const u32x4 (&x)[U], const u32 *__restrict__ t,
                                       const u32x2 *v)
{
    if constexpr (SEC_PROBE_NOGF) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc[r][u] ^= x[u];
        return;
    }
    const Sel<U> s(x);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32 *c = t + r * 5;
        u32 c1 = c[1], c3 = c[3];
        if constexpr (LT) {
            const u32x2 h = v[r];
            c1 = h.x;
            c3 = h.y;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < 4; ++w)
                acc[r][u][w] = xor3(acc[r][u][w], perm(c1, c[0], s.s0[u][w]), perm(c3, c[2], s.s1[u][w])) ^
                               perm(c[4], c[4], s.s2[u][w]);
    }
}

// In the k <= 16 kernels blocks go to gf_mac2 in pairs only for row groups of <= 4 rows: with 8 rows the second
// block's selectors cost registers, and zfec(16,24) measured encode -14 %, decode -42 %
// (C4 encode +12 %, C2 +1 %; profiles/r01_sweep_xor3.jsonl)
// The wide-k (W) kernels load smaller batches (SEC_WIDE_BATCH), which leaves the registers
// to pair blocks for 8-row groups too: zfec(32,48) / (64,96) encode +11 %, decode +7-10 %
// (profiles/r01_sweep_wide_pair.jsonl).
#ifndef SEC_PAIR_ROWS
#define SEC_PAIR_ROWS 4
#endif
#ifndef SEC_WIDE_PAIR_ROWS
#define SEC_WIDE_PAIR_ROWS 8
#endif
template <int R, bool W>
__host__ __device__ constexpr bool kPairRows() { return R <= (W ? SEC_WIDE_PAIR_ROWS : SEC_PAIR_ROWS); }

// Two blocks at once: the 6 products of a dword and row go into acc by 3 XOR3s, so 3 v_perm
// + 1.5 XOR per dword, row and block (a 4-term XOR chain in C took 3 v_xor_b32 per block)
template <int R, int U, bool LT = false>
__device__ __forceinline__ void gf_mac2(u32x4 (&acc)[R][U], const u32x4 (&x)[U], const u32 *__restrict__ t,
                                        const u32x2 *v, const u32x4 (&y)[U], const u32 *__restrict__ q,
                                        const u32x2 *vq)
{
    if constexpr (SEC_PROBE_NOGF) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc[r][u] ^= x[u] ^ y[u];
        return;
    }
    const Sel<U> s(x), z(y);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32 *c = t + r * 5, *d = q + r * 5;
        u32 c1 = c[1], c3 = c[3], d1 = d[1], d3 = d[3];
        if constexpr (LT) {
            const u32x2 h = v[r], g = vq[r];
            c1 = h.x;
            c3 = h.y;
            d1 = g.x;
            d3 = g.y;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                u32 a = xor3(acc[r][u][w], perm(c1, c[0], s.s0[u][w]), perm(c3, c[2], s.s1[u][w]));
                a = xor3(a, perm(c[4], c[4], s.s2[u][w]), perm(d1, d[0], z.s0[u][w]));
                acc[r][u][w] = xor3(a, perm(d3, d[2], z.s1[u][w]), perm(d[4], d[4], z.s2[u][w]));
            }
    }
}

// SEC_LDS_TAB: this wave's LDS slice, filled by its active lanes with dwords 1 and 3 of the tables of blocks
// j0 .. j0 + KB - 1 (those < k), rows 0 .. R - 1 (tj: row 0 of block 0, tstep: dwords per
// block), entry c * R + r.  The launch passes (lanes / 64) * KB * R * 8 bytes of dynamic LDS.
template <int KB, int R, bool LT>
__device__ __forceinline__ const u32x2 *wave_tabs(const u32 *__restrict__ tj, u32 tstep, u32 j0, u32 k)
{
    extern __shared__ u32x2 s_vt[];
    u32x2 *vt = s_vt + (threadIdx.x >> 6) * (KB * R);
    if constexpr (LT && R > 0) {
        // the wave's active lanes share the fill (lanes past a tile's `valid` never get here)
        const u64 live = __builtin_amdgcn_read_exec();
        const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(live >> 32), __builtin_amdgcn_mbcnt_lo((u32)live, 0u));
        const u32 nlive = (u32)__builtin_popcountll(live);
        for (u32 i = rank; i < (u32)(KB * R); i += nlive) {
            const u32 c = i / R, r = i % R;
            if (j0 + c < k) {
                const u32 *src = tj + (j0 + c) * tstep + r * sec::kTabDwords;
                vt[i] = u32x2{src[1], src[3]};
            }
        }
    }
    return vt;
}
// Dynamic LDS bytes of a tile launch (0 without SEC_LDS_TAB)
template <int KB, int R, bool DEC>
constexpr u32 lds_tab_bytes(u32 lanes) { return lds_tab<R, DEC>() ? lanes / 64 * KB * R * 8 : 0; }

// Build knobs (A/B variants are compiled as separate libraries by tools/sweep.py):
//   SEC_NT_LOAD / SEC_NT_STORE  nontemporal (streaming) global loads / stores: every
//                               byte is touched once, so keeping it out of the caches
//                               measured +11% on encode, +4% on decode (r01 sweep)
//   SEC_ENC_BATCH / SEC_DEC_BATCH  16-byte vectors per lane loaded as one batch (all
//                               issued before any arithmetic): KB = this / U blocks (slots)
//                               per batch.  Decode batching: C2 +4 %, RS(8,3) +6.6 %, C4 +2 %
//                               (r01 sweep_dec_batch); encode: C2 +3.5 %, C4 +9 %
//   SEC_ENC_ST / SEC_DEC_ST     store cache policy of the encode / decode kernels:
//                               0 plain, 1 nt, 2 "nt sc1" (write-through, line dropped from
//                               L2), 3 "sc0 sc1".  The asm forms end in s_nop 1: a store of
//                               more than 8 bytes reads its data VGPRs after issue, and the
//                               compiler, blind to the asm, may overwrite them at once
#ifndef SEC_NT_LOAD
#define SEC_NT_LOAD 1
#endif
#ifndef SEC_NT_STORE
#define SEC_NT_STORE 1
#endif
#ifndef SEC_ENC_ST
#define SEC_ENC_ST SEC_NT_STORE
#endif
#ifndef SEC_DEC_ST
#define SEC_DEC_ST SEC_NT_STORE
#endif
#ifndef SEC_DEC_BATCH
#define SEC_DEC_BATCH sec::kBatchVecs
#endif
#ifndef SEC_ENC_BATCH
#define SEC_ENC_BATCH sec::kBatchVecs
#endif
//   SEC_WIDE_BATCH              vectors per batch in the wide-k (W) kernels, which loop over
//                               batches; default: the encode / decode batch
#ifndef SEC_WIDE_BATCH
#define SEC_WIDE_BATCH 8
#endif
//   (Rounds 1-5 also tried, and archived: a compile-time k for single-shape workloads, VGPR caps
//   through amdgpu_waves_per_eu, LDS padding to cap the decode's workgroups per CU.  SEC_DEC_LATE,
//   the decode's copies as each slot arrives instead of after the batch's arithmetic, is gone too:
//   after the arithmetic measured C4 decode +5 %, profiles/r01_sweep_declate.jsonl.)
// Blocks (slots) per batch of a tile kernel: KB * U = the batch's 16 B vectors per lane
template <int U, bool W, bool DEC>
constexpr int batch_blocks()
{
    constexpr int v = (W && SEC_WIDE_BATCH > 0) ? SEC_WIDE_BATCH : (DEC ? SEC_DEC_BATCH : SEC_ENC_BATCH);
    return v / U > 0 ? v / U : 1;
}

__device__ __forceinline__ u32x4 load16(const u8 *p)
{
#if SEC_NT_LOAD
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4_u *>(p));
#else
    return *reinterpret_cast<const u32x4_u *>(p);
#endif
}
template <int POL>
__device__ __forceinline__ void store16(u8 *p, u32x4 v)
{
    if constexpr (POL == 0)
        *reinterpret_cast<u32x4_u *>(p) = v;
    else if constexpr (POL == 1)
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4_u *>(p));
    else if constexpr (POL == 2)
        asm volatile("global_store_dwordx4 %0, %1, off nt sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// GF(2^8) product of one byte through the same 5-dword table (tail kernels)
__device__ __forceinline__ u32 gf_mul_byte(const u32 *__restrict__ t, u32 x)
{
    return (__builtin_amdgcn_perm(t[1], t[0], x & 7u) ^ __builtin_amdgcn_perm(t[3], t[2], (x >> 3) & 7u) ^
            __builtin_amdgcn_perm(t[4], t[4], x >> 6)) & 0xFFu;
}

// ---- the parts the tile kernels' bodies share ----
// (Only what compiles to the instruction streams of the code it replaced.  The accumulator
// zeroing, the batched slot load and the pair / single dispatch stay written out in encode_main,
// decode_main and repair_main: as helpers, each of the three changed register allocation and
// instruction counts of the kernels, by a few instructions up to 36 of about 5000.)
// The lane's U positions, one per u-step of the workgroup, clamped so its 16 bytes end at `valid`
template <int U>
__device__ __forceinline__ void tile_pos(u32 (&pos)[U], u32 t, u32 valid)
{
    const u32 step = blockDim.x * sec::kLaneBytes;  // bytes one u-step of the workgroup covers
#pragma unroll
    for (int u = 0; u < U; ++u)
        pos[u] = min(t + u * step, valid - sec::kLaneBytes);
}

// acc[r] ^= coefficient(row0 + r) * x for one byte of one slot (tab: the chunk's tables, row0:
// the slot's first table of this row group)
template <int R, int N>
__device__ __forceinline__ void gf_mac_bytes(u32 (&acc)[N], const u32 *__restrict__ tab, u32 row0, u32 x)
{
#pragma unroll
    for (int r = 0; r < R; ++r)
        acc[r] ^= gf_mul_byte(tab + (row0 + r) * sec::kTabDwords, x);
}

// ---- encode ----------------------------------------------------------------
// Tile = (chunk, t0, r0): lanes cover t0 + 16*lane + 4096*u.  Every position handled here
// is < `valid` (all k blocks fully readable there, including the last, shorter data
// block); a lane's 16 bytes are clamped to end at `valid`, so the last lane of a ragged
// chunk overlaps its neighbour (identical bytes written twice) instead of taking a
// byte-granular path.  Positions in [valid, B) — at most padlen of them — are computed
// byte by byte by the chunk's last tile (Tile::ntail, encode_ragged) after its main work.
template <int R, int U, bool W>
__device__ __forceinline__ void encode_main(const u8 *__restrict__ in, u8 *__restrict__ par, const sec::EncDesc &d,
                                            const sec::Tile &tl, const u32 *__restrict__ tabs, u32 t);
template <int R>
__device__ __forceinline__ void encode_ragged(const u8 *__restrict__ in, u8 *__restrict__ par, const sec::EncDesc &d,
                                           const sec::Tile &tl, const u32 *__restrict__ tabs);

template <int R, int U, bool W>
__global__ __launch_bounds__(sec::max_lanes(R, U)) void sec_encode_kernel(const u8 *__restrict__ in, u8 *__restrict__ par,
                                                         const sec::EncDesc *__restrict__ descs,
                                                         const sec::Tile *__restrict__ tiles,
                                                         const u32 *__restrict__ tabs)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::EncDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t < d.valid)
        encode_main<R, U, W>(in, par, d, tl, tabs, t);
    if (tl.ntail)
        encode_ragged<R>(in, par, d, tl, tabs);
}

template <int R, int U, bool W>
__device__ __forceinline__ void encode_main(const u8 *__restrict__ in, u8 *__restrict__ par, const sec::EncDesc &d,
                                            const sec::Tile &tl, const u32 *__restrict__ tabs, u32 t)
{
    const u32 B = d.B, k = d.k;
    u32 pos[U];
    tile_pos(pos, t, d.valid);
    const u8 *row = in + d.in_off;
    u8 *dst = par + d.par_off + (u64)tl.r0 * d.par_stride;
    const u32 *tj = tabs + d.tab + tl.r0 * sec::kTabDwords;
    const u32 tstep = d.p * sec::kTabDwords;

    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // Blocks go in batches of KB: every load of a batch is issued before any arithmetic and
    // the batch is consumed in order (counted waits), so a lane keeps KB * U = SEC_ENC_BATCH
    // loads in flight; C2 (k = 4) and C4 (k = 10) are one batch.  A one-block-ahead prefetch
    // loop compiled to a full wait at its head (the next block's load included): one load in
    // flight per lane and u-step, C2 -3.5 %, C4 -9 % (profiles/r01_sweep_enc_batch.jsonl).
    constexpr int KB = batch_blocks<U, W, false>();
    auto batch = [&](u32 j0) {
        constexpr bool LT = lds_tab<R, false>();
        const u32x2 *vt = wave_tabs<KB, R, LT>(tj, tstep, j0, k);
        u32x4 xs[KB][U];
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (j0 + c < k) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    xs[c][u] = load16(row + (u64)(j0 + c) * B + pos[u]);
            }
        if constexpr (kPairRows<R, W>()) {
#pragma unroll
            for (int c = 0; c < KB; c += 2) {
                if (c + 1 < KB && j0 + c + 1 < k)
                    gf_mac2<R, U, LT>(acc, xs[c], tj + (j0 + c) * tstep, vt + c * R, xs[c + 1],
                                  tj + (j0 + c + 1) * tstep, vt + (c + 1) * R);
                else if (j0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (j0 + c) * tstep, vt + c * R);
            }
        } else {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (j0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (j0 + c) * tstep, vt + c * R);
        }
    };
    // W (wide k, U = 1 only): k > KB, several batches.  A separate instantiation: merely
    // compiling this loop into the k <= KB kernel cost C4 15 % (registers; r01 sweep_wide).
    if constexpr (W) {
#pragma unroll 1
        for (u32 j0 = 0; j0 < k; j0 += KB)
            batch(j0);
    } else {
        batch(0);  // the plan guarantees k <= KB here
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            store16<SEC_ENC_ST>(dst + (u64)r * d.par_stride + pos[u], acc[r][u]);
}

// Lane of the workgroup that takes ragged position i first: the lanes past the tile's main
// range (idle there) come first, then the wrap reaches the busy ones.
__device__ __forceinline__ u32 ragged_lane0(u32 valid, u32 t0)
{
    const u32 used = min(blockDim.x, (valid - t0 + sec::kLaneBytes - 1) / sec::kLaneBytes);
    return (threadIdx.x + blockDim.x - used) % blockDim.x;
}

// The chunk's ragged end [valid, valid + ntail), byte by byte, for this tile's R parity rows:
// blocks 0..k-2 are full there and block k-1 is zero padding, so it contributes nothing.
// Each lane issues its bytes' loads kBatch at a time before using any (a loop of dependent
// single-byte loads costs one memory latency per block).
constexpr u32 kBatch = 16;

// Byte tp of slots c0 .. c0 + kBatch - 1 of a decode / repair chunk: zero for slots >= k and for
// bytes past a slot's avail
template <class Slots>
__device__ __forceinline__ void load_slot_bytes(u32 (&x)[kBatch], const u8 *__restrict__ blocks, const Slots &sl,
                                                u32 slot0, u32 c0, u32 k, u32 tp)
{
#pragma unroll
    for (u32 q = 0; q < kBatch; ++q)
        x[q] = (c0 + q < k && tp < sl.avail[slot0 + c0 + q]) ? (u32)blocks[sl.off[slot0 + c0 + q] + tp] : 0u;
}

template <int R>
__device__ __forceinline__ void encode_ragged(const u8 *__restrict__ in, u8 *__restrict__ par, const sec::EncDesc &d,
                                              const sec::Tile &tl, const u32 *__restrict__ tabs)
{
    const u8 *src = in + d.in_off;
    const u32 nblk = d.k - 1;
    for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x) {
        const u32 tp = d.valid + i;
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0;
        for (u32 j0 = 0; j0 < nblk; j0 += kBatch) {
            u32 x[kBatch];
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                x[q] = j0 + q < nblk ? (u32)src[(u64)(j0 + q) * d.B + tp] : 0u;
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                if (j0 + q < nblk) {
                    const u32 *tj = tabs + d.tab + ((j0 + q) * d.p + tl.r0) * sec::kTabDwords;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        acc[r] ^= gf_mul_byte(tj + r * sec::kTabDwords, x[q]);
                }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            par[d.par_off + (u64)(tl.r0 + r) * d.par_stride + tp] = (u8)acc[r];
    }
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16):
// all p parity bytes at that position, the last block's padding read as zero.
__global__ __launch_bounds__(256) void sec_encode_tail(const u8 *__restrict__ in, u8 *__restrict__ par,
                                                       const sec::EncDesc *__restrict__ descs,
                                                       const sec::TailItem *__restrict__ items, u32 nitems,
                                                       const u32 *__restrict__ tabs)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::EncDesc d = descs[it.chunk];
    const u8 *src = in + d.in_off + it.t;
    for (u32 r = 0; r < d.p; ++r) {
        u32 acc = 0;
        for (u32 j = 0; j < d.k; ++j) {
            const u32 x = (j + 1 < d.k || it.t < d.valid) ? (u32)src[(u64)j * d.B] : 0u;
            acc ^= gf_mul_byte(tabs + d.tab + (j * d.p + r) * sec::kTabDwords, x);
        }
        par[d.par_off + (u64)r * d.par_stride + it.t] = (u8)acc;
    }
}

// ---- decode + reassemble -----------------------------------------------------
// Slot c of a chunk holds block number idx[c]; primaries sit in their own slot
// (zfec's normalisation).  Present primaries are copied to their output row;
// the R missing rows of this tile's row group are XOR_c Minv[row][c] * slot_c.
// Positions are < valid = min(the last output row's length, every slot's avail), so every
// row is writable and every slot readable there; the rest is decode_ragged's (Tile::ntail),
// which reads a slot's bytes past its avail as zero (zfec's padded block k-1 read in place).
// Recover-only decodes (SEC_F_RECOVER) use the same kernels: no copies (row = none) and the
// recovered rows go to output rows 0..e-1.
template <int R, int U, bool W, int KBX>
__device__ __forceinline__ void decode_main(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                            const sec::DecDesc &d, const sec::Tile &tl, u32 t,
                                            const u32 *__restrict__ tabs, const sec::DecSlots sl);
template <int R>
__device__ __forceinline__ void decode_ragged(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::DecDesc &d,
                                           const sec::Tile &tl, const u32 *__restrict__ tabs,
                                           const sec::DecSlots sl);

// KBX > 0: slots per load batch fixed at KBX (the plan sends only chunks with k <= KBX; fewer
// live registers, more waves): recover-only and copy-free decodes, see api.cpp dec_small_kb
template <int R, int U, bool W, int KBX>
__global__ __launch_bounds__(sec::max_lanes(R, U)) void sec_decode_kernel(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                         const sec::DecDesc *__restrict__ descs,
                                                         const sec::Tile *__restrict__ tiles,
                                                         const u32 *__restrict__ tabs,
                                                         const sec::DecSlots sl)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::DecDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t < d.valid)
        decode_main<R, U, W, KBX>(blocks, out, d, tl, t, tabs, sl);
    if (tl.ntail)
        decode_ragged<R>(blocks, out, d, tl, tabs, sl);
}

// The chunk's ragged end [valid, valid + ntail), byte by byte: the present primaries' bytes
// (row group 0) and this tile's R recovered rows, wherever the output row still has bytes.
// Every slot's byte is loaded once, kBatch slots at a time, and feeds the copy and all R rows.
template <int R>
__device__ __forceinline__ void decode_ragged(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::DecDesc &d,
                                              const sec::Tile &tl, const u32 *__restrict__ tabs,
                                              const sec::DecSlots sl)
{
    for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x) {
        const u32 tp = d.valid + i;
        u8 *dst = out + d.out_off + tp;
        u32 acc[R > 0 ? R : 1];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0;
        for (u32 c0 = 0; c0 < d.k; c0 += kBatch) {
            u32 x[kBatch];
            load_slot_bytes(x, blocks, sl, d.slot0, c0, d.k, tp);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                if (c0 + q < d.k) {
                    const u32 c = c0 + q;
                    const u32 orow = sl.row[d.slot0 + c];
                    if (tl.r0 == 0 && orow != 0xFFFFFFFFu && (u64)orow * d.B + tp < d.n)
                        dst[(u64)orow * d.B] = (u8)x[q];
                    gf_mac_bytes<R>(acc, tabs + d.tab, c * d.e + tl.r0, x[q]);
                }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u32 orow = sl.miss[d.slot0 + tl.r0 + r];
            if ((u64)orow * d.B + tp < d.n)
                dst[(u64)orow * d.B] = (u8)acc[r];
        }
    }
}

template <int R, int U, bool W, int KBX>
__device__ __forceinline__ void decode_main(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                            const sec::DecDesc &d, const sec::Tile &tl, u32 t,
                                            const u32 *__restrict__ tabs,
                                                         const sec::DecSlots sl)
{
    const u32 B = d.B, k = d.k;
    u32 pos[U];
    tile_pos(pos, t, d.valid);
    u8 *dst = out + d.out_off;
    const bool copies = tl.r0 == 0;  // row group 0 also copies the present primaries
    const u32 *tj = tabs + d.tab + tl.r0 * sec::kTabDwords;
    const u32 tstep = d.e * sec::kTabDwords;

    u32x4 acc[R > 0 ? R : 1][U];
#pragma unroll
    for (int r = 0; r < (R > 0 ? R : 1); ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // Slots go in batches of KB, as in encode_main: every load of a batch before any store
    // or arithmetic, then every slot fed to the R accumulators, then each present primary
    // copied to its output row (copies as each slot arrives measured C4 decode -5 %).  C2 / C4
    // are one batch (all loads in flight).
    constexpr int KB = KBX > 0 ? KBX : batch_blocks<U, W, true>();
    auto batch = [&](u32 c0) {
        constexpr bool LT = lds_tab<R, true>();
        const u32x2 *vt = wave_tabs<KB, R, LT>(tj, tstep, c0, k);
        // the batch's block offsets in one go (the plan pads sl.off by kBatchVecs entries): one
        // offset loaded and waited for per slot would put KB scalar round trips before the last load
        u64 so[KB];
        const u64 *sop = sl.off + d.slot0 + c0;
#pragma unroll
        for (int c = 0; c < KB; ++c)
            so[c] = sop[c];
        u32x4 xs[KB][U];
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u8 *s = blocks + so[c];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    xs[c][u] = load16(s + pos[u]);
            }
        if constexpr (R > 0 && kPairRows<R, W>()) {
#pragma unroll
            for (int c = 0; c < KB; c += 2) {
                if (c + 1 < KB && c0 + c + 1 < k)
                    gf_mac2<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R, xs[c + 1],
                                      tj + (c0 + c + 1) * tstep, vt + (c + 1) * R);
                else if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
            }
        } else if constexpr (R > 0) {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
        }
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u32 orow = sl.row[d.slot0 + c0 + c];
                if (copies && orow != 0xFFFFFFFFu) {
                    u8 *o = dst + (u64)orow * B;
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        store16<SEC_DEC_ST>(o + pos[u], xs[c][u]);
                }
            }
    };
    if constexpr (W) {  // wide k: several batches (see encode_main)
#pragma unroll 1
        for (u32 c0 = 0; c0 < k; c0 += KB)
            batch(c0);
    } else {
        batch(0);  // the plan guarantees k <= KB here
    }
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u8 *o = dst + (u64)sl.miss[d.slot0 + tl.r0 + r] * B;
#pragma unroll
            for (int u = 0; u < U; ++u)
                store16<SEC_DEC_ST>(o + pos[u], acc[r][u]);
        }
    }
}

// One thread per (chunk, position) outside the main kernel's range: copies and
// recovered bytes for every output row that is still inside the chunk there.
__global__ __launch_bounds__(256) void sec_decode_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                       const sec::DecDesc *__restrict__ descs,
                                                       const sec::TailItem *__restrict__ items, u32 nitems,
                                                       const u32 *__restrict__ tabs,
                                                       const sec::DecSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::DecDesc d = descs[it.chunk];
    u8 *dst = out + d.out_off + it.t;
    auto slot_byte = [&](u32 c) -> u32 {  // bytes past the slot's avail read as zero
        return it.t < sl.avail[d.slot0 + c] ? (u32)blocks[sl.off[d.slot0 + c] + it.t] : 0u;
    };
    for (u32 c = 0; c < d.k; ++c) {
        const u32 orow = sl.row[d.slot0 + c];
        if (orow != 0xFFFFFFFFu && (u64)orow * d.B + it.t < d.n)
            dst[(u64)orow * d.B] = (u8)slot_byte(c);
    }
    for (u32 r = 0; r < d.e; ++r) {
        const u32 orow = sl.miss[d.slot0 + r];
        if ((u64)orow * d.B + it.t >= d.n)
            continue;
        u32 acc = 0;
        for (u32 c = 0; c < d.k; ++c)
            acc ^= gf_mul_byte(tabs + d.tab + (c * d.e + r) * sec::kTabDwords, slot_byte(c));
        dst[(u64)orow * d.B] = (u8)acc;
    }
}

// ---- repair: lost pieces from any k survivors ---------------------------------
// Target row r of a chunk is XOR_c Rm[r][c] * slot_c, Rm = E[targets] * Minv (gf_host.hpp
// repair_matrix): a lost data block or a lost parity block alike.  The decomposition is the
// direct decode's (tile = chunk, t0, r0; up to 8 target rows per group, every group re-reading
// the k slots), with three differences: nothing is copied (R >= 1), every row is a whole B-byte
// piece (block k-1's zero padding included, as computed bytes), and every row is stored at an
// address of its own, out + tgt_off[tgt0 + r0 + r], at any byte alignment (a piece is its own
// buffer: a Python bytes payload starts at a header offset), hence the unaligned 16 B stores.
// Positions < valid = min(B, every slot's avail) are the tiles'; [valid, B) goes byte by byte on
// the chunk's last tile of each row group, a slot's bytes past its avail reading as zero.
template <int R, int U, bool W, int KBX>
__device__ __forceinline__ void repair_main(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                            const sec::RepDesc &d, const sec::Tile &tl, u32 t,
                                            const u32 *__restrict__ tabs, const sec::RepSlots sl)
{
    const u32 k = d.k;
    u32 pos[U];
    tile_pos(pos, t, d.valid);
    const u32 *tj = tabs + d.tab + tl.r0 * sec::kTabDwords;
    const u32 tstep = d.nt * sec::kTabDwords;

    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // slots in batches of KB, every load of a batch before its arithmetic (decode_main)
    constexpr int KB = KBX > 0 ? KBX : batch_blocks<U, W, true>();
    auto batch = [&](u32 c0) {
        constexpr bool LT = lds_tab<R, true>();
        const u32x2 *vt = wave_tabs<KB, R, LT>(tj, tstep, c0, k);
        u64 so[KB];  // (the plan pads sl.off by kBatchVecs entries)
        const u64 *sop = sl.off + d.slot0 + c0;
#pragma unroll
        for (int c = 0; c < KB; ++c)
            so[c] = sop[c];
        u32x4 xs[KB][U];
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u8 *s = blocks + so[c];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    xs[c][u] = load16(s + pos[u]);
            }
        if constexpr (kPairRows<R, W>()) {
#pragma unroll
            for (int c = 0; c < KB; c += 2) {
                if (c + 1 < KB && c0 + c + 1 < k)
                    gf_mac2<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R, xs[c + 1],
                                      tj + (c0 + c + 1) * tstep, vt + (c + 1) * R);
                else if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
            }
        } else {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
        }
    };
    if constexpr (W) {  // wide k: several batches (see encode_main)
#pragma unroll 1
        for (u32 c0 = 0; c0 < k; c0 += KB)
            batch(c0);
    } else {
        batch(0);  // the plan guarantees k <= KB here
    }
    const u64 *to = sl.tgt_off + d.tgt0 + tl.r0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        u8 *o = out + to[r];
#pragma unroll
        for (int u = 0; u < U; ++u)
            store16<SEC_DEC_ST>(o + pos[u], acc[r][u]);
    }
}

// The chunk's ragged end [valid, valid + ntail) = [valid, B), byte by byte, for this tile's R
// target rows: every slot's byte loaded once, kBatch slots at a time, zero past the slot's avail.
template <int R>
__device__ __forceinline__ void repair_ragged(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                              const sec::RepDesc &d, const sec::Tile &tl,
                                              const u32 *__restrict__ tabs, const sec::RepSlots sl)
{
    const u64 *to = sl.tgt_off + d.tgt0 + tl.r0;
    for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x) {
        const u32 tp = d.valid + i;
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0;
        for (u32 c0 = 0; c0 < d.k; c0 += kBatch) {
            u32 x[kBatch];
            load_slot_bytes(x, blocks, sl, d.slot0, c0, d.k, tp);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                if (c0 + q < d.k)
                    gf_mac_bytes<R>(acc, tabs + d.tab, (c0 + q) * d.nt + tl.r0, x[q]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            out[to[r] + tp] = (u8)acc[r];
    }
}

// KBX > 0: slots per load batch fixed at KBX, as sec_decode_kernel's (api.cpp dec_small_kb)
template <int R, int U, bool W, int KBX = 0>
__global__ __launch_bounds__(sec::max_lanes(R, U)) void sec_repair_kernel(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                         const sec::RepDesc *__restrict__ descs,
                                                         const sec::Tile *__restrict__ tiles,
                                                         const u32 *__restrict__ tabs,
                                                         const sec::RepSlots sl)
{
    static_assert(R >= 1, "a repair tile has target rows: nothing is copied");
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::RepDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t < d.valid)
        repair_main<R, U, W, KBX>(blocks, out, d, tl, t, tabs, sl);
    if (tl.ntail)
        repair_ragged<R>(blocks, out, d, tl, tabs, sl);
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16): every
// target row's byte there.
__global__ __launch_bounds__(256) void sec_repair_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                       const sec::RepDesc *__restrict__ descs,
                                                       const sec::TailItem *__restrict__ items, u32 nitems,
                                                       const u32 *__restrict__ tabs,
                                                       const sec::RepSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::RepDesc d = descs[it.chunk];
    auto slot_byte = [&](u32 c) -> u32 {  // bytes past the slot's avail read as zero
        return it.t < sl.avail[d.slot0 + c] ? (u32)blocks[sl.off[d.slot0 + c] + it.t] : 0u;
    };
    for (u32 r = 0; r < d.nt; ++r) {
        u32 acc = 0;
        for (u32 c = 0; c < d.k; ++c)
            acc ^= gf_mul_byte(tabs + d.tab + (c * d.nt + r) * sec::kTabDwords, slot_byte(c));
        out[sl.tgt_off[d.tgt0 + r] + it.t] = (u8)acc;
    }
}

// ---- check: the held pieces of a chunk against each other ---------------------------------------
// Check row r of a chunk, as predicted from its k basis slots (XOR_c Rm[r][c] * slot_c, the repair
// matrix's row for that block), must equal the stored block.  The decomposition, the tables and
// the slot loads are repair_main's (a sibling, not a shared body: see DESIGN §5 "Check"); what
// differs is both ends.  The accumulators start as the stored rows instead of zero (kRowsFirst), so
// those loads are the first the lane issues and their latency lies under the slots' loads and the
// arithmetic; after the last slot an accumulator IS predicted ^ stored.
// The epilogue ORs the accumulators: all zero (the clean path) ends the lane with no store at all.
// Otherwise the row's flag word is cleared (plain store; every writer stores the same 0) and the
// position of its first differing byte goes into the chunk's word by atomicMin.
// Positions < valid = min(B, every entry's avail) are the tiles'; [valid, B) goes byte by byte on
// the chunk's last tile of each row group, an entry's bytes past its avail reading as zero.
//
// When a tile loads its stored rows.  Loaded ahead of the slots, the compiler keeps them in
// registers of their own through the arithmetic and XORs them in last (it reorders the XOR chain):
// 4 VGPRs per row on top of repair's.  Where that no longer fits the 128 VGPRs of a 1024-lane
// workgroup (8 rows over the wide-k batches; 7 and 8 rows over a 16-slot batch: 10, 4 and 20 VGPRs
// spilled, tools/kres.py) they are loaded later, into registers the slots have freed: over a
// 16-slot batch half-way through it (kRowsMid), with the other half's arithmetic still ahead of
// them; in the wide-k loop after the last slot (kRowsLast).
constexpr int kRowsFirst = 0, kRowsMid = 1, kRowsLast = 2;
template <int R, bool W, int KB>
constexpr int check_rows_when()
{
    return W ? (R <= 7 ? kRowsFirst : kRowsLast) : (KB <= 4 || R <= 6 ? kRowsFirst : kRowsMid);
}

__device__ __forceinline__ void check_report(const sec::ChkDesc &d, const sec::ChkSlots sl, u32 row, u32 at)
{
    atomicMin(sl.flags + d.flag0, at);
    sl.flags[d.flag0 + 1 + row] = 0u;
}

template <int R, int U, bool W, int KBX>
__device__ __forceinline__ void check_main(const u8 *__restrict__ blocks, const sec::ChkDesc &d, const sec::Tile &tl,
                                           u32 t, const u32 *__restrict__ tabs, const sec::ChkSlots sl)
{
    const u32 k = d.k;
    u32 pos[U];
    tile_pos(pos, t, d.valid);
    const u32 *tj = tabs + d.tab + tl.r0 * sec::kTabDwords;
    const u32 tstep = d.nr * sec::kTabDwords;

    constexpr int KB = KBX > 0 ? KBX : batch_blocks<U, W, true>();
    constexpr int WHEN = check_rows_when<R, W, KB>();
    const u64 *ro = sl.off + d.slot0 + k + tl.r0;  // the stored rows of this group
    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u8 *s = blocks + ro[r];
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc[r][u] = WHEN == kRowsFirst ? load16(s + pos[u]) : u32x4{0u, 0u, 0u, 0u};
    }
    // kRowsMid / kRowsLast: the stored rows into registers the slots have left.  The empty asm
    // makes the lane's position wait for an accumulator as it stands at that point, so the loads
    // cannot be hoisted above the arithmetic before it, where they would spill.
    u32x4 st[R][U];
    auto load_rows = [&]() {
#pragma unroll
        for (int u = 0; u < U; ++u)
            asm volatile("" : "+v"(pos[u]) : "v"(acc[R - 1][u][3]));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u8 *s = blocks + ro[r];
#pragma unroll
            for (int u = 0; u < U; ++u)
                st[r][u] = load16(s + pos[u]);
        }
    };

    // slots in batches of KB, every load of a batch before its arithmetic (decode_main)
    auto batch = [&](u32 c0) {
        constexpr bool LT = lds_tab<R, true>();
        const u32x2 *vt = wave_tabs<KB, R, LT>(tj, tstep, c0, k);
        u64 so[KB];  // (the plan pads sl.off by kBatchVecs entries)
        const u64 *sop = sl.off + d.slot0 + c0;
#pragma unroll
        for (int c = 0; c < KB; ++c)
            so[c] = sop[c];
        u32x4 xs[KB][U];
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u8 *s = blocks + so[c];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    xs[c][u] = load16(s + pos[u]);
            }
        if constexpr (kPairRows<R, W>()) {
#pragma unroll
            for (int c = 0; c < KB; c += 2) {
                if (c + 1 < KB && c0 + c + 1 < k)
                    gf_mac2<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R, xs[c + 1],
                                      tj + (c0 + c + 1) * tstep, vt + (c + 1) * R);
                else if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
            }
        } else {
#pragma unroll
            for (int c = 0; c < KB; ++c) {
                if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
                if constexpr (WHEN == kRowsMid)
                    if (c == KB / 2 - 1)
                        load_rows();
            }
        }
    };
    static_assert(WHEN != kRowsMid || (!W && !kPairRows<R, W>()), "kRowsMid: one batch, slots one by one");
    if constexpr (W) {  // wide k: several batches (see encode_main)
#pragma unroll 1
        for (u32 c0 = 0; c0 < k; c0 += KB)
            batch(c0);
    } else {
        batch(0);  // the plan guarantees k <= KB here
    }
    if constexpr (WHEN == kRowsLast)
        load_rows();
    if constexpr (WHEN != kRowsFirst) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc[r][u] ^= st[r][u];
    }
    u32 any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            any |= acc[r][u][0] | acc[r][u][1] | acc[r][u][2] | acc[r][u][3];
    if (any == 0)
        return;
    // (one pointer and constant offsets: a word address per row, formed ahead of the branch, cost
    // the 8-row kernels scalar registers they do not have)
    u32 *first = sl.flags + d.flag0, *rows = first + 1 + tl.r0;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 lo = acc[r][u][0] | (u64)acc[r][u][1] << 32, hi = acc[r][u][2] | (u64)acc[r][u][3] << 32;
            if (lo | hi) {
                atomicMin(first, pos[u] + (lo ? (u32)__builtin_ctzll(lo) >> 3 : 8u + ((u32)__builtin_ctzll(hi) >> 3)));
                rows[r] = 0u;
            }
        }
}

// Byte tp of check row r of a chunk as predicted from its basis, XOR the stored byte: nonzero when
// they differ.  An entry's bytes past its avail read as zero.
__device__ __forceinline__ u32 check_byte(const u8 *__restrict__ blocks, const sec::ChkDesc &d,
                                          const u32 *__restrict__ tabs, const sec::ChkSlots sl, u32 r, u32 tp)
{
    auto entry_byte = [&](u32 e) -> u32 {
        return tp < sl.avail[d.slot0 + e] ? (u32)blocks[sl.off[d.slot0 + e] + tp] : 0u;
    };
    u32 acc = entry_byte(d.k + r);
    for (u32 c = 0; c < d.k; ++c)
        acc ^= gf_mul_byte(tabs + d.tab + (c * d.nr + r) * sec::kTabDwords, entry_byte(c));
    return acc;
}

// The chunk's ragged end [valid, B), byte by byte, for this tile's R check rows: the stored rows'
// bytes first, then every slot's byte loaded once, kBatch slots at a time (repair_ragged; a loop
// of dependent single-byte loads cost C4, 4 ragged positions per chunk, 2.3x the whole kernel).
template <int R>
__device__ __forceinline__ void check_ragged(const u8 *__restrict__ blocks, const sec::ChkDesc &d, const sec::Tile &tl,
                                             const u32 *__restrict__ tabs, const sec::ChkSlots sl)
{
    const u32 row0 = d.slot0 + d.k + tl.r0;
    for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x) {
        const u32 tp = d.valid + i;
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = tp < sl.avail[row0 + r] ? (u32)blocks[sl.off[row0 + r] + tp] : 0u;
        for (u32 c0 = 0; c0 < d.k; c0 += kBatch) {
            u32 x[kBatch];
            load_slot_bytes(x, blocks, sl, d.slot0, c0, d.k, tp);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                if (c0 + q < d.k)
                    gf_mac_bytes<R>(acc, tabs + d.tab, (c0 + q) * d.nr + tl.r0, x[q]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (acc[r])
                check_report(d, sl, tl.r0 + r, tp);
    }
}

// KBX > 0: slots per load batch fixed at KBX, as sec_repair_kernel's
template <int R, int U, bool W, int KBX = 0>
__global__ __launch_bounds__(sec::max_lanes(R, U)) void sec_check_kernel(const u8 *__restrict__ blocks,
                                                        const sec::ChkDesc *__restrict__ descs,
                                                        const sec::Tile *__restrict__ tiles,
                                                        const u32 *__restrict__ tabs,
                                                        const sec::ChkSlots sl)
{
    static_assert(R >= 1, "a check tile has check rows");
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::ChkDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t < d.valid)
        check_main<R, U, W, KBX>(blocks, d, tl, t, tabs, sl);
    if (tl.ntail)
        check_ragged<R>(blocks, d, tl, tabs, sl);
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16): every check
// row's byte there.
__global__ __launch_bounds__(256) void sec_check_tail(const u8 *__restrict__ blocks,
                                                      const sec::ChkDesc *__restrict__ descs,
                                                      const sec::TailItem *__restrict__ items, u32 nitems,
                                                      const u32 *__restrict__ tabs, const sec::ChkSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::ChkDesc d = descs[it.chunk];
    for (u32 r = 0; r < d.nr; ++r)
        if (check_byte(blocks, d, tabs, sl, r, it.t))
            check_report(d, sl, r, it.t);
}

// One thread per entry, after the kernels above: a check row's flag into row_bad (basis entries 0)
// and, for an inconsistent chunk, the entry's byte at the first differing position into column,
// both indexed in the caller's order; the chunk's first entry also turns the flag words into the
// chunk's result.  (One thread per chunk, looping over its entries, took a third of C4's time.)
__global__ __launch_bounds__(256) void sec_check_final(const u8 *__restrict__ blocks,
                                                       const sec::ChkDesc *__restrict__ descs, u32 nentries,
                                                       const sec::ChkSlots sl, sec::ChkResult *__restrict__ results,
                                                       u8 *__restrict__ row_bad, u8 *__restrict__ column)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nentries)
        return;
    const sec::ChkDesc d = descs[sl.echunk[i]];
    const u32 e = i - d.slot0;
    const u32 first = sl.flags[d.flag0];  // 0xFFFFFFFF: no row differs
    const u32 at = d.cslot0 + sl.cpos[i];
    if (row_bad)
        row_bad[at] = e >= d.k && sl.flags[d.flag0 + 1 + e - d.k] == 0u;
    if (column && first != ~0u)
        column[at] = first < sl.avail[i] ? blocks[sl.off[i] + first] : (u8)0;
    if (e == 0) {
        u32 nbad = 0;
        for (u32 r = 0; r < d.nr; ++r)
            nbad += sl.flags[d.flag0 + 1 + r] == 0u;
        results[d.res] = sec::ChkResult{nbad ? (u64)first : ~(u64)0, nbad, 0u};
    }
}

// ---- decode + check: reassemble from k held pieces and check the spare ones in one pass ----------
// A chunk's rows are one table over its k basis slots (the repair matrix, layout [slot][row][5]):
// rows 0 .. e-1 its missing primaries in ascending order, rows e .. e+nr-1 its check rows.  A tile
// (chunk, t0, r0) takes rows r0 .. r0+R-1 of them.  Those below `split` = e - r0 (clamped to
// [0, R], uniform over the workgroup) are STORE rows: zero-started accumulators stored to output
// row miss[...], as decode_main's.  The rest are COMPARE rows: the stored block is XORed in after
// the last slot, into registers the slots have left (check_main's kRowsLast form, for every R: a
// store row and a compare row then cost the same registers), and the OR epilogue and the report are
// check_main's, so a clean chunk's compare rows store nothing.  The row group r0 == 0 also copies
// the present primaries (row[] = 0xFFFFFFFF for every slot of a recover-only call).  Each unrolled
// r tests r < split, so the accumulators keep static register indices.
// Positions < valid = min(the last output row's length unless recover-only, every entry's avail)
// are the tiles'; [valid, B) goes byte by byte on the chunk's last tile of each row group
// (decode_ragged and check_ragged in one loop), an entry's bytes past its avail reading as zero.
// A sibling of decode_main and check_main, not a shared body.
__device__ __forceinline__ void dchk_report(const sec::DChkDesc &d, const sec::DChkSlots sl, u32 crow, u32 at)
{
    atomicMin(sl.flags + d.flag0, at);
    sl.flags[d.flag0 + 1 + crow] = 0u;
}

template <int R, int U, bool W, int KBX>
__device__ __forceinline__ void dchk_main(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                          const sec::DChkDesc &d, const sec::Tile &tl, u32 t,
                                          const u32 *__restrict__ tabs, const sec::DChkSlots sl)
{
    const u32 B = d.B, k = d.k;
    u32 pos[U];
    tile_pos(pos, t, d.valid);
    u8 *dst = out + d.out_off;
    const bool copies = tl.r0 == 0;  // row group 0 also copies the present primaries
    const u32 *tj = tabs + d.tab + tl.r0 * sec::kTabDwords;
    const u32 tstep = (d.e + d.nr) * sec::kTabDwords;
    const int split = d.e > tl.r0 ? (int)min(d.e - tl.r0, (u32)R) : 0;  // rows below it are stored

    u32x4 acc[R > 0 ? R : 1][U];
#pragma unroll
    for (int r = 0; r < (R > 0 ? R : 1); ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // slots in batches of KB: every load of a batch, its arithmetic, then the copies (decode_main)
    constexpr int KB = KBX > 0 ? KBX : batch_blocks<U, W, true>();
    auto batch = [&](u32 c0) {
        constexpr bool LT = lds_tab<R, true>();
        const u32x2 *vt = wave_tabs<KB, R, LT>(tj, tstep, c0, k);
        u64 so[KB];  // (the plan pads sl.off by kBatchVecs entries)
        const u64 *sop = sl.off + d.slot0 + c0;
#pragma unroll
        for (int c = 0; c < KB; ++c)
            so[c] = sop[c];
        u32x4 xs[KB][U];
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u8 *s = blocks + so[c];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    xs[c][u] = load16(s + pos[u]);
            }
        if constexpr (R > 0 && kPairRows<R, W>()) {
#pragma unroll
            for (int c = 0; c < KB; c += 2) {
                if (c + 1 < KB && c0 + c + 1 < k)
                    gf_mac2<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R, xs[c + 1],
                                      tj + (c0 + c + 1) * tstep, vt + (c + 1) * R);
                else if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
            }
        } else if constexpr (R > 0) {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
        }
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u32 orow = sl.row[d.slot0 + c0 + c];
                if (copies && orow != 0xFFFFFFFFu) {
                    u8 *o = dst + (u64)orow * B;
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        store16<SEC_DEC_ST>(o + pos[u], xs[c][u]);
                }
            }
    };
    if constexpr (W) {  // wide k: several batches (see encode_main)
#pragma unroll 1
        for (u32 c0 = 0; c0 < k; c0 += KB)
            batch(c0);
    } else {
        batch(0);  // the plan guarantees k <= KB here
    }
    if constexpr (R > 0) {
        // compare row r of the tile is check row r0 + r - e: entry k + that, flag word 1 + that
        const int crow0 = (int)tl.r0 - (int)d.e;
        const u64 *ro = sl.off + d.slot0 + k;
        // the stored rows into registers the slots have left: the empty asm makes the lane's position
        // wait for an accumulator as it stands here, so the loads cannot be hoisted above the
        // arithmetic, where they would spill (check_main)
#pragma unroll
        for (int u = 0; u < U; ++u)
            asm volatile("" : "+v"(pos[u]) : "v"(acc[R - 1][u][3]));
        // Nothing but memory effects leaves a branch on `split`: accumulators or stored rows defined
        // on one side of such a branch only (a load per compare row under its own test) became
        // whole-array copies at every join and spilled hundreds of VGPRs.  So the R loads are
        // unconditional wherever the tile has a compare row at all: store row r loads the tile's
        // first compare row again (the same 16 bytes of the same lane, issued back to back), and its
        // mask drops it from the OR.
        const bool compares = split < R;
        u32x4 st[R][U];
        if (compares) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const u8 *s = blocks + ro[crow0 + max(r, split)];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    st[r][u] = load16(s + pos[u]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < split) {
                u8 *o = dst + (u64)sl.miss[d.slot0 + tl.r0 + r] * B;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    store16<SEC_DEC_ST>(o + pos[u], acc[r][u]);
            }
        if (!compares)
            return;
        u32 any = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u32 cmp = r >= split ? ~0u : 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    acc[r][u][w] = (acc[r][u][w] ^ st[r][u][w]) & cmp;
                    any |= acc[r][u][w];
                }
            }
        }
        if (any == 0)
            return;
        u32 *first = sl.flags + d.flag0;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const u64 lo = acc[r][u][0] | (u64)acc[r][u][1] << 32, hi = acc[r][u][2] | (u64)acc[r][u][3] << 32;
                if (lo | hi) {  // (a store row's are zero)
                    atomicMin(first, pos[u] + (lo ? (u32)__builtin_ctzll(lo) >> 3 : 8u + ((u32)__builtin_ctzll(hi) >> 3)));
                    first[1 + crow0 + r] = 0u;
                }
            }
    }
}

// The chunk's ragged end [valid, B), byte by byte, for this tile's R rows: the compare rows' stored
// bytes first, then every slot's byte loaded once, kBatch slots at a time, feeding the copy (row
// group 0) and all R rows; stores only where the output row still has bytes.
template <int R>
__device__ __forceinline__ void dchk_ragged(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                            const sec::DChkDesc &d, const sec::Tile &tl,
                                            const u32 *__restrict__ tabs, const sec::DChkSlots sl)
{
    const int split = d.e > tl.r0 ? (int)min(d.e - tl.r0, (u32)R) : 0;
    const int crow0 = (int)tl.r0 - (int)d.e;
    const u32 ent0 = d.slot0 + d.k;  // the chunk's first check row entry
    const u32 nrows = d.e + d.nr;
    for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x) {
        const u32 tp = d.valid + i;
        u8 *dst = out + d.out_off + tp;
        u32 acc[R > 0 ? R : 1];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = (r >= split && tp < sl.avail[ent0 + crow0 + r]) ? (u32)blocks[sl.off[ent0 + crow0 + r] + tp] : 0u;
        for (u32 c0 = 0; c0 < d.k; c0 += kBatch) {
            u32 x[kBatch];
            load_slot_bytes(x, blocks, sl, d.slot0, c0, d.k, tp);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                if (c0 + q < d.k) {
                    const u32 c = c0 + q;
                    const u32 orow = sl.row[d.slot0 + c];
                    if (tl.r0 == 0 && orow != 0xFFFFFFFFu && (u64)orow * d.B + tp < d.n)
                        dst[(u64)orow * d.B] = (u8)x[q];
                    gf_mac_bytes<R>(acc, tabs + d.tab, c * nrows + tl.r0, x[q]);
                }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < split) {
                const u32 orow = sl.miss[d.slot0 + tl.r0 + r];
                if ((u64)orow * d.B + tp < d.n)
                    dst[(u64)orow * d.B] = (u8)acc[r];
            } else if (acc[r]) {
                dchk_report(d, sl, (u32)(crow0 + r), tp);
            }
        }
    }
}

// R = 0: a chunk with every primary held and no check row, copies only.  KBX > 0: slots per load
// batch fixed at KBX, as sec_decode_kernel's
template <int R, int U, bool W, int KBX = 0>
__global__ __launch_bounds__(sec::max_lanes(R, U)) void sec_decode_check_kernel(const u8 *__restrict__ blocks,
                                                               u8 *__restrict__ out,
                                                               const sec::DChkDesc *__restrict__ descs,
                                                               const sec::Tile *__restrict__ tiles,
                                                               const u32 *__restrict__ tabs,
                                                               const sec::DChkSlots sl)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::DChkDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t < d.valid)
        dchk_main<R, U, W, KBX>(blocks, out, d, tl, t, tabs, sl);
    if (tl.ntail)
        dchk_ragged<R>(blocks, out, d, tl, tabs, sl);
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16): the copies,
// every recovered row's byte and every check row's byte there.
__global__ __launch_bounds__(256) void sec_decode_check_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                             const sec::DChkDesc *__restrict__ descs,
                                                             const sec::TailItem *__restrict__ items, u32 nitems,
                                                             const u32 *__restrict__ tabs, const sec::DChkSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::DChkDesc d = descs[it.chunk];
    u8 *dst = out + d.out_off + it.t;
    auto entry_byte = [&](u32 c) -> u32 {  // bytes past the entry's avail read as zero
        return it.t < sl.avail[d.slot0 + c] ? (u32)blocks[sl.off[d.slot0 + c] + it.t] : 0u;
    };
    for (u32 c = 0; c < d.k; ++c) {
        const u32 orow = sl.row[d.slot0 + c];
        if (orow != 0xFFFFFFFFu && (u64)orow * d.B + it.t < d.n)
            dst[(u64)orow * d.B] = (u8)entry_byte(c);
    }
    const u32 nrows = d.e + d.nr;
    for (u32 r = 0; r < nrows; ++r) {
        if (r < d.e && (u64)sl.miss[d.slot0 + r] * d.B + it.t >= d.n)
            continue;
        u32 acc = r < d.e ? 0u : entry_byte(d.k + r - d.e);
        for (u32 c = 0; c < d.k; ++c)
            acc ^= gf_mul_byte(tabs + d.tab + (c * nrows + r) * sec::kTabDwords, entry_byte(c));
        if (r < d.e)
            dst[(u64)sl.miss[d.slot0 + r] * d.B] = (u8)acc;
        else if (acc)
            dchk_report(d, sl, r - d.e, it.t);
    }
}

// ---- repair + check: regenerate lost pieces and check the spare ones in one pass -----------------
// A chunk's rows are one table over its k basis slots (the repair matrix, layout [slot][row][5]):
// rows 0 .. nt-1 its targets in the caller's order, rows nt .. nt+nr-1 its check rows in entry
// order.  A tile (chunk, t0, r0) takes rows r0 .. r0+R-1 of them.  Those below `split` = nt - r0
// (clamped to [0, R], uniform over the workgroup) are STORE rows: zero-started accumulators stored
// whole with unaligned 16 B stores at the row's own address out + tgt_off[tgt0 + r0 + r], as
// repair_main's.  The rest are COMPARE rows, exactly dchk_main's: the stored block is XORed in after
// the last slot, into registers the slots have left, and the OR epilogue and the report are
// check_main's, so a clean chunk's compare rows store nothing.  What decode + check has and this
// has not: copies of present primaries (no row[] array, no branch on r0 == 0), an output row index
// (miss[]) and a chunk length to truncate against; every target is a whole B-byte piece.  Each
// unrolled r tests r < split, so the accumulators keep static register indices, and the target's
// address is fetched under the store's own test: nothing but memory effects leaves a branch on
// `split` (see dchk_main).
// Positions < valid = min(B, every one of the n entries' avail) are the tiles'; [valid, B) goes byte
// by byte on the chunk's last tile of each row group (repair_ragged and check_ragged in one loop),
// an entry's bytes past its avail reading as zero and every target byte up to B stored.
// A sibling of repair_main and dchk_main, not a shared body.
__device__ __forceinline__ void rchk_report(const sec::RChkDesc &d, const sec::RChkSlots sl, u32 crow, u32 at)
{
    atomicMin(sl.flags + d.flag0, at);
    sl.flags[d.flag0 + 1 + crow] = 0u;
}

template <int R, int U, bool W, int KBX>
__device__ __forceinline__ void rchk_main(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                          const sec::RChkDesc &d, const sec::Tile &tl, u32 t,
                                          const u32 *__restrict__ tabs, const sec::RChkSlots sl)
{
    const u32 k = d.k;
    u32 pos[U];
    tile_pos(pos, t, d.valid);
    const u32 *tj = tabs + d.tab + tl.r0 * sec::kTabDwords;
    const u32 tstep = (d.nt + d.nr) * sec::kTabDwords;
    const int split = d.nt > tl.r0 ? (int)min(d.nt - tl.r0, (u32)R) : 0;  // rows below it are stored

    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // slots in batches of KB, every load of a batch before its arithmetic (repair_main)
    constexpr int KB = KBX > 0 ? KBX : batch_blocks<U, W, true>();
    auto batch = [&](u32 c0) {
        constexpr bool LT = lds_tab<R, true>();
        const u32x2 *vt = wave_tabs<KB, R, LT>(tj, tstep, c0, k);
        u64 so[KB];  // (the plan pads sl.off by kBatchVecs entries)
        const u64 *sop = sl.off + d.slot0 + c0;
#pragma unroll
        for (int c = 0; c < KB; ++c)
            so[c] = sop[c];
        u32x4 xs[KB][U];
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c0 + c < k) {
                const u8 *s = blocks + so[c];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    xs[c][u] = load16(s + pos[u]);
            }
        if constexpr (kPairRows<R, W>()) {
#pragma unroll
            for (int c = 0; c < KB; c += 2) {
                if (c + 1 < KB && c0 + c + 1 < k)
                    gf_mac2<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R, xs[c + 1],
                                      tj + (c0 + c + 1) * tstep, vt + (c + 1) * R);
                else if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
            }
        } else {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c0 + c < k)
                    gf_mac<R, U, LT>(acc, xs[c], tj + (c0 + c) * tstep, vt + c * R);
        }
    };
    if constexpr (W) {  // wide k: several batches (see encode_main)
#pragma unroll 1
        for (u32 c0 = 0; c0 < k; c0 += KB)
            batch(c0);
    } else {
        batch(0);  // the plan guarantees k <= KB here
    }
    // compare row r of the tile is check row r0 + r - nt: entry k + that, flag word 1 + that
    const int crow0 = (int)tl.r0 - (int)d.nt;
    const u64 *ro = sl.off + d.slot0 + k;
    // the stored rows into registers the slots have left: the empty asm makes the lane's position
    // wait for an accumulator as it stands here, so the loads cannot be hoisted above the
    // arithmetic, where they would spill (check_main)
#pragma unroll
    for (int u = 0; u < U; ++u)
        asm volatile("" : "+v"(pos[u]) : "v"(acc[R - 1][u][3]));
    // The R loads are unconditional wherever the tile has a compare row at all (dchk_main): store
    // row r loads the tile's first compare row again, and its mask drops it from the OR.
    const bool compares = split < R;
    u32x4 st[R][U];
    if (compares) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u8 *s = blocks + ro[crow0 + max(r, split)];
#pragma unroll
            for (int u = 0; u < U; ++u)
                st[r][u] = load16(s + pos[u]);
        }
    }
    const u64 *to = sl.tgt_off + d.tgt0 + tl.r0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r < split) {
            u8 *o = out + to[r];
#pragma unroll
            for (int u = 0; u < U; ++u)
                store16<SEC_DEC_ST>(o + pos[u], acc[r][u]);
        }
    if (!compares)
        return;
    u32 any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32 cmp = r >= split ? ~0u : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                acc[r][u][w] = (acc[r][u][w] ^ st[r][u][w]) & cmp;
                any |= acc[r][u][w];
            }
        }
    }
    if (any == 0)
        return;
    u32 *first = sl.flags + d.flag0;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 lo = acc[r][u][0] | (u64)acc[r][u][1] << 32, hi = acc[r][u][2] | (u64)acc[r][u][3] << 32;
            if (lo | hi) {  // (a store row's are zero)
                atomicMin(first, pos[u] + (lo ? (u32)__builtin_ctzll(lo) >> 3 : 8u + ((u32)__builtin_ctzll(hi) >> 3)));
                first[1 + crow0 + r] = 0u;
            }
        }
}

// The chunk's ragged end [valid, B), byte by byte, for this tile's R rows: the compare rows' stored
// bytes first (zero past the row's avail), then every slot's byte loaded once, kBatch slots at a
// time, feeding all R rows; every store row's byte is stored, up to B.
template <int R>
__device__ __forceinline__ void rchk_ragged(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                            const sec::RChkDesc &d, const sec::Tile &tl,
                                            const u32 *__restrict__ tabs, const sec::RChkSlots sl)
{
    const int split = d.nt > tl.r0 ? (int)min(d.nt - tl.r0, (u32)R) : 0;
    const int crow0 = (int)tl.r0 - (int)d.nt;
    const u32 ent0 = d.slot0 + d.k;  // the chunk's first check row entry
    const u32 nrows = d.nt + d.nr;
    const u64 *to = sl.tgt_off + d.tgt0 + tl.r0;
    for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x) {
        const u32 tp = d.valid + i;
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = (r >= split && tp < sl.avail[ent0 + crow0 + r]) ? (u32)blocks[sl.off[ent0 + crow0 + r] + tp] : 0u;
        for (u32 c0 = 0; c0 < d.k; c0 += kBatch) {
            u32 x[kBatch];
            load_slot_bytes(x, blocks, sl, d.slot0, c0, d.k, tp);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                if (c0 + q < d.k)
                    gf_mac_bytes<R>(acc, tabs + d.tab, (c0 + q) * nrows + tl.r0, x[q]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < split)
                out[to[r] + tp] = (u8)acc[r];
            else if (acc[r])
                rchk_report(d, sl, (u32)(crow0 + r), tp);
        }
    }
}

// KBX > 0: slots per load batch fixed at KBX, as sec_repair_kernel's.  (No R = 0: a chunk with
// neither a target nor a check row launches nothing.)
template <int R, int U, bool W, int KBX = 0>
__global__ __launch_bounds__(sec::max_lanes(R, U)) void sec_repair_check_kernel(const u8 *__restrict__ blocks,
                                                               u8 *__restrict__ out,
                                                               const sec::RChkDesc *__restrict__ descs,
                                                               const sec::Tile *__restrict__ tiles,
                                                               const u32 *__restrict__ tabs,
                                                               const sec::RChkSlots sl)
{
    static_assert(R >= 1, "a repair + check tile has target or check rows: nothing is copied");
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::RChkDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t < d.valid)
        rchk_main<R, U, W, KBX>(blocks, out, d, tl, t, tabs, sl);
    if (tl.ntail)
        rchk_ragged<R>(blocks, out, d, tl, tabs, sl);
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16): every target
// row's byte and every check row's byte there.
__global__ __launch_bounds__(256) void sec_repair_check_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                             const sec::RChkDesc *__restrict__ descs,
                                                             const sec::TailItem *__restrict__ items, u32 nitems,
                                                             const u32 *__restrict__ tabs, const sec::RChkSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::RChkDesc d = descs[it.chunk];
    auto entry_byte = [&](u32 c) -> u32 {  // bytes past the entry's avail read as zero
        return it.t < sl.avail[d.slot0 + c] ? (u32)blocks[sl.off[d.slot0 + c] + it.t] : 0u;
    };
    const u32 nrows = d.nt + d.nr;
    for (u32 r = 0; r < nrows; ++r) {
        u32 acc = r < d.nt ? 0u : entry_byte(d.k + r - d.nt);
        for (u32 c = 0; c < d.k; ++c)
            acc ^= gf_mul_byte(tabs + d.tab + (c * nrows + r) * sec::kTabDwords, entry_byte(c));
        if (r < d.nt)
            out[sl.tgt_off[d.tgt0 + r] + it.t] = (u8)acc;
        else if (acc)
            rchk_report(d, sl, r - d.nt, it.t);
    }
}

// ---- decode + correct: reassemble, and put right one wrong entry per byte position -------------
// The chunk's table is decode + check's (rows 0 .. e-1 the missing primaries, rows e .. e+nr-1 the
// check rows, over the k basis slots).  At every position the n held bytes are a column, and the
// kernel does to it what sec_check_locate (gf_host.hpp check_locate) says of it: a code word is
// decoded as it is; one differing check row is that row's own error (the output is unaffected);
// all nr differing with d_j = R[j][s] * v for one basis slot s means slot s is wrong by v, and the
// output is the decode of the basis with that byte put right; anything else is open and decoded as
// held.  A sibling of dchk_main, not a change to it (DESIGN §5 "Corrected decode").
//
// Two levels.  A tile is (chunk, t0) and takes ALL rows of its positions, in groups of R rows
// (a position's verdict needs every check row, and the fix every stored row).  A lane with 16
// whole positions below `valid` first forms the check deltas of every group with the v_perm
// products and ORs them (cor_rows: 8-slot load batches, coalesced entry by entry); with the OR zero
// it has located nothing and goes on to store the recovered rows and copy the present primaries, a
// plain decode.  Only a lane whose OR is nonzero takes its 16 positions byte by byte (cor_pos),
// and stores nothing as a vector: no output byte is written twice, so no store has to be ordered
// after another.  The lane that straddles `valid`, the ragged end [valid, B) and the chunks too
// small for a tile go byte by byte as well.
//
// cor_byte keeps nothing per row or per slot beyond one group of R rows and one batch of 16 slot
// bytes (nr reaches 32, k 64: no dynamically indexed array, no scratch): the deltas are formed
// group by group, counted, and rows 0 and 1 kept.  The slot search needs no division:
// d_0 = R[0][s] v and d_1 = R[1][s] v  <=>  R[1][s] d_0 = R[0][s] d_1 (R[0][s] != 0), two products
// by constants the table already has, and at most one s passes since every 2 x 2 minor of the
// matrix is nonzero.  v = d_0 / R[0][s] through the exp/log tables (R[0][s] is byte 1 of the
// table's first dword), and rows 2 .. nr-1 are formed again to confirm.
//
// Counters are ordinary vector atomics on the call's words (CorDesc::flag0 / cnt0), summed over
// the wave's active lanes first: a wholly corrupt piece makes every position hit the same words.
struct CorVerdict {
    int hit;    // the entry (kernel order: basis slots, then check rows) that was changed, or -1
    bool bad;   // the column is no code word
    bool open;  // ... and no single-entry change explains it
};

__device__ __forceinline__ u32 cor_lane()
{
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// *w += the number of active lanes with pred
__device__ __forceinline__ void wave_count(u32 *w, bool pred)
{
    const u64 m = __ballot(pred);
    if (pred && cor_lane() == (u32)__builtin_ctzll(m))
        atomicAdd(w, (u32)__builtin_popcountll(m));
}

__device__ __forceinline__ void min_word(u32 *w, u32 v)
{
    if (*(volatile u32 *)w > v)
        atomicMin(w, v);
}

// WAVE: every lane of the wave is on the same chunk (the tile kernel), so their counts go through
// one atomic per word; else (the tail kernel: a lane per item of any chunk) each lane adds its own.
template <bool WAVE, class Slots>
__device__ __forceinline__ void cor_tally(const sec::CorDesc &d, const Slots sl, u32 p, const CorVerdict v)
{
    u32 *f = sl.flags + d.flag0, *c = sl.flags + d.cnt0;
    if (v.bad)
        min_word(f, p);
    if (v.open)
        min_word(f + 1, p);
    if constexpr (!WAVE) {
        if (v.hit >= 0) {
            atomicAdd(c, 1u);
            atomicAdd(c + 2 + v.hit, 1u);
        }
        if (v.open)
            atomicAdd(c + 1, 1u);
        return;
    }
    wave_count(c, v.hit >= 0);
    wave_count(c + 1, v.open);
    // one atomic per distinct entry among the wave's active lanes
    // (the loop is wave-uniform: `rem` is a ballot, so no lane leaves it ahead of another)
    u64 rem = __ballot(v.hit >= 0);
    while (rem) {
        const u32 lead = (u32)__builtin_ctzll(rem);
        const int h = __builtin_amdgcn_readlane(v.hit, (int)lead);
        const u64 m = __ballot(v.hit == h);
        if (cor_lane() == lead)
            atomicAdd(c + 2 + h, (u32)__builtin_popcountll(m));
        rem &= ~m;
    }
}

// Position p of a chunk, whole, in two parts both correcting operations share the first of: the
// verdict on its column (cor_judge) and every output byte there (cor_byte: the decode's; rcor_byte:
// the repair's targets).  Rows go in groups of R and the slots' bytes in batches of kBatch loads
// issued together (repair_ragged: a loop of dependent single-byte loads costs one memory latency per
// slot and row).
struct CorFix {
    CorVerdict v;
    u32 fix, val;  // the basis slot put right (~0u: none), by which value
};

// acc[r] ^= XOR_c T[c][min(row0 + r, rlast)] * (slot c's byte at p, slot `fix` changed by `val`)
template <int R, class Slots>
__device__ __forceinline__ void cor_byte_rows(u32 (&acc)[R], const u8 *__restrict__ blocks, const sec::CorDesc &d,
                                              const u32 *__restrict__ tabs, const Slots sl, u32 p, u32 row0,
                                              u32 rlast, u32 fix, u32 val)
{
    const u32 k = d.k, nrows = d.e + d.nr;
    for (u32 c0 = 0; c0 < k; c0 += kBatch) {
        u32 x[kBatch];
        load_slot_bytes(x, blocks, sl, d.slot0, c0, k, p);
#pragma unroll
        for (u32 q = 0; q < kBatch; ++q)
            if (c0 + q < k) {
                const u32 xv = x[q] ^ (c0 + q == fix ? val : 0u);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    acc[r] ^= gf_mul_byte(
                        tabs + d.tab + ((c0 + q) * nrows + min(row0 + (u32)r, rlast)) * sec::kTabDwords, xv);
            }
    }
}

template <int R, class Slots>
__device__ __forceinline__ CorFix cor_judge(const u8 *__restrict__ blocks, const sec::CorDesc &d,
                                            const u32 *__restrict__ tabs, const Slots sl, u32 p)
{
    const u32 k = d.k, e = d.e, nr = d.nr, nrows = e + nr;
    auto tab = [&](u32 c, u32 r) { return tabs + d.tab + (c * nrows + r) * sec::kTabDwords; };
    auto rows = [&](u32 (&acc)[R], u32 row0, u32 rlast, u32 fix, u32 val) {
        cor_byte_rows<R>(acc, blocks, d, tabs, sl, p, row0, rlast, fix, val);
    };
    // the deltas of check rows g0 .. g0 + R - 1 (those past nr - 1 repeat row nr - 1)
    auto deltas = [&](u32 (&acc)[R], u32 g0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u32 ent = d.slot0 + k + min(g0 + (u32)r, nr - 1);
            acc[r] = p < sl.avail[ent] ? (u32)blocks[sl.off[ent] + p] : 0u;
        }
        rows(acc, e + g0, nrows - 1, ~0u, 0u);
    };
    u32 cnt = 0, last = 0, d0 = 0, d1 = 0;
    for (u32 g0 = 0; g0 < nr; g0 += R) {
        u32 acc[R];
        deltas(acc, g0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u32 j = g0 + r;
            if (j < nr && acc[r]) {
                ++cnt;
                last = j;
            }
            d0 = j == 0 ? acc[r] : d0;
            d1 = j == 1 ? acc[r] : d1;
        }
    }
    CorVerdict v{-1, cnt != 0, false};
    u32 fix = ~0u, val = 0;  // basis slot put right, by which value
    if (cnt == 0) {
    } else if (nr < 2) {
        v.open = true;
    } else if (cnt == 1) {
        v.hit = (int)(k + last);
    } else if (cnt == nr) {
        u32 s = 0;
        for (; s < k; ++s) {
            const u32 r0 = (tab(s, e)[0] >> 8) & 0xFFu;  // R[0][s]
            if (r0 && gf_mul_byte(tab(s, e + 1), d0) == gf_mul_byte(tab(s, e), d1)) {
                val = c_gf.exp[(u32)c_gf.log[d0] + 255u - (u32)c_gf.log[r0]];
                break;
            }
        }
        bool ok = s < k;
        for (u32 g0 = 0; ok && nr > 2 && g0 < nr; g0 += R) {  // rows 2 .. nr - 1 confirm the slot
            u32 acc[R];
            deltas(acc, g0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const u32 j = g0 + r;
                if (j >= 2 && j < nr && gf_mul_byte(tab(s, e + j), val) != acc[r])
                    ok = false;
            }
        }
        if (ok) {
            fix = s;
            v.hit = (int)s;
        } else {
            v.open = true;
        }
    } else {
        v.open = true;
    }
    return {v, fix, val};
}

// The decode's output part: the present primaries' bytes and the recovered rows', from the basis
// column with slot `fix` changed by `val`, up to the chunk's length
template <int R>
__device__ __forceinline__ CorVerdict cor_byte(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                               const sec::CorDesc &d, const u32 *__restrict__ tabs,
                                               const sec::CorSlots sl, u32 p)
{
    const CorFix f = cor_judge<R>(blocks, d, tabs, sl, p);
    const u32 k = d.k, e = d.e, fix = f.fix, val = f.val;
    u8 *dst = out + d.out_off + p;
    for (u32 c0 = 0; c0 < k; c0 += kBatch) {
        u32 x[kBatch];
        load_slot_bytes(x, blocks, sl, d.slot0, c0, k, p);
#pragma unroll
        for (u32 q = 0; q < kBatch; ++q)
            if (c0 + q < k) {
                const u32 orow = sl.row[d.slot0 + c0 + q];
                if (orow != 0xFFFFFFFFu && (u64)orow * d.B + p < d.n)
                    dst[(u64)orow * d.B] = (u8)(x[q] ^ (c0 + q == fix ? val : 0u));
            }
    }
    for (u32 g0 = 0; g0 < e; g0 += R) {
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0u;
        cor_byte_rows<R>(acc, blocks, d, tabs, sl, p, g0, e - 1, fix, val);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < e) {
                const u32 orow = sl.miss[d.slot0 + g0 + r];
                if ((u64)orow * d.B + p < d.n)
                    dst[(u64)orow * d.B] = (u8)acc[r];
            }
    }
    return f.v;
}

// The repair's output part: every target's byte, (its row of the table) . (the basis column with
// slot `fix` changed by `val`), at the target's own address.  A held target goes through the table
// like a lost one: a basis entry's row is the unit row, a check row's its own row once more.
template <int R>
__device__ __forceinline__ CorVerdict rcor_byte(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                const sec::CorDesc &d, const u32 *__restrict__ tabs,
                                                const sec::RCorSlots sl, u32 p)
{
    const CorFix f = cor_judge<R>(blocks, d, tabs, sl, p);
    const u32 nt = d.e;
    for (u32 g0 = 0; g0 < nt; g0 += R) {
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0u;
        cor_byte_rows<R>(acc, blocks, d, tabs, sl, p, g0, nt - 1, f.fix, f.val);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < nt)
                out[sl.tgt_off[d.tgt0 + g0 + r] + p] = (u8)acc[r];
    }
    return f.v;
}

// Which judge the byte level runs: cor_judge (one error), or corx_judge with the call's bound
struct CorOne {};
struct CorMany {
    u32 tmax;  // min(max_errors, 16), 16 for max_errors == 0; a chunk's t = min(tmax, nr / 2)
};

template <int R, bool WAVE = true>
__device__ __forceinline__ void cor_pos(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                        const u32 *__restrict__ tabs, const sec::CorSlots sl, u32 p, CorOne = {})
{
    cor_tally<WAVE>(d, sl, p, cor_byte<R>(blocks, out, d, tabs, sl, p));
}

template <int R, bool WAVE = true>
__device__ __forceinline__ void cor_pos(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                        const u32 *__restrict__ tabs, const sec::RCorSlots sl, u32 p, CorOne = {})
{
    cor_tally<WAVE>(d, sl, p, rcor_byte<R>(blocks, out, d, tabs, sl, p));
}

// ---- the byte level with several errors per position (sec_*_correct_ex_kernel) -----------------
// The judge is a bounded-distance Reed-Solomon decoder on one column, gf_host.hpp check_correct step
// for step (the reasoning is there): syndromes from the check deltas, Berlekamp-Massey, the roots of
// the reversed connection polynomial among the n held points (piece 0's point, 0, is a root like any
// other there), the error values by synthetic division, and the check rows once more on the changed
// column, which makes the verdict exact.  The chunk's table carries, behind its k * (e + nr) row
// coefficients, 3n more in entry order (basis slots, then check rows): x_j, u_j and 1 / u_j, each
// expanded like a coefficient, so every product by one of them is gf_mul_byte (the judge needs them
// in no other way).  Products of two variables go through c_gf.
//
// State per position: 32 syndromes, two polynomials of 17 coefficients and 16 (entry, value) fixes,
// all indexed at run time, so they live in LDS, byte i of lane l at i * 256 + l (four lanes to a
// dword, no two lanes on one bank's different dwords).  The fixes' entries take the place of
// Berlekamp-Massey's second polynomial, which is dead once the locator stands: 82 bytes per lane,
// 20.5 KiB per workgroup, so seven workgroups fit a CU's 160 KiB as seven waves per SIMD do the
// registers of the R = 2 kernels.  Every loop is bounded by a constant or a chunk field: 2t
// Berlekamp-Massey steps, n root evaluations of L <= 16 Horner steps, nr rows to verify.  A miscount
// gives a wrong verdict, which the verification turns into open.
constexpr u32 kCxT = 16;  // sec::kMaxErrors (gf_host.hpp)
constexpr u32 kCxS = 0, kCxC = 2 * kCxT, kCxB = kCxC + kCxT + 1, kCxSlot = kCxB, kCxVal = kCxB + kCxT + 1,
              kCxBytes = kCxVal + kCxT;

struct CxState {
    u8 *p;
    __device__ __forceinline__ u8 &at(u32 i) const { return p[i * 256u]; }
    __device__ __forceinline__ u8 &S(u32 i) const { return at(kCxS + i); }
    __device__ __forceinline__ u8 &C(u32 i) const { return at(kCxC + i); }
    __device__ __forceinline__ u8 &B(u32 i) const { return at(kCxB + i); }
    __device__ __forceinline__ u8 &slot(u32 i) const { return at(kCxSlot + i); }
    __device__ __forceinline__ u8 &val(u32 i) const { return at(kCxVal + i); }
};

// The calling lane's slice (kernels of 256 lanes)
__device__ __forceinline__ CxState cx_state()
{
    __shared__ u8 s_cx[kCxBytes * 256u];
    return {s_cx + threadIdx.x};
}

__device__ __forceinline__ u32 gf_mul2(u32 a, u32 b)
{
    return a && b ? (u32)c_gf.exp[(u32)c_gf.log[a] + (u32)c_gf.log[b]] : 0u;
}

__device__ __forceinline__ u32 gf_div2(u32 a, u32 b)  // b != 0
{
    return a ? (u32)c_gf.exp[(u32)c_gf.log[a] + 255u - (u32)c_gf.log[b]] : 0u;
}

struct CxVerdict {
    bool bad, open;
    u32 nfix;  // entries changed: st.slot(f) (kernel order), st.val(f), f < nfix
};

// cor_byte_rows with the first nfix fixes of st applied to the basis bytes
template <int R, class Slots>
__device__ __forceinline__ void corx_byte_rows(u32 (&acc)[R], const u8 *__restrict__ blocks, const sec::CorDesc &d,
                                               const u32 *__restrict__ tabs, const Slots sl, u32 p, u32 row0,
                                               u32 rlast, const CxState st, u32 nfix)
{
    const u32 k = d.k, nrows = d.e + d.nr;
    for (u32 c0 = 0; c0 < k; c0 += kBatch) {
        u32 x[kBatch];
        load_slot_bytes(x, blocks, sl, d.slot0, c0, k, p);
        for (u32 f = 0; f < nfix; ++f) {
            const u32 s = st.slot(f), v = st.val(f);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                x[q] ^= s == c0 + q ? v : 0u;
        }
#pragma unroll
        for (u32 q = 0; q < kBatch; ++q)
            if (c0 + q < k) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    acc[r] ^= gf_mul_byte(
                        tabs + d.tab + ((c0 + q) * nrows + min(row0 + (u32)r, rlast)) * sec::kTabDwords, x[q]);
            }
    }
}

template <int R, class Slots>
__device__ __forceinline__ CxVerdict corx_judge(const u8 *__restrict__ blocks, const sec::CorDesc &d,
                                                const u32 *__restrict__ tabs, const Slots sl, u32 p, u32 tmax,
                                                const CxState st)
{
    const u32 k = d.k, e = d.e, nr = d.nr, nrows = e + nr, n = k + nr;
    const u32 t = min(min(tmax, nr / 2), kCxT);
    const u32 *xt = tabs + d.tab + k * nrows * sec::kTabDwords;  // read only when t > 0: the chunk then has a table
    auto xtab = [&](u32 j) { return xt + j * sec::kTabDwords; };
    auto utab = [&](u32 j) { return xt + (n + j) * sec::kTabDwords; };
    auto vtab = [&](u32 j) { return xt + (2 * n + j) * sec::kTabDwords; };
    // the deltas of check rows g0 .. g0 + R - 1 (those past nr - 1 repeat row nr - 1) of the column with the
    // first nfix fixes applied
    auto deltas = [&](u32 (&acc)[R], u32 g0, u32 nfix) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u32 ent = d.slot0 + k + min(g0 + (u32)r, nr - 1);
            acc[r] = p < sl.avail[ent] ? (u32)blocks[sl.off[ent] + p] : 0u;
        }
        for (u32 f = 0; f < nfix; ++f) {
            const u32 s = st.slot(f), v = st.val(f);
#pragma unroll
            for (int r = 0; r < R; ++r)
                acc[r] ^= s == k + min(g0 + (u32)r, nr - 1) ? v : 0u;
        }
        corx_byte_rows<R>(acc, blocks, d, tabs, sl, p, e + g0, nrows - 1, st, nfix);
    };
    for (u32 l = 0; l < 2 * t; ++l)
        st.S(l) = 0;
    bool bad = false;
    for (u32 g0 = 0; g0 < nr; g0 += R) {
        u32 acc[R];
        deltas(acc, g0, 0u);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const u32 j = g0 + r;
            if (j < nr && acc[r]) {
                bad = true;
                if (t) {  // S_l ^= u_j x_j^l d_j
                    u32 term = gf_mul_byte(utab(k + j), acc[r]);
                    for (u32 l = 0; l < 2 * t; ++l) {
                        st.S(l) ^= (u8)term;
                        term = gf_mul_byte(xtab(k + j), term);
                    }
                }
            }
        }
    }
    if (!bad)
        return {false, false, 0u};
    if (t == 0)
        return {true, true, 0u};
    // Berlekamp-Massey, 2t steps: S_i = sum_{q = 1 .. L} C_q S_{i - q}
    for (u32 q = 0; q <= kCxT; ++q)
        st.C(q) = st.B(q) = q == 0;
    u32 L = 0, sh = 1, b = 1;
    for (u32 i = 0; i < 2 * t; ++i) {
        u32 dd = st.S(i);
        const u32 qn = min(min(L, i), kCxT);
        for (u32 q = 1; q <= qn; ++q)
            dd ^= gf_mul2(st.C(q), st.S(i - q));
        if (dd == 0) {
            ++sh;
            continue;
        }
        const u32 f = gf_div2(dd, b);
        const bool grow = 2 * L <= i;
        for (int q = (int)kCxT; q >= 0; --q) {  // C += f z^sh B, and B = the old C where L grows, in place
            const u32 c = st.C(q);
            if ((u32)q >= sh)
                st.C(q) = (u8)(c ^ gf_mul2(f, st.B((u32)q - sh)));
            if (grow)
                st.B(q) = (u8)c;
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
        return {true, true, 0u};
    // the roots of R(z) = sum_q C_q z^(L - q) among the held points
    u32 nloc = 0;
    for (u32 j = 0; j < n; ++j) {
        u32 v = 0;
        for (u32 q = 0; q <= L; ++q)
            v = gf_mul_byte(xtab(j), v) ^ st.C(q);
        if (v == 0) {
            if (nloc < L)
                st.slot(nloc) = (u8)j;
            ++nloc;
        }
    }
    if (nloc != L)
        return {true, true, 0u};
    bool ok = true;
    for (u32 a = 0; a < L; ++a) {
        const u32 j = st.slot(a);
        u32 q = 0, num = 0, den = 0;
        for (int l = (int)L - 1; l >= 0; --l) {
            q = st.C(L - 1 - (u32)l) ^ gf_mul_byte(xtab(j), q);
            num ^= gf_mul2(q, st.S((u32)l));
            den = gf_mul_byte(xtab(j), den) ^ q;
        }
        const u32 ev = den ? gf_mul_byte(vtab(j), gf_div2(num, den)) : 0u;
        ok = ok && ev != 0;
        st.val(a) = (u8)ev;
    }
    for (u32 g0 = 0; ok && g0 < nr; g0 += R) {  // the check rows once more, on the changed column
        u32 acc[R];
        deltas(acc, g0, L);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < nr && acc[r])
                ok = false;
    }
    return ok ? CxVerdict{true, false, L} : CxVerdict{true, true, 0u};
}

// The decode's output part (cor_byte's) from the basis column with nfix fixes applied
template <int R>
__device__ __forceinline__ void corx_store(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                           const u32 *__restrict__ tabs, const sec::CorSlots sl, u32 p,
                                           const CxState st, u32 nfix)
{
    const u32 k = d.k, e = d.e;
    u8 *dst = out + d.out_off + p;
    for (u32 c0 = 0; c0 < k; c0 += kBatch) {
        u32 x[kBatch];
        load_slot_bytes(x, blocks, sl, d.slot0, c0, k, p);
        for (u32 f = 0; f < nfix; ++f) {
            const u32 s = st.slot(f), v = st.val(f);
#pragma unroll
            for (u32 q = 0; q < kBatch; ++q)
                x[q] ^= s == c0 + q ? v : 0u;
        }
#pragma unroll
        for (u32 q = 0; q < kBatch; ++q)
            if (c0 + q < k) {
                const u32 orow = sl.row[d.slot0 + c0 + q];
                if (orow != 0xFFFFFFFFu && (u64)orow * d.B + p < d.n)
                    dst[(u64)orow * d.B] = (u8)x[q];
            }
    }
    for (u32 g0 = 0; g0 < e; g0 += R) {
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0u;
        corx_byte_rows<R>(acc, blocks, d, tabs, sl, p, g0, e - 1, st, nfix);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < e) {
                const u32 orow = sl.miss[d.slot0 + g0 + r];
                if ((u64)orow * d.B + p < d.n)
                    dst[(u64)orow * d.B] = (u8)acc[r];
            }
    }
}

// The repair's output part (rcor_byte's): every target's row times the basis column with nfix fixes applied
template <int R>
__device__ __forceinline__ void corx_store(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                           const u32 *__restrict__ tabs, const sec::RCorSlots sl, u32 p,
                                           const CxState st, u32 nfix)
{
    const u32 nt = d.e;
    for (u32 g0 = 0; g0 < nt; g0 += R) {
        u32 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            acc[r] = 0u;
        corx_byte_rows<R>(acc, blocks, d, tabs, sl, p, g0, nt - 1, st, nfix);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < nt)
                out[sl.tgt_off[d.tgt0 + g0 + r] + p] = (u8)acc[r];
    }
}

// cor_tally with up to 16 hits per position: the position counts once in `corrected`, every changed
// entry once in its own word
template <bool WAVE, class Slots>
__device__ __forceinline__ void corx_tally(const sec::CorDesc &d, const Slots sl, u32 p, const CxVerdict v,
                                           const CxState st)
{
    u32 *f = sl.flags + d.flag0, *c = sl.flags + d.cnt0;
    if (v.bad)
        min_word(f, p);
    if (v.open)
        min_word(f + 1, p);
    if constexpr (!WAVE) {
        if (v.nfix)
            atomicAdd(c, 1u);
        for (u32 a = 0; a < v.nfix; ++a)
            atomicAdd(c + 2 + st.slot(a), 1u);
        if (v.open)
            atomicAdd(c + 1, 1u);
        return;
    }
    wave_count(c, v.nfix != 0);
    wave_count(c + 1, v.open);
    // per fix index, one atomic per distinct entry among the wave's active lanes (both loops are
    // wave-uniform and bounded: ballots decide them, and every pass clears its leader's bit)
    for (u32 a = 0; a < kCxT; ++a) {
        const int h = a < v.nfix ? (int)st.slot(a) : -1;
        u64 rem = __ballot(h >= 0);
        for (int pass = 0; pass < 64 && rem; ++pass) {
            const u32 lead = (u32)__builtin_ctzll(rem);
            const int hl = __builtin_amdgcn_readlane(h, (int)lead);
            const u64 m = __ballot(h == hl);
            if (cor_lane() == lead)
                atomicAdd(c + 2 + hl, (u32)__builtin_popcountll(m));
            rem &= ~m;
        }
    }
}

template <int R, bool WAVE = true, class Slots>
__device__ __forceinline__ void cor_pos(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                        const u32 *__restrict__ tabs, const Slots sl, u32 p, CorMany j)
{
    const CxState st = cx_state();
    const CxVerdict v = corx_judge<R>(blocks, d, tabs, sl, p, j.tmax, st);
    corx_store<R>(blocks, out, d, tabs, sl, p, st, v.nfix);
    corx_tally<WAVE>(d, sl, p, v, st);
}

constexpr int kCorBatch = 8;  // slots per load batch of cor_rows

// acc[r] = XOR_c T[c][min(row0 + r, rlast)] * slot_c[pos .. pos + 16): R rows of the chunk's table
// from row0 on (a group's rows past rlast repeat row rlast; the caller drops them)
template <int R, class Slots>
__device__ __forceinline__ void cor_rows(u32x4 (&acc)[R], const u8 *__restrict__ blocks, const sec::CorDesc &d,
                                         const u32 *__restrict__ tabs, const Slots sl, u32 pos, u32 row0,
                                         u32 rlast)
{
    const u32 k = d.k, nrows = d.e + d.nr;
#pragma unroll
    for (int r = 0; r < R; ++r)
        acc[r] = u32x4{0u, 0u, 0u, 0u};
    const u32 *rt[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        rt[r] = tabs + d.tab + min(row0 + (u32)r, rlast) * sec::kTabDwords;
    const u32 tstep = nrows * sec::kTabDwords;
#pragma unroll 1
    for (u32 c0 = 0; c0 < k; c0 += kCorBatch) {
        u32x4 xs[kCorBatch][1];
#pragma unroll
        for (int c = 0; c < kCorBatch; ++c)
            if (c0 + c < k)
                xs[c][0] = load16(blocks + sl.off[d.slot0 + c0 + c] + pos);
#pragma unroll
        for (int c = 0; c < kCorBatch; ++c)
            if (c0 + c < k) {
                const Sel<1> s(xs[c]);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const u32 *t = rt[r] + (c0 + c) * tstep;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        acc[r][w] = xor3(acc[r][w], perm(t[1], t[0], s.s0[0][w]), perm(t[3], t[2], s.s1[0][w])) ^
                                    perm(t[4], t[4], s.s2[0][w]);
                }
            }
    }
}

// The OR of every check row's delta over a lane's 16 whole positions [pos, pos + 16), all below
// `valid`: zero when all 16 columns are code words
template <int R, class Slots>
__device__ __forceinline__ u32 cor_lane_deltas(u32x4 (&acc)[R], const u8 *__restrict__ blocks, const sec::CorDesc &d,
                                               u32 pos, const u32 *__restrict__ tabs, const Slots sl)
{
    const u32 k = d.k, e = d.e, nr = d.nr;
    u32 any = 0;
#pragma unroll 1
    for (u32 g0 = 0; g0 < nr; g0 += R) {
        cor_rows<R>(acc, blocks, d, tabs, sl, pos, e + g0, e + nr - 1);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < nr) {
                const u32x4 st = load16(blocks + sl.off[d.slot0 + k + g0 + r] + pos);
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    any |= acc[r][w] ^ st[w];
            }
    }
    return any;
}

// A lane's 16 whole positions [pos, pos + 16), all below `valid`
template <int R, class J = CorOne>
__device__ __forceinline__ void cor_main(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                         u32 pos, const u32 *__restrict__ tabs, const sec::CorSlots sl, J j = {})
{
    const u32 k = d.k, e = d.e;
    u32x4 acc[R];
    const u32 any = cor_lane_deltas<R>(acc, blocks, d, pos, tabs, sl);
    if (any) {
        for (u32 i = 0; i < (u32)sec::kLaneBytes; ++i)
            cor_pos<R>(blocks, out, d, tabs, sl, pos + i, j);
        return;
    }
    u8 *dst = out + d.out_off + pos;
#pragma unroll 1
    for (u32 g0 = 0; g0 < e; g0 += R) {
        cor_rows<R>(acc, blocks, d, tabs, sl, pos, g0, e - 1);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < e)
                store16<SEC_DEC_ST>(dst + (u64)sl.miss[d.slot0 + g0 + r] * d.B, acc[r]);
    }
#pragma unroll 1
    for (u32 c0 = 0; c0 < k; c0 += 4) {
        u32x4 x[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c0 + c < k && sl.row[d.slot0 + c0 + c] != 0xFFFFFFFFu)
                x[c] = load16(blocks + sl.off[d.slot0 + c0 + c] + pos);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c0 + c < k && sl.row[d.slot0 + c0 + c] != 0xFFFFFFFFu)
                store16<SEC_DEC_ST>(dst + (u64)sl.row[d.slot0 + c0 + c] * d.B, x[c]);
    }
}

// R: rows per group (the plan picks the least of 2, 4, 8 that holds the chunk's e + nr rows, else 8)
template <int R>
__global__ __launch_bounds__(sec::kLanes) void sec_decode_correct_kernel(const u8 *__restrict__ blocks,
                                                                         u8 *__restrict__ out,
                                                                         const sec::CorDesc *__restrict__ descs,
                                                                         const sec::Tile *__restrict__ tiles,
                                                                         const u32 *__restrict__ tabs,
                                                                         const sec::CorSlots sl)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::CorDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t + sec::kLaneBytes <= d.valid) {
        cor_main<R>(blocks, out, d, t, tabs, sl);
    } else if (t < d.valid) {  // the lane that straddles `valid`
        for (u32 p = t; p < d.valid; ++p)
            cor_pos<R>(blocks, out, d, tabs, sl, p);
    }
    if (tl.ntail)
        for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x)
            cor_pos<R>(blocks, out, d, tabs, sl, d.valid + i);
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16)
__global__ __launch_bounds__(256) void sec_decode_correct_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                               const sec::CorDesc *__restrict__ descs,
                                                               const sec::TailItem *__restrict__ items, u32 nitems,
                                                               const u32 *__restrict__ tabs, const sec::CorSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::CorDesc d = descs[it.chunk];
    cor_pos<4, false>(blocks, out, d, tabs, sl, it.t);
}

// The same two kernels with corx_judge at the byte level (sec_decode_correct_ex_batch): a lane whose
// check deltas OR to zero takes cor_main's vector path unchanged
template <int R>
__global__ __launch_bounds__(sec::kLanes) void sec_decode_correct_ex_kernel(const u8 *__restrict__ blocks,
                                                                            u8 *__restrict__ out,
                                                                            const sec::CorDesc *__restrict__ descs,
                                                                            const sec::Tile *__restrict__ tiles,
                                                                            const u32 *__restrict__ tabs,
                                                                            const sec::CorSlots sl, const u32 tmax)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::CorDesc d = descs[tl.chunk];
    const CorMany j{tmax};
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t + sec::kLaneBytes <= d.valid) {
        cor_main<R>(blocks, out, d, t, tabs, sl, j);
    } else if (t < d.valid) {  // the lane that straddles `valid`
        for (u32 p = t; p < d.valid; ++p)
            cor_pos<R>(blocks, out, d, tabs, sl, p, j);
    }
    if (tl.ntail)
        for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x)
            cor_pos<R>(blocks, out, d, tabs, sl, d.valid + i, j);
}

__global__ __launch_bounds__(256) void sec_decode_correct_ex_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                                  const sec::CorDesc *__restrict__ descs,
                                                                  const sec::TailItem *__restrict__ items, u32 nitems,
                                                                  const u32 *__restrict__ tabs, const sec::CorSlots sl,
                                                                  const u32 tmax)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::CorDesc d = descs[it.chunk];
    cor_pos<4, false>(blocks, out, d, tabs, sl, it.t, CorMany{tmax});
}

// One thread per entry, after the kernels above: the entry's counter into hits (the caller's
// order); the chunk's first entry also turns the chunk's words into its result.
__global__ __launch_bounds__(256) void sec_decode_correct_final(const sec::CorDesc *__restrict__ descs, u32 nentries,
                                                                const sec::CorSlots sl,
                                                                sec::CorResult *__restrict__ results,
                                                                u32 *__restrict__ hits)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nentries)
        return;
    const sec::CorDesc d = descs[sl.echunk[i]];
    const u32 e = i - d.slot0;
    if (hits)
        hits[d.cslot0 + sl.cpos[i]] = sl.flags[d.cnt0 + 2 + e];
    if (e == 0) {
        const u32 first = sl.flags[d.flag0], fopen = sl.flags[d.flag0 + 1];
        results[d.res] = sec::CorResult{first == ~0u ? ~(u64)0 : (u64)first, fopen == ~0u ? ~(u64)0 : (u64)fopen,
                                        sl.flags[d.cnt0], sl.flags[d.cnt0 + 1]};
    }
}

// ---- repair + correct: regenerate and heal pieces from the column-corrected code word ----------
// Decode + correct with repair + check's outputs.  The chunk's table has rows 0 .. nt-1 for the
// targets (CorDesc::e is nt) and rows nt .. nt+nr-1 for the check rows; every column is judged by
// cor_judge, the verdict decode + correct reaches, and counted by cor_tally into the same words, so
// sec_decode_correct_final reports both.  Target r is a whole B-byte piece at out +
// tgt_off[tgt0 + r], any alignment: byte p = (row r) . (the basis column at p, one slot put right
// where the verdict says so).  A target may be a held entry; it takes the same route through the
// table (a basis entry's row is the unit row, a held check row's equals its check row), so at an
// open position it is what the basis as held predicts.  The two levels are cor_main's: a lane whose
// 16 columns are code words stores every target row as one unaligned 16-byte vector (rchk_main's
// stores), in groups of R rows over the same positions; a lane with a nonzero delta, the lane that
// straddles `valid`, the ragged end [valid, B) and the tail kernel's chunks go byte by byte
// (rcor_byte), and no output byte is written twice.  valid = min(B, every entry's avail): every
// target byte up to B is stored.
template <int R, class J = CorOne>
__device__ __forceinline__ void rcor_main(const u8 *__restrict__ blocks, u8 *__restrict__ out, const sec::CorDesc &d,
                                          u32 pos, const u32 *__restrict__ tabs, const sec::RCorSlots sl, J j = {})
{
    const u32 nt = d.e;
    u32x4 acc[R];
    const u32 any = cor_lane_deltas<R>(acc, blocks, d, pos, tabs, sl);
    if (any) {
        for (u32 i = 0; i < (u32)sec::kLaneBytes; ++i)
            cor_pos<R>(blocks, out, d, tabs, sl, pos + i, j);
        return;
    }
    const u64 *to = sl.tgt_off + d.tgt0;
#pragma unroll 1
    for (u32 g0 = 0; g0 < nt; g0 += R) {
        cor_rows<R>(acc, blocks, d, tabs, sl, pos, g0, nt - 1);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g0 + r < nt)
                store16<SEC_DEC_ST>(out + to[g0 + r] + pos, acc[r]);
    }
}

// R: rows per group (the plan picks the least of 2, 4, 8 that holds the chunk's nt + nr rows, else 8)
template <int R>
__global__ __launch_bounds__(sec::kLanes) void sec_repair_correct_kernel(const u8 *__restrict__ blocks,
                                                                         u8 *__restrict__ out,
                                                                         const sec::CorDesc *__restrict__ descs,
                                                                         const sec::Tile *__restrict__ tiles,
                                                                         const u32 *__restrict__ tabs,
                                                                         const sec::RCorSlots sl)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::CorDesc d = descs[tl.chunk];
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t + sec::kLaneBytes <= d.valid) {
        rcor_main<R>(blocks, out, d, t, tabs, sl);
    } else if (t < d.valid) {  // the lane that straddles `valid`
        for (u32 p = t; p < d.valid; ++p)
            cor_pos<R>(blocks, out, d, tabs, sl, p);
    }
    if (tl.ntail)
        for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x)
            cor_pos<R>(blocks, out, d, tabs, sl, d.valid + i);
}

// One thread per (chunk, position) of the chunks too small for a tile (valid < 16)
__global__ __launch_bounds__(256) void sec_repair_correct_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                               const sec::CorDesc *__restrict__ descs,
                                                               const sec::TailItem *__restrict__ items, u32 nitems,
                                                               const u32 *__restrict__ tabs, const sec::RCorSlots sl)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::CorDesc d = descs[it.chunk];
    cor_pos<4, false>(blocks, out, d, tabs, sl, it.t);
}

// The same two kernels with corx_judge at the byte level (sec_repair_correct_ex_batch)
template <int R>
__global__ __launch_bounds__(sec::kLanes) void sec_repair_correct_ex_kernel(const u8 *__restrict__ blocks,
                                                                            u8 *__restrict__ out,
                                                                            const sec::CorDesc *__restrict__ descs,
                                                                            const sec::Tile *__restrict__ tiles,
                                                                            const u32 *__restrict__ tabs,
                                                                            const sec::RCorSlots sl, const u32 tmax)
{
    const sec::Tile tl = sec::own_tile(tiles);
    const sec::CorDesc d = descs[tl.chunk];
    const CorMany j{tmax};
    const u32 t = tl.t0 + threadIdx.x * sec::kLaneBytes;
    if (t + sec::kLaneBytes <= d.valid) {
        rcor_main<R>(blocks, out, d, t, tabs, sl, j);
    } else if (t < d.valid) {  // the lane that straddles `valid`
        for (u32 p = t; p < d.valid; ++p)
            cor_pos<R>(blocks, out, d, tabs, sl, p, j);
    }
    if (tl.ntail)
        for (u32 i = ragged_lane0(d.valid, tl.t0); i < tl.ntail; i += blockDim.x)
            cor_pos<R>(blocks, out, d, tabs, sl, d.valid + i, j);
}

__global__ __launch_bounds__(256) void sec_repair_correct_ex_tail(const u8 *__restrict__ blocks, u8 *__restrict__ out,
                                                                  const sec::CorDesc *__restrict__ descs,
                                                                  const sec::TailItem *__restrict__ items, u32 nitems,
                                                                  const u32 *__restrict__ tabs, const sec::RCorSlots sl,
                                                                  const u32 tmax)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems)
        return;
    const sec::TailItem it = items[i];
    const sec::CorDesc d = descs[it.chunk];
    cor_pos<4, false>(blocks, out, d, tabs, sl, it.t, CorMany{tmax});
}

// ---- SHA-1 of pieces (storb piece ids, /root/reference/storb/util/piece.py:54-68) ----
// One lane per message: SHA-1 is a sequential chain of 64-byte compressions, so a
// message cannot be split; the kernel is latency-bound on each lane's round chain
// and wants many messages in flight.  Words are loaded 16 B at a time (unaligned
// allowed) and byte-swapped to SHA-1's big-endian order.
__device__ __forceinline__ u32 rotl(u32 x, int n) { return __builtin_amdgcn_alignbit(x, x, 32 - n); }

// FIPS 180-4 SHA-1 compression: per round rotl(a, 5), f (v_bfi / XOR3 / Maj), two add3 and
// rotl(b, 30); per scheduled word XOR3, XOR and a rotate.
__device__ __forceinline__ void sha1_compress(u32 (&h)[5], u32 (&w)[16])
{
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int t = 0; t < 80; ++t) {
        u32 wt;
        if (t < 16) {
            wt = w[t];
        } else {
            wt = rotl(xor3(w[(t - 3) & 15], w[(t - 8) & 15], w[(t - 14) & 15]) ^ w[t & 15], 1);
            w[t & 15] = wt;
        }
        u32 f, k;
        if (t < 20) {
            f = bfi(b, c, d);
            k = 0x5A827999u;
        } else if (t < 40) {
            f = xor3(b, c, d);
            k = 0x6ED9EBA1u;
        } else if (t < 60) {
            f = maj(b, c, d);
            k = 0x8F1BBCDCu;
        } else {
            f = xor3(b, c, d);
            k = 0xCA62C1D6u;
        }
        const u32 tmp = rotl(a, 5) + f + (e + k + wt);
        e = d;
        d = c;
        c = rotl(b, 30);
        b = a;
        a = tmp;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
}

// byte i of the message: real below `avail`, zero from there to `len`
// Blocks are loaded SEC_SHA1_DEPTH ahead of their compression (a ring of registers), so a
// block's load latency overlaps earlier blocks' round chains.  Interleaved in-process A/B
// against the plain loop (tools/sha1_ab.py, profiles/r02_sha1_prefetch_ab.jsonl; HIP-event
// kernel times, median of 7 rounds, spread under 2 %): 1.14x on C4's 114688 pieces of
// 6554 B (1.75 waves per SIMD) and 1.26-1.37x on every other shape measured (C2's 6144
// pieces of 256 KiB, 4096 x 1 MiB, 16384 x 64 KiB, 65536 x 16 KiB, 32768 x 6554 B), so it
// is used for every launch.  (Round 1 kept the plain loop for >= 65536 messages on wall-time
// numbers that were dominated by launch and sync time.)  SEC_SHA1_PF = 0 forces it off (A/B).
#ifndef SEC_SHA1_PF
#define SEC_SHA1_PF 1
#endif
#ifndef SEC_SHA1_DEPTH
#define SEC_SHA1_DEPTH 2
#endif
__device__ __forceinline__ u32 msg_byte(const u8 *p, uint64_t i, uint64_t avail) { return i < avail ? p[i] : 0u; }

template <bool PF>
__global__ __launch_bounds__(64) void sec_sha1_kernel(const u8 *__restrict__ base0, const u8 *__restrict__ base1,
                                                      const sec::MsgDesc *__restrict__ msgs, u32 nmsgs,
                                                      u8 *__restrict__ digests)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nmsgs)
        return;
    const sec::MsgDesc m = msgs[i];
    const u8 *p = (m.base ? base1 : base0) + m.off;
    u32 h[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
    u32 w[16];
    const uint64_t nfull = m.len / 64;
    // PF: the next block's four 16 B loads are issued before this block's compression, so
    // with one wave per SIMD their latency overlaps the round chain
    const uint64_t nfast = PF ? min(nfull, m.avail / 64) : 0;  // blocks wholly inside the real bytes
    // SEC_SHA1_DEPTH blocks ahead (1 or 2), in a ring of registers walked by an unrolled loop
    constexpr int D = SEC_SHA1_DEPTH;
    u32x4 nx[D][4];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if ((uint64_t)d < nfast) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                nx[d][q] = *reinterpret_cast<const u32x4_u *>(p + d * 64 + 16 * q);
        }
    for (uint64_t b0 = 0; b0 < nfast; b0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint64_t blk = b0 + d;
            if (blk < nfast) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    w[4 * q + 0] = __builtin_bswap32(nx[d][q].x);
                    w[4 * q + 1] = __builtin_bswap32(nx[d][q].y);
                    w[4 * q + 2] = __builtin_bswap32(nx[d][q].z);
                    w[4 * q + 3] = __builtin_bswap32(nx[d][q].w);
                }
                if (blk + D < nfast) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        nx[d][q] = *reinterpret_cast<const u32x4_u *>(p + (blk + D) * 64 + 16 * q);
                }
                sha1_compress(h, w);
            }
        }
    }
    for (uint64_t blk = nfast; blk < nfull; ++blk) {
        const uint64_t o = blk * 64;
        if (o + 64 <= m.avail) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 v = *reinterpret_cast<const u32x4_u *>(p + o + 16 * q);
                w[4 * q + 0] = __builtin_bswap32(v.x);
                w[4 * q + 1] = __builtin_bswap32(v.y);
                w[4 * q + 2] = __builtin_bswap32(v.z);
                w[4 * q + 3] = __builtin_bswap32(v.w);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                u32 x = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    x = (x << 8) | msg_byte(p, o + 4 * q + b, m.avail);
                w[q] = x;
            }
        }
        sha1_compress(h, w);
    }
    // final block(s): remaining bytes, 0x80, zeros, 64-bit big-endian bit length
    const uint64_t o = nfull * 64;
    const u32 rem = (u32)(m.len - o);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        u32 x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const u32 pos = 4 * q + b;
            const u32 byte = pos < rem ? msg_byte(p, o + pos, m.avail) : (pos == rem ? 0x80u : 0u);
            x = (x << 8) | byte;
        }
        w[q] = x;
    }
    const uint64_t bits = m.len * 8;
    if (rem >= 56) {
        sha1_compress(h, w);
#pragma unroll
        for (int q = 0; q < 16; ++q)
            w[q] = 0;
    }
    w[14] = (u32)(bits >> 32);
    w[15] = (u32)bits;
    sha1_compress(h, w);
    u32 *out = reinterpret_cast<u32 *>(digests + (uint64_t)i * 20);
#pragma unroll
    for (int q = 0; q < 5; ++q)
        out[q] = __builtin_bswap32(h[q]);
}

// SHA-1 with the message schedule on a second wave (few, long messages: the latency-bound
// regime, e.g. C2's 6144 pieces of 256 KiB are 96 waves, one per SIMD at most).  A workgroup is
// two waves for the same 64 messages: wave 1 loads each block (prefetched), byte-swaps it and
// expands the 80 schedule words W_t + K_t into LDS; wave 0 runs only the 80 rounds from LDS
// (rotl 5, f, add3, add, rotl 30: 5 VALU per round, 405 per block against 597 with the
// schedule inline), one block behind, the two buffers handed over by one s_barrier per block.
// Blocks past a message's real bytes (zfec's zero padding) and the final padded block(s) go
// through sha1_compress on wave 0 afterwards, as in sec_sha1_kernel.
constexpr u32 kShaK[4] = {0x5A827999u, 0x6ED9EBA1u, 0x8F1BBCDCu, 0xCA62C1D6u};

__device__ __forceinline__ void sha1_rounds_wk(u32 (&h)[5], const u32x4 (&vs)[20])
{
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int q = 0; q < 20; ++q) {
        const u32x4 v = vs[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = 4 * q + j;
            const u32 f = t < 20 ? bfi(b, c, d) : t < 40 ? xor3(b, c, d) : t < 60 ? maj(b, c, d) : xor3(b, c, d);
            const u32 tmp = rotl(a, 5) + f + e + v[j];
            e = d;
            d = c;
            c = rotl(b, 30);
            b = a;
            a = tmp;
        }
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
}

// one block's 80 words from LDS into registers (left to the scheduler, the reads went out two
// at a time, each pair waited for a few rounds later: 1.06x over the one-lane kernel, not 1.26x)
__device__ __forceinline__ void sha1_fetch_wk(u32x4 (&vs)[20], const u32x4 *__restrict__ wk, u32 lane)
{
#pragma unroll
    for (int q = 0; q < 20; ++q)
        vs[q] = wk[q * 64 + lane];
}

// W_t + K_t of one block (16 big-endian words in w) into wk[t / 4][lane][t % 4]
__device__ __forceinline__ void sha1_schedule_wk(u32 (&w)[16], u32x4 *__restrict__ wk, u32 lane)
{
#pragma unroll
    for (int q = 0; q < 20; ++q) {
        u32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = 4 * q + j;
            u32 wt;
            if (t < 16) {
                wt = w[t];
            } else {
                wt = rotl(xor3(w[(t - 3) & 15], w[(t - 8) & 15], w[(t - 14) & 15]) ^ w[t & 15], 1);
                w[t & 15] = wt;
            }
            v[j] = wt + kShaK[t / 20];
        }
        wk[q * 64 + lane] = v;
    }
}

__global__ __launch_bounds__(128) void sec_sha1_split_kernel(const u8 *__restrict__ base0, const u8 *__restrict__ base1,
                                                              const sec::MsgDesc *__restrict__ msgs, u32 nmsgs,
                                                              u8 *__restrict__ digests)
{
    __shared__ u32x4 s_wk[2][20 * 64];  // two blocks' W + K, [t / 4][lane]
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 i = blockIdx.x * 64 + lane;
    const bool live = i < nmsgs;
    sec::MsgDesc m{};
    if (live)
        m = msgs[i];
    const u8 *p = (m.base ? base1 : base0) + m.off;
    const uint64_t nfast = live ? min(m.len / 64, m.avail / 64) : 0;  // blocks wholly inside the real bytes
    // the workgroup walks the longest message's blocks (shorter ones idle, masked)
    uint64_t nmax = nfast;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        nmax = max(nmax, (uint64_t)__shfl_xor((unsigned long long)nmax, o, 64));
    u32 h[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
    // Two LDS buffers, one barrier per block: before barrier j wave 1 has written block j into
    // buffer j & 1, and wave 0 has finished block j - 1 (buffer (j - 1) & 1, which wave 1 fills
    // next).  (Three buffers with block j + 1 read into registers during block j measured
    // 1.22-1.25x over the one-lane kernel against 1.23-1.26x for this form.)
    if (wave == 1) {  // the schedule, one block ahead of wave 0; loads two blocks ahead of that
        u32x4 nx[2][4];
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if ((uint64_t)d < nfast) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    nx[d][q] = *reinterpret_cast<const u32x4_u *>(p + d * 64 + 16 * q);
            }
        for (uint64_t b0 = 0; b0 < nmax; b0 += 2) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const uint64_t blk = b0 + d;
                if (blk >= nmax)
                    break;
                if (blk < nfast) {
                    u32 w[16];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        w[4 * q + 0] = __builtin_bswap32(nx[d][q].x);
                        w[4 * q + 1] = __builtin_bswap32(nx[d][q].y);
                        w[4 * q + 2] = __builtin_bswap32(nx[d][q].z);
                        w[4 * q + 3] = __builtin_bswap32(nx[d][q].w);
                    }
                    if (blk + 2 < nfast) {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            nx[d][q] = *reinterpret_cast<const u32x4_u *>(p + (blk + 2) * 64 + 16 * q);
                    }
                    sha1_schedule_wk(w, s_wk[d], lane);
                }
                __syncthreads();  // barrier blk
            }
        }
        __syncthreads();  // barrier nmax, wave 0's last (both waves take nmax + 1 barriers)
        return;
    }
    __syncthreads();  // barrier 0: block 0 is in buffer 0
    for (uint64_t blk = 0; blk < nmax; ++blk) {
        if (blk < nfast) {
            u32x4 v[20];
            sha1_fetch_wk(v, s_wk[blk & 1], lane);
            __builtin_amdgcn_sched_barrier(0);  // all 20 reads out before the first round
            sha1_rounds_wk(h, v);
        }
        __syncthreads();  // barrier blk + 1: block blk + 1 is in its buffer, buffer blk & 1 free
    }
    if (!live)
        return;
    u32 w[16];
    const uint64_t nfull = m.len / 64;
    for (uint64_t blk = nfast; blk < nfull; ++blk) {
        const uint64_t o = blk * 64;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            u32 x = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                x = (x << 8) | msg_byte(p, o + 4 * q + b, m.avail);
            w[q] = x;
        }
        sha1_compress(h, w);
    }
    const uint64_t o = nfull * 64;
    const u32 rem = (u32)(m.len - o);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        u32 x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const u32 pos = 4 * q + b;
            const u32 byte = pos < rem ? msg_byte(p, o + pos, m.avail) : (pos == rem ? 0x80u : 0u);
            x = (x << 8) | byte;
        }
        w[q] = x;
    }
    const uint64_t bits = m.len * 8;
    if (rem >= 56) {
        sha1_compress(h, w);
#pragma unroll
        for (int q = 0; q < 16; ++q)
            w[q] = 0;
    }
    w[14] = (u32)(bits >> 32);
    w[15] = (u32)bits;
    sha1_compress(h, w);
    u32 *out = reinterpret_cast<u32 *>(digests + (uint64_t)i * 20);
#pragma unroll
    for (int q = 0; q < 5; ++q)
        out[q] = __builtin_bswap32(h[q]);
}

// Timing events for the next launch (sec_launch_events): the kernel's own dispatch records
// them (hipExtLaunchKernelGGL), so timing adds no marker packets between kernels.  Two event
// records per launch around back-to-back kernels cost the bench 3-5 % of its rate.
// The start event goes to the first launch after sec_launch_events, the stop event to every
// launch until the next call (the last record of an event is the one timed).
thread_local hipEvent_t t_start = nullptr, t_stop = nullptr;
thread_local int t_launched = 0;

template <class K, class... A>
hipError_t launch_shm(K kernel, dim3 grid, dim3 block, u32 shm, hipStream_t s, A... args)
{
    hipEvent_t a = t_start;
    t_start = nullptr;
    ++t_launched;
    hipExtLaunchKernelGGL(kernel, grid, block, shm, s, a, t_stop, 0, args...);
    return hipGetLastError();
}
template <class K, class... A>
hipError_t launch(K kernel, dim3 grid, dim3 block, hipStream_t s, A... args)
{
    return launch_shm(kernel, grid, block, 0, s, args...);
}

// rows -> f(std::integral_constant<int, R>), R in [R0, 8] (the row counts the tile kernels are built for)
template <int R0, class F>
hipError_t with_rows(int rows, F f)
{
    switch (rows) {
    case 0:
        if constexpr (R0 == 0)
            return f(std::integral_constant<int, 0>{});
        return hipErrorInvalidValue;
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
    }
}

template <int U, bool W>
hipError_t dispatch_enc(int rows, const u8 *in, u8 *par, const sec::EncDesc *d, const sec::Tile *t, u32 nt,
                        const u32 *tabs, u32 lanes, hipStream_t s)
{
    return with_rows<1>(rows, [&](auto r) {
        constexpr int R = decltype(r)::value;
        return launch_shm(sec_encode_kernel<R, U, W>, dim3(nt), dim3(lanes),
                          lds_tab_bytes<batch_blocks<U, W, false>(), R, false>(lanes), s, in, par, d, t, tabs);
    });
}

// The tile kernels that take (blocks[, out], descs, tiles, tabs, slots), by descriptor type: the
// kernel of R rows, the lowest R built, the tail kernel, and whether there is an `out`.
template <class Desc>
struct RowKernels;
#define SEC_ROW_KERNELS(Desc, R0, OUT, TILE, TAIL)                                 \
    template <>                                                                    \
    struct RowKernels<sec::Desc> {                                                 \
        static constexpr int kRows0 = R0;                                          \
        static constexpr bool kOut = OUT;                                          \
        template <int R, bool W, int KBX>                                          \
        static constexpr auto tile() { return TILE<R, 1, W, KBX>; }                \
        static constexpr auto tail() { return TAIL; }                              \
    }
SEC_ROW_KERNELS(DecDesc, 0, true, sec_decode_kernel, sec_decode_tail);
SEC_ROW_KERNELS(RepDesc, 1, true, sec_repair_kernel, sec_repair_tail);
SEC_ROW_KERNELS(ChkDesc, 1, false, sec_check_kernel, sec_check_tail);
SEC_ROW_KERNELS(DChkDesc, 0, true, sec_decode_check_kernel, sec_decode_check_tail);
SEC_ROW_KERNELS(RChkDesc, 1, true, sec_repair_check_kernel, sec_repair_check_tail);
#undef SEC_ROW_KERNELS

template <bool W, int KBX, class Desc, class Slots>
hipError_t dispatch_rows(int rows, const u8 *b, u8 *o, const Desc *d, const sec::Tile *t, u32 nt, const u32 *tabs,
                         Slots sl, u32 lanes, hipStream_t s)
{
    using K = RowKernels<Desc>;
    return with_rows<K::kRows0>(rows, [&](auto r) {
        constexpr int R = decltype(r)::value;
        constexpr int KB = KBX > 0 ? KBX : batch_blocks<1, W, true>();
        const u32 shm = lds_tab_bytes<KB, R, true>(lanes);
        if constexpr (K::kOut)
            return launch_shm(K::template tile<R, W, KBX>(), dim3(nt), dim3(lanes), shm, s, b, o, d, t, tabs, sl);
        else
            return launch_shm(K::template tile<R, W, KBX>(), dim3(nt), dim3(lanes), shm, s, b, d, t, tabs, sl);
    });
}

}  // namespace

void sec_next_launch_events(void **start, void **stop)
{
    *start = t_start;
    t_start = nullptr;
    *stop = t_stop;
    ++t_launched;
}

int sec_launch_events(void *start, void *stop)
{
    const int n = t_launched;
    t_start = (hipEvent_t)start;
    t_stop = (hipEvent_t)stop;
    t_launched = 0;
    return n;
}

int sec_launch_expand(const uint8_t *coef, uint32_t ncoef, uint32_t *tabs, void *stream)
{
    if (ncoef == 0)
        return hipSuccess;
    return launch(sec_expand_tables, dim3((ncoef + 255) / 256), dim3(256), (hipStream_t)stream, coef, ncoef, tabs);
}

int sec_launch_encode(int rows, int U, int wide, int lanes, const uint8_t *in, uint8_t *par,
                      const sec::EncDesc *descs, const sec::Tile *tiles, uint32_t ntiles, const uint32_t *tabs,
                      void *stream)
{
    if (ntiles == 0)
        return hipSuccess;
    if (lanes < 64 || lanes % 64 || lanes > sec::max_lanes(rows, U) || (wide && U != 1))
        return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (wide)
        return dispatch_enc<1, true>(rows, in, par, descs, tiles, ntiles, tabs, (u32)lanes, s);
    if (U != 1)  // U > 1 tiles measured slower (profiles/r01_sweep_u.jsonl) and are not built
        return hipErrorInvalidValue;
    return dispatch_enc<1, false>(rows, in, par, descs, tiles, ntiles, tabs, (u32)lanes, s);
}

int sec_launch_encode_tail(const uint8_t *in, uint8_t *par, const sec::EncDesc *descs, const sec::TailItem *items,
                           uint32_t nitems, const uint32_t *tabs, void *stream)
{
    if (nitems == 0)
        return hipSuccess;
    return launch(sec_encode_tail, dim3((nitems + 255) / 256), dim3(256), (hipStream_t)stream, in, par, descs, items,
                  nitems, tabs);
}

template <class Desc, class Slots>
int sec_launch_rows(int rows, int U, int wide, int lanes, const uint8_t *blocks, uint8_t *out, const Desc *descs,
                    const sec::Tile *tiles, uint32_t ntiles, const uint32_t *tabs, Slots sl, void *stream, int kb)
{
    if (ntiles == 0)
        return hipSuccess;
    if (rows < RowKernels<Desc>::kRows0 || U != 1 || lanes < 64 || lanes % 64 || lanes > sec::max_lanes(rows, U))
        return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const u32 L = (u32)lanes;
    if (kb) {  // small load batches: tiles of chunks with k <= kb only
        if (wide || kb != 4)
            return hipErrorInvalidValue;
        return dispatch_rows<false, 4>(rows, blocks, out, descs, tiles, ntiles, tabs, sl, L, s);
    }
    if (wide)
        return dispatch_rows<true, 0>(rows, blocks, out, descs, tiles, ntiles, tabs, sl, L, s);
    return dispatch_rows<false, 0>(rows, blocks, out, descs, tiles, ntiles, tabs, sl, L, s);
}

template <class Desc, class Slots>
int sec_launch_rows_tail(const uint8_t *blocks, uint8_t *out, const Desc *descs, const sec::TailItem *items,
                         uint32_t nitems, const uint32_t *tabs, Slots sl, void *stream)
{
    if (nitems == 0)
        return hipSuccess;
    using K = RowKernels<Desc>;
    const dim3 grid((nitems + 255) / 256), block(256);
    if constexpr (K::kOut)
        return launch(K::tail(), grid, block, (hipStream_t)stream, blocks, out, descs, items, nitems, tabs, sl);
    else
        return launch(K::tail(), grid, block, (hipStream_t)stream, blocks, descs, items, nitems, tabs, sl);
}

#define SEC_ROW_LAUNCHERS(Desc, Slots)                                                                              \
    template int sec_launch_rows(int, int, int, int, const uint8_t *, uint8_t *, const sec::Desc *,                 \
                                 const sec::Tile *, uint32_t, const uint32_t *, sec::Slots, void *, int);           \
    template int sec_launch_rows_tail(const uint8_t *, uint8_t *, const sec::Desc *, const sec::TailItem *,         \
                                      uint32_t, const uint32_t *, sec::Slots, void *)
// (kernel templates land in the code object in the order of their first use here: the decode's,
// the SHA-1 kernels, then the other families, as tools/kres.py lists them)
SEC_ROW_LAUNCHERS(DecDesc, DecSlots);

int sec_launch_sha1(const uint8_t *base0, const uint8_t *base1, const sec::MsgDesc *msgs, uint32_t nmsgs,
                    uint8_t *digests, void *stream, int split)
{
    if (nmsgs == 0)
        return hipSuccess;
    if (split)
        return launch(sec_sha1_split_kernel, dim3((nmsgs + 63) / 64), dim3(128), (hipStream_t)stream, base0, base1,
                      msgs, nmsgs, digests);
    if (SEC_SHA1_PF)
        return launch(sec_sha1_kernel<true>, dim3((nmsgs + 63) / 64), dim3(64), (hipStream_t)stream, base0, base1, msgs,
                      nmsgs, digests);
    return launch(sec_sha1_kernel<false>, dim3((nmsgs + 63) / 64), dim3(64), (hipStream_t)stream, base0, base1, msgs,
                  nmsgs, digests);
}

SEC_ROW_LAUNCHERS(RepDesc, RepSlots);
SEC_ROW_LAUNCHERS(ChkDesc, ChkSlots);
SEC_ROW_LAUNCHERS(DChkDesc, DChkSlots);
SEC_ROW_LAUNCHERS(RChkDesc, RChkSlots);
#undef SEC_ROW_LAUNCHERS

int sec_launch_check_final(const uint8_t *blocks, const sec::ChkDesc *descs, uint32_t nentries, sec::ChkSlots sl,
                           sec::ChkResult *results, uint8_t *row_bad, uint8_t *column, void *stream)
{
    if (nentries == 0)
        return hipSuccess;
    return launch(sec_check_final, dim3((nentries + 255) / 256), dim3(256), (hipStream_t)stream, blocks, descs,
                  nentries, sl, results, row_bad, column);
}

int sec_launch_correct(int rows, const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::Tile *tiles,
                       uint32_t ntiles, const uint32_t *tabs, sec::CorSlots sl, void *stream, uint32_t tmax)
{
    if (ntiles == 0)
        return hipSuccess;
    const dim3 grid(ntiles), block(sec::kLanes);
    hipStream_t s = (hipStream_t)stream;
    switch (tmax ? rows : 0) {
    case 2: return launch(sec_decode_correct_ex_kernel<2>, grid, block, s, blocks, out, descs, tiles, tabs, sl, tmax);
    case 4: return launch(sec_decode_correct_ex_kernel<4>, grid, block, s, blocks, out, descs, tiles, tabs, sl, tmax);
    case 8: return launch(sec_decode_correct_ex_kernel<8>, grid, block, s, blocks, out, descs, tiles, tabs, sl, tmax);
    case 0: break;
    default: return hipErrorInvalidValue;
    }
    switch (rows) {
    case 2: return launch(sec_decode_correct_kernel<2>, grid, block, s, blocks, out, descs, tiles, tabs, sl);
    case 4: return launch(sec_decode_correct_kernel<4>, grid, block, s, blocks, out, descs, tiles, tabs, sl);
    case 8: return launch(sec_decode_correct_kernel<8>, grid, block, s, blocks, out, descs, tiles, tabs, sl);
    default: return hipErrorInvalidValue;
    }
}

int sec_launch_correct_tail(const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::TailItem *items,
                            uint32_t nitems, const uint32_t *tabs, sec::CorSlots sl, void *stream, uint32_t tmax)
{
    if (nitems == 0)
        return hipSuccess;
    if (tmax)
        return launch(sec_decode_correct_ex_tail, dim3((nitems + 255) / 256), dim3(256), (hipStream_t)stream, blocks,
                      out, descs, items, nitems, tabs, sl, tmax);
    return launch(sec_decode_correct_tail, dim3((nitems + 255) / 256), dim3(256), (hipStream_t)stream, blocks, out,
                  descs, items, nitems, tabs, sl);
}

int sec_launch_correct(int rows, const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::Tile *tiles,
                       uint32_t ntiles, const uint32_t *tabs, sec::RCorSlots sl, void *stream, uint32_t tmax)
{
    if (ntiles == 0)
        return hipSuccess;
    const dim3 grid(ntiles), block(sec::kLanes);
    hipStream_t s = (hipStream_t)stream;
    switch (tmax ? rows : 0) {
    case 2: return launch(sec_repair_correct_ex_kernel<2>, grid, block, s, blocks, out, descs, tiles, tabs, sl, tmax);
    case 4: return launch(sec_repair_correct_ex_kernel<4>, grid, block, s, blocks, out, descs, tiles, tabs, sl, tmax);
    case 8: return launch(sec_repair_correct_ex_kernel<8>, grid, block, s, blocks, out, descs, tiles, tabs, sl, tmax);
    case 0: break;
    default: return hipErrorInvalidValue;
    }
    switch (rows) {
    case 2: return launch(sec_repair_correct_kernel<2>, grid, block, s, blocks, out, descs, tiles, tabs, sl);
    case 4: return launch(sec_repair_correct_kernel<4>, grid, block, s, blocks, out, descs, tiles, tabs, sl);
    case 8: return launch(sec_repair_correct_kernel<8>, grid, block, s, blocks, out, descs, tiles, tabs, sl);
    default: return hipErrorInvalidValue;
    }
}

int sec_launch_correct_tail(const uint8_t *blocks, uint8_t *out, const sec::CorDesc *descs, const sec::TailItem *items,
                            uint32_t nitems, const uint32_t *tabs, sec::RCorSlots sl, void *stream, uint32_t tmax)
{
    if (nitems == 0)
        return hipSuccess;
    if (tmax)
        return launch(sec_repair_correct_ex_tail, dim3((nitems + 255) / 256), dim3(256), (hipStream_t)stream, blocks,
                      out, descs, items, nitems, tabs, sl, tmax);
    return launch(sec_repair_correct_tail, dim3((nitems + 255) / 256), dim3(256), (hipStream_t)stream, blocks, out,
                  descs, items, nitems, tabs, sl);
}

int sec_launch_correct_final(const sec::CorDesc *descs, uint32_t nentries, sec::CorSlots sl, sec::CorResult *results,
                             uint32_t *hits, void *stream)
{
    if (nentries == 0)
        return hipSuccess;
    return launch(sec_decode_correct_final, dim3((nentries + 255) / 256), dim3(256), (hipStream_t)stream, descs,
                  nentries, sl, results, hits);
}
