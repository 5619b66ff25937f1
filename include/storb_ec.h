/*
 * storb_ec.h — C ABI of libstorbec.so, the MI355X (gfx950) Reed–Solomon engine
 * behind storb's chunk-and-shard path.
 *
 * Boundary.  In the reference the path crosses into native code at zfec's
 * CPython extension:
 *   zfec.easyfec.Encoder(k, m).encode(chunk)         /root/reference/storb/util/piece.py:129-130
 *   zfec.easyfec.Decoder(k, m).decode(b, s, padlen)  /root/reference/storb/util/piece.py:196-197
 * (zfec 1.6.0.0, /root/reference/uv.lock:1088-1091; import at piece.py:8).
 * This header replaces that extension with plain C entry points (no torch or
 * HIP types in any signature) that a ctypes / cffi / cgo binding can bind
 * directly; storb_amd/_lib.py is the ctypes binding, INTEGRATION.md shows it.
 *
 * Conventions (zfec's, kept on purpose):
 *   k = data blocks, m = TOTAL blocks (data + parity), 1 <= k <= m <= 256
 *   B = ceil(n / k) bytes per block; padlen = k*B - n; the last data block
 *   is zero-padded to B (easyfec).  Block numbers 0..k-1 are primaries
 *   (systematic: the chunk bytes themselves), k..m-1 are secondaries.
 *
 * Ownership.  The caller owns every buffer passed in; the library never frees
 * caller memory.  Device scratch, coefficient tables, pinned staging and
 * streams belong to the sec_ctx and are reused across calls.
 *
 * Threading.  One sec_ctx per (device, host thread).  Calls on different
 * contexts are independent; a context must not be used from two threads at
 * once.
 *
 * Errors.  Every int-returning function returns SEC_OK (0) or a negative
 * SEC_E* code; sec_strerror() names it.  The zfec preconditions map as
 * follows (zfec raises zfec.Error for each; storb_amd.easyfec raises
 * storb_amd.easyfec.Error with the same message text).
 */
#ifndef STORB_EC_H
#define STORB_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEC_ABI_VERSION 1

enum sec_status {
    SEC_OK = 0,
    SEC_EINVAL = -1,     /* NULL pointer / negative count / bad flag                  */
    SEC_EKM = -2,        /* 1 <= k <= m <= 256 violated (zfec Encoder/Decoder init)    */
    SEC_EBLOCKLEN = -3,  /* blocks not all the same length (easyfec short middle slice) */
    SEC_ENBLOCKS = -4,   /* decode given other than exactly k blocks                   */
    SEC_ESHARENUM = -5,  /* sharenum < 0 or >= m                                       */
    SEC_EDUPSHARE = -6,  /* duplicate sharenum                                         */
    SEC_EPADLEN = -7,    /* padlen > k*B                                               */
    SEC_ESIZE = -8,      /* block size B >= 2^31 bytes                                 */
    SEC_ENODEV = -9,     /* no HIP device / bad device ordinal                         */
    SEC_EHIP = -10,      /* HIP runtime error; sec_last_hip_error() has the text       */
    SEC_ENOMEM = -11,    /* device / pinned allocation failed                          */
    SEC_ESINGULAR = -12, /* decode matrix singular (cannot happen for valid inputs)    */
    SEC_EMODULUS = -13,  /* bignum modulus not an odd 2048-bit integer                 */
    SEC_ENOTAG = -14,    /* APDP call on a key without sec_bn_key_set_tag              */
    SEC_ENOCRT = -15     /* CRT call on a key without sec_bn_key_set_crt               */
};

/* flags for sec_encode_batch / sec_decode_batch */
#define SEC_F_HOST 1u  /* in/out/blocks are HOST pointers; the call returns when the
                          results are back in host memory.  When every buffer of an
                          encode / decode lies in pinned memory mapped at the same address
                          on the device (sec_host_alloc, sec_host_register, hipHostMalloc),
                          the kernels read and write it directly over PCIe: no staging
                          copy.  Pageable buffers of a large call (context option SEC_REGISTER_MIN
                          bytes, default 4 MiB, in ranges of >= 1 MiB on average) are page-locked
                          for the call and used the same way; otherwise (or if locking
                          fails) they are staged through pinned slabs and device scratch.
                          sec_ctx_host_paths counts which path each call took        */
#define SEC_F_ASYNC 2u /* device pointers only: return once enqueued on the context
                          stream (sec_sync() waits)                                  */
#define SEC_F_RECOVER 4u /* decode only, recover-only: write just the chunk's missing
                          primaries, i.e. what zfec's fec_decode itself produces: the
                          e = (primaries absent from the chunk's k blocks) recovered
                          blocks, B bytes each (block k-1 with its zero padding), in
                          increasing block number at out + out_off + r*B.  Present
                          primaries are not copied; a chunk with e = 0 writes nothing  */
#define SEC_F_STAGED 8u /* SEC_F_HOST only: never page-lock pageable buffers for this call
                          (they are staged; persistently pinned ones stay zero-copy).
                          Page-locking takes the process's memory-map lock, so it stalls
                          while other threads fault in or free memory: one 8 MiB encode
                          beside storb's piece copies took 6.4 ms locked, 0.55 ms staged */
#define SEC_F_GPU_PARITY_IDS 16u /* sec_encode_pieces with digests only: the parity pieces'
                          SHA-1 ids come from the GPU (sec_sha1_kernel on the parity while it
                          is device-resident, one lane per piece, sub-batches of up to
                          SEC_SLAB_BYTES_DIGEST input bytes) while the host threads hash the
                          data pieces; without it the host threads hash every piece  */

typedef struct sec_ctx sec_ctx;

/* One chunk to encode: the easyfec.Encoder(k, m).encode(chunk) of piece.py:129-130. */
typedef struct sec_enc_chunk {
    uint64_t in_off;        /* byte offset of the chunk in `in`                       */
    uint64_t n;             /* chunk bytes (EncodedChunk.original_chunk_size)         */
    uint64_t parity_off;    /* byte offset in `parity` of block k (first secondary)   */
    uint64_t parity_stride; /* bytes from one secondary block to the next (>= B)      */
    int32_t k;              /* data blocks                                            */
    int32_t m;              /* total blocks                                           */
} sec_enc_chunk;

/* One chunk to reassemble: the easyfec.Decoder(k, m).decode(blocks, sharenums,
 * padlen) of piece.py:196-197.  The chunk's k blocks are entries
 * slot0 .. slot0+k-1 of the call's sharenums[] / block_offs[] arrays. */
typedef struct sec_dec_chunk {
    uint64_t out_off; /* byte offset in `out` of the k*B - padlen reassembled bytes    */
    uint64_t B;       /* block size (EncodedChunk.chunk_size)                          */
    uint64_t padlen;  /* EncodedChunk.padlen                                           */
    uint64_t slot0;   /* first index into sharenums[] / block_offs[]                   */
    int32_t k;
    int32_t m;
} sec_dec_chunk;

/* ---- library / device ------------------------------------------------- */
int sec_abi_version(void);
const char *sec_strerror(int status);
const char *sec_last_hip_error(void);          /* thread-local text of the last SEC_EHIP */
int sec_device_count(int *count);              /* SEC_ENODEV when the HIP runtime has none */

/* ---- context ------------------------------------------------------------ */
int sec_ctx_create(int device, sec_ctx **out);
void sec_ctx_destroy(sec_ctx *ctx);
/* Launch on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the context's own stream, which is created blocking (ordered with
 * the legacy NULL stream, torch's default stream).  Producers on any other stream
 * must be ordered by the caller (or the context switched onto their stream). */
int sec_ctx_set_stream(sec_ctx *ctx, void *hip_stream);
int sec_sync(sec_ctx *ctx);
/* HIP-event timing of the hot kernels: when enabled every batch call records an
 * event pair around its encode / decode kernels on the launch stream. */
int sec_ctx_set_timing(sec_ctx *ctx, int enable);
/* Waits for recorded pairs, returns the summed milliseconds and launch count of
 * kind 0 = encode, 1 = decode, 2 = SHA-1, 3 = bignum (APDP), 4 = repair (its kernels and,
 * with digests, their SHA-1), 5 = check, 6 = decode + check, 7 = repair + check (its main kernel and
 * tail, sec_check_final and, with digests, their SHA-1), 8 = the correcting calls: decode + correct, repair +
 * correct (with digests, their SHA-1 too), and clears them. */
int sec_timing_collect(sec_ctx *ctx, int kind, double *total_ms, int64_t *launches);

/* ---- context options --------------------------------------------------------
 * The library picks kernels, tile widths and host paths by measured rules and reads no
 * environment variable.  A test or an A/B tool that must force another choice sets it on
 * its own context; the context's cached plans are dropped, so the next call is planned
 * with it.  Names (e.g. "SEC_SYN": -1 cost rule, 0 direct decode, 1 syndrome path;
 * "SEC_BS"; "SEC_REGISTER_MIN": bytes, 0 = never page-lock) are listed by
 * sec_option_name(0, 1, ...) up to NULL; their meaning is documented in api.cpp (enum Opt).
 * Only options that force a shipped path or size the host pipeline exist (round 5 archived
 * the A/B-only ones with their kernels).
 * No zfec counterpart: the reference has no tuning surface on this path.
 * SEC_EINVAL for an unknown name or a value out of the option's range. */
int sec_ctx_set_option(sec_ctx *ctx, const char *name, int64_t value);
/* The context's value (NULL ctx: the library default). */
int sec_ctx_get_option(sec_ctx *ctx, const char *name, int64_t *value);
const char *sec_option_name(int index);

/* ---- choosing the blocks to decode from (host logic, no device needed) ---------------
 * A caller holding n > k blocks of a chunk (storb's validator fetches every data and parity
 * piece: validator.py:1556-1604, 1631) passes their sharenums; pick[0..k) receives the
 * positions of the k blocks to hand to sec_decode_batch(_ex): every present primary, then
 * parity rows from as few of the decode kernels' row groups as possible (the cheapest decode;
 * any k distinct blocks give the same bytes).  Replaces the reference's `pieces[:k]`
 * (storb/util/piece.py:189-191).  Out-of-range and repeated sharenums are never chosen;
 * SEC_ENBLOCKS when fewer than k distinct valid ones are present. */
int sec_decode_choose(int k, int m, int64_t n, const int32_t *sharenums, int32_t *pick);

/* ---- matrices (host arithmetic, no device needed) ------------------------ */
/* Rows k..m-1 of zfec's systematic encode matrix ((m-k)*k bytes, row-major). */
int sec_encode_matrix(int k, int m, uint8_t *out_rows);
/* zfec decode matrix for the given k sharenums: slots normalised as
 * _fecmodule.c does (each primary moved to its own slot), rows built, inverted.
 * out: k*k bytes of the inverse; out_index (nullable): k normalised sharenums. */
int sec_decode_matrix(int k, int m, const int32_t *sharenums, uint8_t *out, int32_t *out_index);

/* ---- the hot path ----------------------------------------------------------
 * Encode: for every chunk, parity block r (r = k..m-1) is written at
 * parity + parity_off + (r-k)*parity_stride, B bytes.  Data blocks are not
 * written: they are the chunk bytes themselves (systematic code); the zero
 * padding of the last data block is synthesised, never read from `in`.
 */
int sec_encode_batch(sec_ctx *ctx, const sec_enc_chunk *chunks, int64_t nchunks,
                     const uint8_t *in, uint8_t *parity, unsigned flags);

/* Decode + reassemble: for every chunk, its k blocks are at
 * blocks + block_offs[slot0 + i] (B bytes each) with block numbers
 * sharenums[slot0 + i]; the chunk's k*B - padlen bytes are written at
 * out + out_off.  Present primaries are copied, missing ones recovered.
 * `blocks` may be NULL, in which case block_offs are absolute addresses.
 * Every block must have B readable bytes here; sec_decode_batch_ex lifts that.
 * SEC_F_RECOVER: recover-only output instead (see the flag).
 * Aliasing: a chunk's output range must not overlap any block of any chunk in
 * the call (no in-place reassembly).  The kernels read blocks while other
 * workgroups write `out`, and a SEC_F_HOST call joins present primaries on the
 * host while the device writes the recovered rows, so an overlap gives
 * unspecified bytes.  The library does not check this. */
int sec_decode_batch(sec_ctx *ctx, const sec_dec_chunk *chunks, int64_t nchunks,
                     const int32_t *sharenums, const uint64_t *block_offs,
                     const uint8_t *blocks, uint8_t *out, unsigned flags);

/* sec_decode_batch with a readable length per block: block_avail[slot0 + i] bytes
 * of block i exist at its address and bytes [avail, B) read as zero (values
 * above B count as B; block_avail NULL = every block has B).  This is zfec's
 * padded last data block read in place from the chunk buffer: avail = B - padlen
 * (the same mechanism as sec_msg.avail).  Nothing past a block's avail is read. */
int sec_decode_batch_ex(sec_ctx *ctx, const sec_dec_chunk *chunks, int64_t nchunks,
                        const int32_t *sharenums, const uint64_t *block_offs,
                        const uint64_t *block_avail, const uint8_t *blocks, uint8_t *out,
                        unsigned flags);

/* ---- repair: lost pieces regenerated from any k survivors ---------------------------------
 * A miner is gone; the validator still reaches k other pieces of the chunk and needs the lost
 * pieces back AS PIECES, data or parity, to seed them elsewhere, and their piece ids to check
 * against what it recorded at upload.  Block t of the code word is a fixed GF(2^8) combination of
 * any k blocks: row t of zfec's encode matrix times the inverse sec_decode_matrix returns.  No
 * zfec counterpart: the reference would decode the chunk and encode it again.
 *
 * sec_repair_matrix (host arithmetic, no device needed): the ntargets x k matrix, row-major, row r
 * for block targets[r], columns in the caller's sharenum order, so that
 *     block targets[r] = XOR_j out[r*k + j] * (block sharenums[j]).
 * Errors, checked in this order and shared with sec_repair_batch (there before any device work):
 * SEC_EINVAL ntargets < 0 or a NULL array; SEC_EKM; SEC_ESHARENUM a source or target outside
 * [0, m); SEC_EDUPSHARE a repeated source, a repeated target, or a target that is also a source
 * (repair never copies a block the caller already holds).  ntargets == 0 is valid and writes
 * nothing. */
int sec_repair_matrix(int k, int m, const int32_t *sharenums, const int32_t *targets, int ntargets,
                      uint8_t *out);

/* One chunk to repair.  Its k source blocks are entries slot0 .. slot0+k-1 of sharenums[] /
 * block_offs[] / block_avail[] (as sec_dec_chunk's), its lost blocks entries tgt0 ..
 * tgt0+ntargets-1 of target_nums[] / target_offs[]. */
typedef struct sec_rep_chunk {
    uint64_t B;      /* block bytes                                                     */
    uint64_t slot0;  /* first of the chunk's k entries in sharenums[] / block_offs[] /
                        block_avail[]                                                   */
    uint64_t tgt0;   /* first of its ntargets entries in target_nums[] / target_offs[]  */
    int32_t ntargets;
    int32_t k;
    int32_t m;
    int32_t pad;
} sec_rep_chunk; /* 40 bytes */

/* For every chunk, block target_nums[tgt0 + j] is written at out + target_offs[tgt0 + j], all B
 * bytes of it (for data block k-1 too: zfec's zero padding is part of the piece), in the caller's
 * target order, from the k blocks at blocks + block_offs[slot0 + i] numbered sharenums[slot0 + i].
 * Every target is its own buffer at any byte alignment.  `blocks` or `out` may be NULL: the
 * offsets are then absolute addresses.  block_avail (nullable) as in sec_decode_batch_ex: that
 * many bytes of a source exist, the rest read as zero, and nothing past them is read.
 * digests (nullable): 20 bytes per target at digests + 20 (tgt0 + j), the SHA-1 of the repaired
 * piece (storb's piece id), computed by the SHA-1 kernel while the targets are device-resident;
 * digests live where the targets do (device memory, or host memory with SEC_F_HOST).
 * More than 8 targets of a chunk take ceil(ntargets / 8) passes over its sources on the direct
 * (v_perm) kernels; a chunk whose k sources are its data blocks (every target is then a parity row)
 * may take the bit-sliced repair kernel instead, one pass per 16-row group that holds a target,
 * whatever ntargets (sec_repair_method, option "SEC_CHECK_BS"; one call may hold both kinds).  The
 * bytes written are the same.
 * Aliasing: no target range may overlap a source block or another target of any chunk in the
 * call: workgroups read sources while others write targets, so an overlap gives unspecified
 * bytes.  The library does not check this (sec_decode_batch's rule).
 * Flags: none (device pointers; SEC_F_ASYNC allowed) or SEC_F_HOST (host pointers; SEC_F_ASYNC
 * is then SEC_EINVAL); any other flag is SEC_EINVAL.  SEC_F_HOST is ALWAYS staged: the sources
 * are gathered into pinned slabs and the targets and digests scattered back from them.  Unlike
 * the encode / decode host paths it never page-locks a caller's buffer for the call and never
 * runs the kernels on caller memory in place, pinned or not; sec_ctx_host_paths counts every
 * such call as staged.
 * Errors: sec_repair_matrix's per chunk, SEC_ESIZE for B >= 2^31. */
int sec_repair_batch(sec_ctx *ctx, const sec_rep_chunk *chunks, int64_t nchunks,
                     const int32_t *sharenums, const uint64_t *block_offs,
                     const uint64_t *block_avail, const uint8_t *blocks,
                     const int32_t *target_nums, const uint64_t *target_offs, uint8_t *out,
                     uint8_t *digests, unsigned flags);

/* ---- check: do the held pieces of a chunk agree with each other ---------------------------
 * A Reed-Solomon code word carries its own check: of the n > k blocks a caller holds, each one
 * past any k of them is a fixed GF(2^8) combination of those k (a row of sec_repair_matrix).  The
 * check predicts every such extra block from k basis blocks and compares it with what is stored:
 * any corruption confined to at most n - k of the n blocks is detected with certainty, n*B bytes
 * are read and nothing is written but the results.  No zfec counterpart. */
typedef struct sec_chk_chunk {
    uint64_t B;      /* block bytes                                                     */
    uint64_t slot0;  /* first of the chunk's n entries in sharenums[] / block_offs[] /
                        block_avail[]                                                   */
    int32_t n;       /* blocks held, k <= n <= m                                        */
    int32_t k;
    int32_t m;
    int32_t pad;
} sec_chk_chunk; /* 32 bytes */

typedef struct sec_chk_result {
    uint64_t first;  /* lowest byte position at which a check row disagrees with its
                        prediction; UINT64_MAX: the chunk is consistent                 */
    uint32_t nbad;   /* check rows that disagree anywhere in the chunk                  */
    uint32_t pad;
} sec_chk_result; /* 16 bytes */

/* Entries slot0 .. slot0+k-1 of a chunk are its basis (any order; normalised as repair's sources
 * are), entries slot0+k .. slot0+n-1 its check rows.  Each check row's block as predicted from the
 * basis is compared with the stored block over all B bytes.
 * results[c] (8-byte aligned): `first` and `nbad` of chunk c.
 * row_bad (nullable): one byte per slot entry, indexed as sharenums[]: 1 for a check row that
 * disagrees somewhere, 0 for one that agrees and for every basis entry.
 * column (nullable): one byte per slot entry; for an inconsistent chunk the byte of each of its n
 * entries at position `first` (zero for a position past the entry's avail): the input of
 * sec_check_locate.  Untouched for a consistent chunk.
 * block_avail (nullable) as in sec_repair_batch, for basis entries and check rows alike: that many
 * bytes of the block exist, the rest read as zero (so the prediction there must be zero), and
 * nothing past them is read.
 * A chunk with n == k has nothing to check: it is consistent and launches nothing.  More than 8
 * check rows take ceil((n - k) / 8) passes over the basis on the direct (v_perm) kernels; a chunk
 * whose basis is its k data blocks may take the bit-sliced check kernel instead, one pass per
 * 16-row group whatever n - k (sec_check_method, option "SEC_CHECK_BS").  The results are the same.
 * results, row_bad and column live where the blocks live: device memory, or host memory with
 * SEC_F_HOST.  Nothing is ever written to the blocks.  Every call starts from clean state.
 * Flags: none (device pointers; SEC_F_ASYNC allowed) or SEC_F_HOST (host pointers, always staged
 * through pinned slabs as sec_repair_batch's: n*B bytes per chunk gathered, only the results
 * scattered back; SEC_F_ASYNC is then SEC_EINVAL); any other flag is SEC_EINVAL.
 * Errors, all before any device work, in this order: SEC_EINVAL a NULL array, NULL results or
 * n < 0; SEC_EKM; SEC_ENBLOCKS n < k or n > m; SEC_ESHARENUM; SEC_EDUPSHARE any repeat among the
 * n sharenums; SEC_ESIZE B >= 2^31. */
int sec_check_batch(sec_ctx *ctx, const sec_chk_chunk *chunks, int64_t nchunks,
                    const int32_t *sharenums, const uint64_t *block_offs,
                    const uint64_t *block_avail, const uint8_t *blocks, sec_chk_result *results,
                    uint8_t *row_bad, uint8_t *column, unsigned flags);

/* ---- decode + check: reassemble from k held pieces and check the spare ones in one pass -------
 * A caller holding n > k blocks of a chunk (storb's validator fetches all m) gets the chunk's
 * bytes and the code word's verdict from one read of the n blocks: n*B bytes read and k*B written,
 * where sec_check_batch followed by sec_decode_batch_ex reads the k chosen blocks twice.  The
 * contract is the COMPOSITION of those two calls on the same arrays:
 *   - `out` receives exactly what sec_decode_batch_ex writes for entries slot0 .. slot0+k-1
 *     (present primaries copied, missing ones recovered; k*B - padlen bytes at out + out_off and
 *     nothing past them); with SEC_F_RECOVER only the e recovered rows, as that flag specifies.
 *     `out` is written whether or not the chunk turns out consistent.
 *   - results, row_bad (nullable) and column (nullable) receive exactly what sec_check_batch
 *     reports for entries slot0 .. slot0+n-1: the first k are the basis, the rest the check rows.
 * The first k entries may be any k distinct blocks in any order.  block_avail (nullable) has the
 * meaning both calls give it, for basis entries and check rows alike.  A chunk with n == k is a
 * plain decode and is reported consistent.  `blocks` may be NULL (absolute block_offs).  Nothing is
 * ever written to the blocks; every call starts from clean state.  A chunk that lost a
 * primary always takes the direct (v_perm) kernels, never the syndrome path; one whose first k
 * entries are its k data blocks may take the bit-sliced check kernel, which copies them to `out`
 * while it checks (sec_check_method, option "SEC_CHECK_BS"; one call may hold both kinds).
 * sec_ctx_decode_paths and sec_ctx_decode_methods do not count this call (sec_ctx_check_methods
 * does), and sec_ctx_host_paths counts a SEC_F_HOST call as staged (as sec_check_batch's).
 * Aliasing: sec_decode_batch's rule (no output range may overlap any block of the call).
 * Flags: none or SEC_F_ASYNC (device pointers); SEC_F_RECOVER in either mode; SEC_F_HOST (host
 * pointers) is ALWAYS staged through pinned slabs as sec_check_batch's: n*B bytes per chunk are
 * gathered ONCE, and the output (with SEC_F_RECOVER only the recovered rows) and the results are
 * scattered back.  SEC_F_HOST with SEC_F_ASYNC is SEC_EINVAL; any other flag is SEC_EINVAL.
 * Errors, all before any device work, in this order: SEC_EINVAL a NULL array, NULL results, NULL
 * `out` where a chunk has bytes to write, or n < 0; SEC_EKM; SEC_ENBLOCKS n < k or n > m;
 * SEC_ESHARENUM; SEC_EDUPSHARE any repeat among the n sharenums; SEC_EPADLEN padlen > k*B;
 * SEC_ESIZE B >= 2^31.
 * sec_timing_collect kind 6 times this call's kernels. */
typedef struct sec_dchk_chunk {
    uint64_t out_off; /* as sec_dec_chunk                                                */
    uint64_t B;
    uint64_t padlen;
    uint64_t slot0;   /* first of the chunk's n entries in sharenums[] / block_offs[] /
                         block_avail[]                                                   */
    int32_t n;        /* blocks held, k <= n <= m                                        */
    int32_t k;
    int32_t m;
    int32_t pad;
} sec_dchk_chunk; /* 48 bytes */

int sec_decode_check_batch(sec_ctx *ctx, const sec_dchk_chunk *chunks, int64_t nchunks,
                           const int32_t *sharenums, const uint64_t *block_offs,
                           const uint64_t *block_avail, const uint8_t *blocks, uint8_t *out,
                           sec_chk_result *results, uint8_t *row_bad, uint8_t *column,
                           unsigned flags);

/* ---- decode + correct: reassemble, and put right one wrong entry per byte position -------------
 * sec_decode_check_batch detects a corrupt piece; taking it out means dropping the whole piece and
 * checking again, which gives up once two pieces are damaged and n - k = 2, even when their damage
 * lies at different offsets.  This call corrects per byte position instead.  Chunks, entries, basis
 * and block_avail mean what they mean for sec_decode_check_batch: the first k entries are the basis
 * in any order, the rest check rows, bytes past an entry's avail read as zero and nothing past them
 * is read.  For every position p in [0, B) the n bytes at p are a column, and the call does to it
 * exactly what sec_check_locate says of it:
 *   -1, a code word        nothing to correct;
 *   a check-row entry      counted as corrected; the output is unaffected;
 *   a basis entry          that entry's byte is replaced by the one value that makes the column a
 *                          code word; counted as corrected;
 *   -2 (every bad position when n - k < 2)   open: left as held.
 * `out` receives what sec_decode_batch_ex would write from the basis AFTER those replacements:
 * k*B - padlen bytes at out + out_off and nothing past them.  At open positions it holds the decode
 * of the basis as held, the bytes sec_decode_check_batch writes there.  results[c] (8-byte aligned)
 * is chunk c's sec_cor_result.  entry_hits (nullable) has one uint32_t per entry, in the caller's
 * order: the positions at which that entry was the one changed; every entry of the call is
 * written, zero included.  Nothing is ever written to the blocks; every call starts from clean
 * state.  A chunk with n == k is a plain decode and is reported consistent.
 * What it promises.  The code has distance n - k + 1.  With n - k >= 2 a position where at most
 * one held byte is wrong is always put right.  With n - k >= 3 a position where two are wrong is
 * always reported open.  With n - k = 2 a position where two are wrong may be attributed to a
 * third entry (two errors are never a code word, but can look like one error elsewhere).
 * The call always takes its own kernel (sec_decode_correct_kernel): there is no bit-sliced form,
 * and sec_ctx_check_methods, sec_ctx_decode_paths and sec_ctx_decode_methods do not count it;
 * sec_ctx_host_paths counts a SEC_F_HOST call as staged.
 * Aliasing: sec_decode_batch's rule (no output range may overlap any block of the call).
 * Flags: none or SEC_F_ASYNC (device pointers); SEC_F_HOST (host pointers) is ALWAYS staged
 * through pinned slabs as sec_decode_check_batch's: n*B bytes per chunk are gathered ONCE, and the
 * output, the results and the hits are scattered back.  SEC_F_HOST with SEC_F_ASYNC,
 * SEC_F_RECOVER and any other flag are SEC_EINVAL.
 * Errors, all before any device work, in sec_decode_check_batch's order: SEC_EINVAL a NULL array,
 * NULL results, NULL `out` where a chunk has bytes to write, n < 0 or a NULL context; SEC_EKM;
 * SEC_ENBLOCKS; SEC_ESHARENUM; SEC_EDUPSHARE; SEC_EPADLEN; SEC_ESIZE.
 * sec_timing_collect kind 8 times this call's kernels. */
typedef struct sec_cor_result {
    uint64_t first;      /* lowest position whose held bytes are no code word; UINT64_MAX: consistent */
    uint64_t first_open; /* lowest position that no single-entry change explains; UINT64_MAX: none    */
    uint32_t corrected;  /* positions where one entry was changed to reach a code word                */
    uint32_t open;       /* positions that are no code word and were left as held                     */
} sec_cor_result; /* 24 bytes */

int sec_decode_correct_batch(sec_ctx *ctx, const sec_dchk_chunk *chunks, int64_t nchunks,
                             const int32_t *sharenums, const uint64_t *block_offs,
                             const uint64_t *block_avail, const uint8_t *blocks, uint8_t *out,
                             sec_cor_result *results, uint32_t *entry_hits, unsigned flags);

/* ---- repair + check: regenerate lost pieces and check the spare ones in one pass ---------------
 * A repair runs because a miner is gone, and the caller usually still reaches more than k of the
 * chunk's pieces.  This call regenerates the lost pieces from k of them and checks the spare ones
 * against the same k from one read of the n blocks: n*B bytes read and ntargets*B written, where
 * sec_check_batch followed by sec_repair_batch reads the k basis blocks twice.  The contract is the
 * COMPOSITION of those two calls on the same arrays:
 *   - the targets and `digests` (nullable) receive exactly what sec_repair_batch writes for entries
 *     slot0 .. slot0+k-1 as sources: block target_nums[tgt0 + j] whole at out + target_offs[tgt0 + j],
 *     all B bytes (for data block k-1 too, zero padding included), in the caller's target order, each
 *     at its own address and any byte alignment; 20 digest bytes per target at digests + 20 (tgt0 + j),
 *     from the SHA-1 kernel while the targets are device-resident.  The targets are written whether
 *     or not the chunk turns out consistent.
 *   - results, row_bad (nullable) and column (nullable) receive exactly what sec_check_batch
 *     reports for entries slot0 .. slot0+n-1: the first k are the basis, the rest the check rows.
 * The first k entries may be any k distinct blocks in any order.  block_avail (nullable) has the
 * meaning both calls give it, for basis entries and check rows alike; nothing past an entry's avail
 * is read.  A chunk with ntargets == 0 is a plain check, one with n == k a plain repair, reported
 * consistent; with both it launches nothing.  `blocks` or `out` may be NULL: the offsets are then
 * absolute addresses.  Nothing is ever written to the blocks; every call starts from clean state.
 * More than 8 rows (targets + check rows) of a chunk take ceil((ntargets + n - k) / 8) row groups
 * over its basis on the direct (v_perm) kernels; a chunk with a target whose first k entries are
 * its k data blocks may take the bit-sliced repair kernel instead, one pass per 16-row group with a
 * target or a check row (sec_repair_method, option "SEC_CHECK_BS"; one call may hold both kinds).
 * Targets and results are the same.  A chunk with no target always takes the direct kernels.
 * Aliasing: sec_repair_batch's rule (no target range may overlap a block or another target of the
 * call).
 * Flags: none or SEC_F_ASYNC (device pointers); SEC_F_HOST (host pointers) is ALWAYS staged through
 * pinned slabs as sec_check_batch's: the n*B bytes of a chunk are gathered ONCE, and the targets,
 * digests and results are scattered back; sec_ctx_host_paths counts the call as staged.
 * SEC_F_HOST with SEC_F_ASYNC is SEC_EINVAL; any other flag is SEC_EINVAL.
 * Errors, all before any device work, in this order: SEC_EINVAL a NULL array, NULL results, n < 0
 * or ntargets < 0; SEC_EKM; SEC_ENBLOCKS n < k or n > m; SEC_ESHARENUM an entry or a target outside
 * [0, m); SEC_EDUPSHARE a repeat among the n entries, a repeated target, or a target that is also
 * one of the n entries; SEC_ESIZE B >= 2^31.
 * sec_timing_collect kind 7 times this call's kernels. */
typedef struct sec_rchk_chunk {
    uint64_t B;      /* block bytes                                                     */
    uint64_t slot0;  /* first of the chunk's n entries in sharenums[] / block_offs[] /
                        block_avail[]                                                   */
    uint64_t tgt0;   /* first of its ntargets entries in target_nums[] / target_offs[]  */
    int32_t ntargets;
    int32_t n;       /* blocks held, k <= n <= m                                        */
    int32_t k;
    int32_t m;
} sec_rchk_chunk; /* 40 bytes */

int sec_repair_check_batch(sec_ctx *ctx, const sec_rchk_chunk *chunks, int64_t nchunks,
                           const int32_t *sharenums, const uint64_t *block_offs,
                           const uint64_t *block_avail, const uint8_t *blocks,
                           const int32_t *target_nums, const uint64_t *target_offs, uint8_t *out,
                           uint8_t *digests, sec_chk_result *results, uint8_t *row_bad,
                           uint8_t *column, unsigned flags);

/* ---- repair + correct: regenerate and heal pieces from the column-corrected code word ----------
 * A repair's output is seeded to other miners, so a damaged survivor that gets through becomes
 * permanent.  sec_repair_check_batch names one corrupt piece and the caller drops it whole, which
 * gives up once two pieces are damaged and n - k = 2, even at different offsets.  This call corrects
 * per byte position, as sec_decode_correct_batch does, and gives PIECES back.  The contract is the
 * COMPOSITION of two existing ones:
 *   - chunks (sec_rchk_chunk), entries, basis and block_avail mean what they mean for
 *     sec_repair_check_batch: the first k entries, in any order, are the basis, the rest check rows;
 *     bytes past an entry's avail read as zero and nothing past them is read.
 *   - for every position p in [0, B) the n held bytes are a column, judged exactly as
 *     sec_decode_correct_batch / sec_check_locate judge it: a code word; a check-row entry wrong
 *     (counted); a basis entry wrong (replaced by the one value that makes the column a code word,
 *     counted); open (left as held: every bad position when n - k < 2).
 * Targets.  Target j of chunk c is block target_nums[tgt0 + j], written whole at
 * out + target_offs[tgt0 + j]: B bytes at any byte alignment, in the caller's order, data block k-1
 * with its zero padding.  One rule defines its bytes:
 *     byte p = (row target_nums[tgt0 + j] of the repair matrix over the basis)
 *              . (the basis column at p after the replacement above).
 * A target MAY be one of the n held entries (a heal target), so
 *   - a lost block is regenerated;
 *   - a held basis entry comes back as held, with its byte replaced wherever it was the entry
 *     changed;
 *   - a held check-row entry comes back as the prediction from the corrected basis: its held byte
 *     wherever the column is a code word or a basis entry was changed, the corrected byte where
 *     that row was the entry changed;
 *   - at OPEN positions every target is what the basis as held predicts, which for a held check
 *     row may differ from the byte it holds there.
 * Targets are distinct among themselves.  digests (nullable): 20 bytes per target at
 * digests + 20 (tgt0 + j), the SHA-1 of the target as written, from the SHA-1 kernel while the
 * targets are device-resident, as sec_repair_batch's.  results[c] (8-byte aligned) is chunk c's
 * sec_cor_result; entry_hits (nullable) has one uint32_t per entry of the call in the caller's
 * order, zero included, exactly sec_decode_correct_batch's.  What the verdicts promise is stated
 * there (the code has distance n - k + 1; with n - k = 2 two wrong bytes at one position may be
 * attributed to a third entry).
 * A chunk with n == k is a plain repair, reported consistent (a heal target is then a copy); one
 * with ntargets == 0 judges and counts and writes no block (`out` may then be NULL).  Nothing is
 * ever written to the blocks; every call starts from clean state.
 * Aliasing: sec_repair_batch's rule (no target range may overlap a block or another target of the
 * call): healing is never in place.
 * The call always takes its own kernels (sec_repair_correct_kernel): there is no bit-sliced form,
 * and sec_ctx_check_methods, sec_ctx_repair_methods, sec_ctx_decode_paths and
 * sec_ctx_decode_methods do not count it.
 * Flags: none or SEC_F_ASYNC (device pointers); SEC_F_HOST (host pointers) is ALWAYS staged through
 * pinned slabs: the n*B bytes of a chunk are gathered ONCE, and the targets, digests, results and
 * hits are scattered back; sec_ctx_host_paths counts the call as staged.  SEC_F_HOST with
 * SEC_F_ASYNC and every other flag are SEC_EINVAL.
 * Errors, all before any device work, in sec_repair_check_batch's order: SEC_EINVAL a NULL array,
 * NULL results, a NULL context, n < 0, ntargets < 0 or targets without their arrays; SEC_EKM;
 * SEC_ENBLOCKS n < k or n > m; SEC_ESHARENUM an entry or a target outside [0, m); SEC_EDUPSHARE a
 * repeat among the n entries or a repeated target (a target that is an entry is NOT an error
 * here); SEC_ESIZE B >= 2^31.
 * sec_timing_collect kind 8 times this call's kernels and, with digests, their SHA-1. */
int sec_repair_correct_batch(sec_ctx *ctx, const sec_rchk_chunk *chunks, int64_t nchunks,
                             const int32_t *sharenums, const uint64_t *block_offs,
                             const uint64_t *block_avail, const uint8_t *blocks,
                             const int32_t *target_nums, const uint64_t *target_offs, uint8_t *out,
                             uint8_t *digests, sec_cor_result *results, uint32_t *entry_hits,
                             unsigned flags);

/* Which single entry explains an inconsistent column (host arithmetic, no device needed).
 * sharenums: the n block numbers, the first k the basis; column: the n bytes sec_check_batch
 * returned.  *culprit = -1: the column is a code word; i in [0, n): changing entry i alone makes
 * it one; -2: inconsistent and no single entry explains it, which is also the answer whenever
 * n - k < 2 (one check row cannot tell itself from the basis).  The code is MDS, so with two or
 * more check rows a single-entry explanation is unique; it names the corrupt piece only if one
 * piece is corrupt at that position.
 * Errors: sec_repair_matrix's for (k, m, sharenums[0..k), sharenums[k..n), n - k); SEC_EINVAL
 * also for a NULL column or culprit. */
int sec_check_locate(int k, int m, const int32_t *sharenums, int n, const uint8_t *column,
                     int32_t *culprit);

/* ---- decode + correct and repair + correct, several errors per byte position -------------------
 * sec_decode_correct_batch and sec_repair_correct_batch put right ONE wrong entry per position,
 * whatever n - k is.  The n held blocks of a chunk are a Reed-Solomon code of distance r + 1,
 * r = n - k, which carries floor(r / 2) errors per position; these two calls use it.  They take the
 * arguments of their namesakes, with the same meaning, and max_errors behind them.  The bound is
 *     t = min(T, floor(r / 2), 16),  T = max_errors, or no limit when max_errors == 0,
 * and a position whose column is no code word is
 *   corrected  when some code word differs from the column in at most t entries.  That word is
 *              unique (2t <= r).  Every differing entry counts one hit in entry_hits, the position
 *              counts once in `corrected`, and every output byte there is computed from the
 *              corrected column (a repair target: its row of the repair matrix times the corrected
 *              basis column, every changed basis entry applied);
 *   open       when no such code word exists: the column is left as held, counted in `open`, and the
 *              outputs there are what the basis as held gives.
 * sec_cor_result, first, first_open and entry_hits keep their layout and meaning, "the entry
 * changed" read as "an entry changed".  What this promises:
 *   - at most t wrong bytes at a position are always put right;
 *   - more than t and at most r - t wrong bytes are always reported open;
 *   - beyond r - t the column may lie within t of ANOTHER code word and is then corrected to that
 *     one: only the piece ids the caller recorded exclude it;
 *   - with max_errors == 1 results, hits and every output byte equal sec_decode_correct_batch's /
 *     sec_repair_correct_batch's exactly, for every r.
 * Heal targets, digests, flags, staging, aliasing, timing (kind 8; sec_ctx_*_methods count none of
 * it) and the errors with their order are the namesakes'; max_errors < 0 is SEC_EINVAL, reported
 * with the other SEC_EINVALs, before SEC_EKM.  The kernels are sec_decode_correct_ex_kernel and
 * sec_repair_correct_ex_kernel: clean lanes decode or repair as vectors exactly as the namesakes'
 * do; only a lane with a nonzero check delta runs, per position, a bounded-distance decoder
 * (syndromes from the check deltas, Berlekamp-Massey in exactly 2t steps, a root search over the n
 * held points, the error values, and the check rows once more on the changed column). */
int sec_decode_correct_ex_batch(sec_ctx *ctx, const sec_dchk_chunk *chunks, int64_t nchunks,
                                const int32_t *sharenums, const uint64_t *block_offs,
                                const uint64_t *block_avail, const uint8_t *blocks, uint8_t *out,
                                sec_cor_result *results, uint32_t *entry_hits, int max_errors,
                                unsigned flags);

int sec_repair_correct_ex_batch(sec_ctx *ctx, const sec_rchk_chunk *chunks, int64_t nchunks,
                                const int32_t *sharenums, const uint64_t *block_offs,
                                const uint64_t *block_avail, const uint8_t *blocks,
                                const int32_t *target_nums, const uint64_t *target_offs,
                                uint8_t *out, uint8_t *digests, sec_cor_result *results,
                                uint32_t *entry_hits, int max_errors, unsigned flags);

/* The one-column model of that contract (host arithmetic, no device needed), beside
 * sec_check_locate.  sharenums: the n block numbers, the first k the basis; column: the n held
 * bytes of one position.  fixed receives the n corrected bytes; *nchanged = 0: the column is a code
 * word; 1 .. t: that many entries were changed to reach the one code word within t; -2: open
 * (fixed = column).  t as above; with max_errors == 1 the verdict is sec_check_locate's.
 * Errors: sec_check_locate's; SEC_EINVAL also for max_errors < 0 or a NULL fixed or nchanged. */
int sec_check_correct(int k, int m, const int32_t *sharenums, int n, const uint8_t *column,
                      int max_errors, uint8_t *fixed, int32_t *nchanged);

/* Whether a chunk of sec_check_batch / sec_decode_check_batch is eligible for the bit-sliced check
 * kernel (host logic, no device needed): *method = 1 when (k, m) is one of the bit-sliced shapes
 * ((10,14), (8,12), (16,24), (32,48), (64,96), (8,11)), B >= 16, n > k, the first k sharenums are
 * the data blocks 0 .. k-1 in any order, every entry but data block k-1 is readable to B
 * (block_avail: the chunk's n entries, nullable = all B) and padlen < B (0 for a check); else 0.
 * Eligibility alone: whether an eligible chunk takes that kernel is option "SEC_CHECK_BS" (-1 the
 * measured rule, 0 never, 1 always).  The same option governs the bit-sliced repair kernel of
 * sec_repair_batch / sec_repair_check_batch (sec_repair_method), whose measured rule is a rule of
 * its own.
 * Errors: sec_check_batch's for the same arguments, in its order (SEC_EINVAL also for a NULL
 * method or padlen < 0). */
int sec_check_method(int k, int m, const int32_t *sharenums, int n, uint64_t B,
                     const uint64_t *block_avail, int64_t padlen, int *method);

/* Chunks with at least one check row that sec_check_batch and sec_decode_check_batch have sent to
 * the bit-sliced check kernel and to the direct kernels on this context (cumulative; either
 * pointer nullable). */
int sec_ctx_check_methods(sec_ctx *ctx, int64_t *bitsliced, int64_t *direct);

/* Whether a chunk of sec_repair_batch (n == k) / sec_repair_check_batch is eligible for the
 * bit-sliced repair kernel (host logic, no device needed): *method = 1 when (k, m) is one of the
 * bit-sliced shapes (sec_check_method's), B >= 16, the chunk has a target or a check row
 * (ntargets + n - k >= 1), the first k sharenums are the data blocks 0 .. k-1 in any order (so every
 * target is a parity row) and every entry but data block k-1 is readable to B (block_avail: the
 * chunk's n entries, nullable = all B); else 0.
 * Eligibility alone: whether an eligible chunk takes that kernel is option "SEC_CHECK_BS", and a
 * chunk with no target never does.
 * Errors: sec_repair_check_batch's for the same arguments, in its order (SEC_EINVAL also for a NULL
 * method). */
int sec_repair_method(int k, int m, const int32_t *sharenums, int n, const int32_t *targets,
                      int ntargets, uint64_t B, const uint64_t *block_avail, int *method);

/* Chunks with at least one target that sec_repair_batch and sec_repair_check_batch have sent to the
 * bit-sliced repair kernel and to the direct kernels on this context (cumulative; either pointer
 * nullable).  sec_ctx_check_methods does not count these calls. */
int sec_ctx_repair_methods(sec_ctx *ctx, int64_t *bitsliced, int64_t *direct);

/* ---- piece ids: SHA-1 (piece_hash, /root/reference/storb/util/piece.py:54-68) ----
 * A message is `len` bytes at `addr`, of which the first `avail` exist in
 * memory and the rest read as zero (so zfec's zero-padded last data block can
 * be hashed in place).  digests: 20 bytes per message, in order.
 * Device mode: addr / digests are device memory.  SEC_F_HOST: both are host
 * memory (messages are staged through pinned slabs).                        */
typedef struct sec_msg {
    uint64_t addr;
    uint64_t len;
    uint64_t avail;
} sec_msg;

int sec_sha1_batch(sec_ctx *ctx, const sec_msg *msgs, int64_t nmsgs, uint8_t *digests, unsigned flags);

/* Encode + the SHA-1 of every one of the chunk's m blocks (the piece ids the
 * validator computes right after encode, validator.py:1081), while data and
 * parity are still on the device.  Block j of chunk c gets digest slot
 * M_c + j with M_c = sum of m over chunks before c; digests (20 B per slot)
 * live where the parity does (device, or host with SEC_F_HOST). */
int sec_encode_digest_batch(sec_ctx *ctx, const sec_enc_chunk *chunks, int64_t nchunks,
                            const uint8_t *in, uint8_t *parity, uint8_t *digests, unsigned flags);

/* ---- pieces: easyfec's Encoder.encode output in the caller's piece buffers -------------------
 * Replaces zfec.easyfec.Encoder(k, m).encode(chunk) at /root/reference/storb/util/piece.py:
 * 129-130 (k slices copied out of the chunk, the last zero-padded, then the m - k parity
 * blocks), writing every one of chunk c's m pieces to its own host buffer pieces[M_c + j]
 * (B = ceil(n / k) bytes each; M_c = sum of m over chunks before c), and, when digests is not
 * NULL, each piece's SHA-1 (20 bytes at digests + 20 (M_c + j): storb's piece id,
 * hashlib.sha1(piece), piece.py:54-68 / validator.py:1081).  Host memory only (SEC_F_HOST
 * required; SEC_F_STAGED as for sec_encode_batch); chunks[c].parity_off / parity_stride are
 * ignored (the parity goes through a context-owned pinned scratch).  The data pieces are copied
 * and hashed on the context's host threads while the calling thread runs the GPU encode, the
 * parity pieces right after it; the call returns when every piece and digest is written.
 * Preconditions and errors as sec_encode_batch; SEC_EINVAL for a NULL piece buffer of a
 * non-empty chunk.  Flags: SEC_F_HOST (required), SEC_F_STAGED, SEC_F_GPU_PARITY_IDS. */
int sec_encode_pieces(sec_ctx *ctx, const sec_enc_chunk *chunks, int64_t nchunks, const uint8_t *in,
                      uint8_t *const *pieces, uint8_t *digests, unsigned flags);

/* ---- APDP proofs of data possession: 2048-bit modular arithmetic ----------
 * Replaces the gmpy2 calls of storb's ChallengeSystem
 * (/root/reference/storb/challenge/__init__.py:304-350 generate_tag,
 * :401-463 generate_proof, :465-528 verify_proof; gmpy2 2.2.1,
 * /root/reference/uv.lock).  Integers cross the boundary as 256-byte big-endian
 * strings (int.to_bytes(256, "big")).  The modulus is an RSA-2048 modulus:
 * odd, exactly 2048 bits (DEFAULT_RSA_KEY_SIZE, storb/constants.py:26);
 * anything else is SEC_EMODULUS.  Results are fully reduced (< n).
 * Device mode: every data pointer is device memory; SEC_F_HOST: host memory. */
typedef struct sec_bn_key sec_bn_key;

int sec_bn_key_create(sec_ctx *ctx, const uint8_t n_be[256], sec_bn_key **out);
void sec_bn_key_destroy(sec_bn_key *key);
/* The key owner's factors (the validator's RSA key): n = p*q with p, q odd and exactly
 * 1024 bits (128 B big-endian each), cp = q*(q^-1 mod p) and cq = p*(p^-1 mod q) (256 B,
 * mod n).  Enables sec_bn_crt_modexp_batch and CRT tags.  The caller guarantees
 * n = p*q; p or q not odd 1024-bit integers give SEC_EMODULUS. */
int sec_bn_key_set_crt(sec_ctx *ctx, sec_bn_key *key, const uint8_t p_be[128], const uint8_t q_be[128],
                       const uint8_t cp_be[256], const uint8_t cq_be[256]);
/* generate_tag's per-key constants: g, fdh = full_domain_hash(prf(prf_key, 0)) (each taken
 * mod n) and the private exponent d (< 2^2048), 256 B each.  dp, dq (128 B each, or both
 * NULL): exponents for p and q congruent to d mod p-1 and q-1, nonzero when d is (e.g.
 * (d-1) mod (p-1) + 1); given with a CRT key, tags run as two 1024-bit halves.  Builds the
 * key's 16 MiB fixed-base table of g (sec_apdp_gpow_batch, tags).  Host memory. */
int sec_bn_key_set_tag(sec_ctx *ctx, sec_bn_key *key, const uint8_t g_be[256], const uint8_t fdh_be[256],
                       const uint8_t d_be[256], const uint8_t *dp_be, const uint8_t *dq_be);

/* out[i] = int.from_bytes(message i, "big") mod n (256 B each); messages as in
 * sec_sha1_batch (bytes past `avail` read as zero).  block_int of
 * generate_tag / generate_proof. */
int sec_bn_reduce_batch(sec_ctx *ctx, const sec_bn_key *key, const sec_msg *msgs, int64_t nmsgs,
                        uint8_t *out, unsigned flags);
/* out[i] = bases[i] ^ exps[i] mod n.  bases: 256 B each (any value < 2^2048);
 * exps: exp_bytes each, big-endian (1 <= exp_bytes <= 4096). */
int sec_bn_modexp_batch(sec_ctx *ctx, const sec_bn_key *key, const uint8_t *bases,
                        const uint8_t *exps, uint32_t exp_bytes, int64_t count, uint8_t *out,
                        unsigned flags);
/* out[i] = bases[i] ^ e[i] mod n by CRT, given exps_p[i] / exps_q[i] (exp_bytes each,
 * big-endian, 1 <= exp_bytes <= 4096) congruent to e[i] mod p-1 / q-1 and nonzero when
 * e[i] is (e.g. (e-1) mod (p-1) + 1): exact for every base, including multiples of p or
 * q.  Needs sec_bn_key_set_crt. */
int sec_bn_crt_modexp_batch(sec_ctx *ctx, const sec_bn_key *key, const uint8_t *bases,
                            const uint8_t *exps_p, const uint8_t *exps_q, uint32_t exp_bytes,
                            int64_t count, uint8_t *out, unsigned flags);
/* out[i] = g ^ exps[i] mod n from the fixed-base table (issue_challenge's g_s,
 * challenge/__init__.py:387); exps: exp_bytes each, 1 <= exp_bytes <= 256.  Needs
 * sec_bn_key_set_tag. */
int sec_apdp_gpow_batch(sec_ctx *ctx, const sec_bn_key *key, const uint8_t *exps, uint32_t exp_bytes,
                        int64_t count, uint8_t *out, unsigned flags);
/* out[i] = a[i] * b[i] mod n (256 B each, any values < 2^2048). */
int sec_bn_mulmod_batch(sec_ctx *ctx, const sec_bn_key *key, const uint8_t *a, const uint8_t *b,
                        int64_t count, uint8_t *out, unsigned flags);
/* APDP tags, fused per message: X = message mod n; tag = (fdh * g^X)^d mod n
 * (generate_tag's tag_value), g^X from the fixed-base table, the d power by CRT when
 * the key has it.  Needs sec_bn_key_set_tag; 256 B per tag. */
int sec_apdp_tag_batch(sec_ctx *ctx, const sec_bn_key *key, const sec_msg *msgs, int64_t nmsgs,
                       uint8_t *tags, unsigned flags);

/* ---- the challenge round: prove (miner) and verify (validator), one call each ----------
 * Flags of the first two calls: none or SEC_F_ASYNC (device pointers), or SEC_F_HOST (host
 * pointers).  Errors of all three, before any device work and in this order: SEC_EINVAL for a
 * NULL ctx, key or (with a non-zero count) data pointer, a count < 0, any other flag,
 * SEC_F_HOST | SEC_F_ASYNC, or a key of another device; SEC_ENOCRT (sec_bn_crt_modexp2_batch,
 * sec_apdp_verify_batch) for a key without sec_bn_key_set_crt; SEC_EINVAL for exp_bytes outside
 * 1..4096.  A count of 0 then succeeds and touches nothing.  Timing: kind 3, as every bignum
 * kernel. */
/* out[i] = a[i]^ea[i] * b[i]^eb[i] mod n by CRT: one simultaneous two-base exponentiation per
 * factor.  a, b: 256 B each (any values < 2^2048); ea_p / ea_q and eb_p / eb_q: exp_bytes each,
 * big-endian, congruent to ea[i] (eb[i]) mod p-1 / q-1 and nonzero when it is, as
 * sec_bn_crt_modexp_batch's: exact for every base.  A negative power of a base invertible mod
 * n is the exponent (-e) mod (p-1) / (q-1).  Needs sec_bn_key_set_crt. */
int sec_bn_crt_modexp2_batch(sec_ctx *ctx, const sec_bn_key *key, const uint8_t *a, const uint8_t *b,
                             const uint8_t *ea_p, const uint8_t *ea_q, const uint8_t *eb_p,
                             const uint8_t *eb_q, uint32_t exp_bytes, int64_t count, uint8_t *out,
                             unsigned flags);
/* generate_proof (challenge/__init__.py:401-463) per message, X = message mod n (messages as
 * in sec_bn_reduce_batch), T = tags[i], g_s = g_ss[i] (256 B each, any values < 2^2048),
 * c = coefs[i] (32 B big-endian: prf(challenge key, 0)):
 *   tag_c[i] = T^c mod n (256 B), block[i] = c * X (288 B big-endian, the plain product),
 *   rho[i] = g_s^(c * X) mod n (256 B).
 * Needs the modulus only (the miner's side): no CRT factors, no tag constants.  SEC_F_HOST
 * stages the messages through pinned slabs as sec_apdp_tag_batch does. */
int sec_apdp_prove_batch(sec_ctx *ctx, const sec_bn_key *key, const sec_msg *msgs, int64_t nmsgs,
                         const uint8_t *tags, const uint8_t *g_ss, const uint8_t *coefs,
                         uint8_t *tag_c, uint8_t *block, uint8_t *rho, unsigned flags);
/* verify_proof's tau_s (challenge/__init__.py:497-524) per item:
 *   values[i] = (T^e * (F^c)^-1)^s mod n, T = proof_tags[i], F = fdhs[i], s = ss[i] (256 B
 *   each), c = coefs[i] (32 B), e = e_be (the public exponent, 256 B), all big-endian;
 * the caller compares SHA-256 of values[i] (minimal big-endian bytes) with the proof's hash.
 * status[i] = 1 and values[i] = 0 where F^c is not invertible mod n (c != 0 and F a multiple of
 * p or q: gmpy2's powmod(x, -1, n) raises there), else 0.  The library reduces the exponents
 * e*s and -c*s for p-1 and q-1 on its host threads and makes one sec_bn_crt_modexp2 launch.
 * Host memory only: SEC_F_HOST is required, any other flag is SEC_EINVAL.  Needs
 * sec_bn_key_set_crt. */
int sec_apdp_verify_batch(sec_ctx *ctx, const sec_bn_key *key, const uint8_t *proof_tags,
                          const uint8_t *fdhs, const uint8_t *coefs, const uint8_t *ss,
                          const uint8_t e_be[256], int64_t count, uint8_t *values, int32_t *status,
                          unsigned flags);

/* ---- tagged encode: parity, piece ids and APDP tags from one pass over the chunk ----------
 * The upload's three steps per piece (encode, validator.py:1380; SHA-1 id, :1081; APDP tag,
 * process_tag :945-947) while the chunk and its parity are on the device, so a chunk crosses
 * PCIe once.  The composition of the calls it replaces: `parity` gets what sec_encode_batch
 * writes; `digests`, when not NULL, what sec_encode_digest_batch writes; `tags` (256 B
 * big-endian at tags + 256 (M_c + j), the digests' slot numbering) what sec_apdp_tag_batch
 * returns for the chunk's m blocks as messages: data block j with len = B and
 * avail = min(B, n - j B) (the padding zeros are part of the integer, as of the piece), parity
 * block r with len = avail = B.  A chunk with m == k still gets its k tags; one with n == 0
 * gets the tag of the empty message in each of its m slots.
 * Device mode (no flag, or SEC_F_ASYNC): every pointer is device memory.  SEC_F_HOST: host
 * memory, always staged (as digest mode: each chunk gathered once into a slab of
 * SEC_SLAB_BYTES_DIGEST; parity, digests and tags scattered back; counted as staged by
 * sec_ctx_host_paths).  Errors, before any device work and in this order: SEC_EINVAL for a NULL
 * ctx / key / tags, any other flag, SEC_F_HOST | SEC_F_ASYNC, or a key of another device;
 * SEC_ENOTAG for a key without sec_bn_key_set_tag; then sec_encode_batch's per-chunk errors.
 * Timing: the tag kernels under kind 3, the encode and SHA-1 as sec_encode_digest_batch. */
int sec_encode_tag_batch(sec_ctx *ctx, const sec_bn_key *key, const sec_enc_chunk *chunks,
                         int64_t nchunks, const uint8_t *in, uint8_t *parity,
                         uint8_t *digests /* nullable */, uint8_t *tags, unsigned flags);
/* sec_encode_pieces (same flags, host-thread copies and ids) plus each piece's APDP tag: 256 B
 * at tags + 256 (M_c + j), host memory.  The tags come from the GPU call of each sub-batch,
 * which holds the staged chunk and its parity, so no piece crosses PCIe for its tag; a sub-batch
 * is therefore bounded by its staged chunk bytes (twice the bound of its parity, at least one
 * chunk) as well as by its parity, and chunks with m == k take the GPU call too.  key and tags both NULL: sec_encode_pieces
 * itself.  Errors: SEC_EINVAL (NULL ctx, one of key / tags NULL, a bad flag, a key of another
 * device), SEC_ENOTAG, then sec_encode_pieces' own. */
int sec_encode_pieces_tags(sec_ctx *ctx, const sec_bn_key *key, const sec_enc_chunk *chunks,
                           int64_t nchunks, const uint8_t *in, uint8_t *const *pieces,
                           uint8_t *digests /* nullable */, uint8_t *tags, unsigned flags);

/* ---- memory helpers for hosts without a device allocator ----------------- */
int sec_malloc(sec_ctx *ctx, size_t bytes, void **dptr);
int sec_free(sec_ctx *ctx, void *dptr);
int sec_host_alloc(sec_ctx *ctx, size_t bytes, void **hptr); /* pinned */
int sec_host_free(sec_ctx *ctx, void *hptr);                 /* ctx may be NULL */
/* Page-lock an existing host buffer (hipHostRegister) so SEC_F_HOST calls on it take the
 * zero-copy path; unregister (ctx may be NULL) before freeing it. */
int sec_host_register(sec_ctx *ctx, void *hptr, size_t bytes);
int sec_host_unregister(sec_ctx *ctx, void *hptr);
/* SEC_F_HOST encode / decode calls so far on this context: zero-copy on the caller's pinned
 * buffers, zero-copy on pages the call locked itself, and staged. */
int sec_ctx_host_paths(sec_ctx *ctx, int64_t *zero_copy, int64_t *registered, int64_t *staged);
/* Pinned staging memory of the whole process (all contexts): bytes lent to host-mode calls in
 * progress, and idle bytes the library keeps for the next call (at most 512 MiB; the rest is
 * freed).  A context holds none between calls: its slabs and parity scratch are borrowed per
 * call from one process-wide pool.  Either pointer may be NULL. */
int sec_host_pinned_bytes(int64_t *loaned, int64_t *idle);
/* Chunks with a lost data block decoded so far on this context, by method: `syndrome` (the
 * wide-decode path: bit-sliced syndromes of the present parity rows, then the e x e solve) and
 * `direct` (the decode matrix rows over all k blocks).  Which one a chunk takes is the library's
 * choice (cost estimate; context option SEC_SYN = 0 / 1 turns the syndrome path off / forces
 * it where it applies); the bytes are the same. */
int sec_ctx_decode_paths(sec_ctx *ctx, int64_t *syndrome, int64_t *direct);
/* The same chunks by kernel: the one-wave fused syndrome kernel, `pair` (always 0 since round 5:
 * the one-kernel wave pair for parity rows of both groups of zfec(64,96) lost its A/B and is no
 * longer built; the slot stays for ABI stability), the two syndrome kernels (syndromes through
 * device scratch), the direct decode (syndrome = fused + two_kernel). */
int sec_ctx_decode_methods(sec_ctx *ctx, int64_t *fused, int64_t *pair, int64_t *two_kernel, int64_t *direct);
/* kind: 0 host->device, 1 device->host, 2 device->device; synchronous on the ctx stream */
int sec_memcpy(sec_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);
int sec_memset(sec_ctx *ctx, void *dptr, int value, size_t bytes);
/* Host-to-host copies on the context's copy threads (the caller's thread takes part): dst[i] <-
 * src[i] for len[i] bytes, src 0 = zero-fill.  The Python layer joins a reassembled chunk's rows
 * (present pieces and recovered rows) into its output object with this instead of a
 * single-threaded b"".join (easyfec's join, /root/reference/storb/util/piece.py:196-197). */
typedef struct sec_copy {
    uint64_t dst;
    uint64_t src;
    uint64_t len;
} sec_copy;
int sec_host_copy(sec_ctx *ctx, const sec_copy *jobs, int64_t njobs);

#ifdef __cplusplus
}
#endif
#endif /* STORB_EC_H */
