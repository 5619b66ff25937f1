"""Host-side engine over libstorbec.so: one HIP context per (device, thread).

Two ways in (``repair_batch`` / ``repair_host``, lost blocks regenerated from any k survivors,
and ``check_batch`` / ``check_host``, the held blocks checked against each other, come in both):
  * device-resident batches (``encode_batch`` / ``decode_batch``): descriptor arrays +
    device addresses (torch tensors, or any integer address) — the bench and the GPU parity
    tests use these;
  * host batches (``encode_host`` / ``decode_host``): lists of bytes-like objects; the
    library gathers them into pinned staging, runs the kernels and copies results back —
    this is what the easyfec-compatible layer and the ``piece`` drop-in use.

There is no CPU compute path: every call goes to the HIP kernels; construction raises
``ECRuntimeError`` when no device is present.
"""

from __future__ import annotations

import contextlib
import ctypes
import os
import threading
import weakref

import numpy as np

from . import _lib
from ._lib import (CHK_DTYPE, CHK_RESULT_DTYPE, COPY_DTYPE, COR_RESULT_DTYPE, DCHK_DTYPE, DEC_DTYPE, ENC_DTYPE,
                   MSG_DTYPE, RCHK_DTYPE, REP_DTYPE, SEC_F_ASYNC, SEC_F_GPU_PARITY_IDS, SEC_F_HOST, SEC_F_RECOVER,
                   SEC_F_STAGED)


class Error(Exception):
    """A zfec precondition violation (zfec raises ``zfec.Error`` for the same cases)."""


class ECRuntimeError(RuntimeError):
    """Device / runtime failure (no GPU, HIP error, out of memory)."""


def check(rc: int, lib=None) -> None:
    if rc == 0:
        return
    msg = _lib.strerror(rc, lib)
    if rc in _lib.PRECONDITION_CODES:
        raise Error(msg)
    raise ECRuntimeError(f"libstorbec: {msg} (status {rc})")


def addr(obj) -> tuple[int, object]:
    """(address, keep-alive) of a buffer: int, torch tensor, numpy array or bytes-like."""
    if obj is None:
        return 0, None
    if isinstance(obj, int):
        return obj, None
    if hasattr(obj, "data_ptr"):  # torch.Tensor (device or host)
        return int(obj.data_ptr()), obj
    if isinstance(obj, np.ndarray):
        return int(obj.ctypes.data), obj
    arr = np.frombuffer(obj, dtype=np.uint8)
    return (int(arr.ctypes.data) if arr.size else 0), arr


def _ptr(a: np.ndarray) -> int:
    return int(a.ctypes.data) if a.size else 0


def _flags(host: bool = False, asynchronous: bool = False, staged: bool = False, recover_only: bool = False) -> int:
    """The flag word of a batch call."""
    return ((SEC_F_HOST if host else 0) | (SEC_F_ASYNC if asynchronous else 0) |
            (SEC_F_STAGED if staged else 0) | (SEC_F_RECOVER if recover_only else 0))


def _rows(flat, width: int, counts, conv=bytes) -> list[list]:
    """A flat array of `width`-byte records cut into rows, counts[c] records for chunk c, each
    record through `conv`."""
    mv = memoryview(flat)
    out, f = [], 0
    for n in counts:
        out.append([conv(mv[width * (f + j):width * (f + j + 1)]) for j in range(n)])
        f += n
    return out


def _decoded_len(item) -> int:
    """The k*B - padlen bytes a decode item (k, m, blocks, sharenums, padlen) reassembles to."""
    return item[0] * len(item[2][0]) - item[4]


def _decoded_starts(items) -> list[int]:
    """Where each decode item's bytes start in the concatenation of them all; last, its length."""
    starts = [0]
    for it in items:
        starts.append(starts[-1] + _decoded_len(it))
    return starts


def default_device() -> int:
    for var in ("STORB_EC_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v is not None and v.strip().lstrip("-").isdigit():
            return int(v)
    return 0


def device_count() -> int:
    lib = _lib.load()
    n = ctypes.c_int(0)
    rc = lib.sec_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


_TIMING_KINDS = {"encode": 0, "decode": 1, "sha1": 2, "bignum": 3, "repair": 4, "check": 5,
                 "decode_check": 6, "repair_check": 7, "decode_correct": 8}


class Engine:
    """A libstorbec context on one device.  Not thread-safe; use ``get_engine()`` per thread."""

    def __init__(self, device: int | None = None, lib_path: str | None = None, options: dict | None = None):
        self.lib = _lib.load(lib_path)
        self.device = default_device() if device is None else int(device)
        h = ctypes.c_void_p()
        rc = self.lib.sec_ctx_create(self.device, ctypes.byref(h))
        if rc:
            raise ECRuntimeError(f"cannot create HIP context on device {self.device}: {_lib.strerror(rc)}")
        self._ctx = h
        try:
            for k, v in (options or {}).items():  # sec_ctx_set_option: forced plan choices (tests, A/B)
                self.set_option(k, int(v))
        except BaseException:  # an unknown option or a bad value: no context left behind
            self.close()
            raise

    def _check(self, rc: int) -> None:
        check(rc, self.lib)

    # -- lifecycle / stream / timing ----------------------------------------
    def close(self) -> None:
        if self._ctx:
            self.lib.sec_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream) -> None:
        """Launch on an external hipStream_t (int handle or torch.cuda.Stream); None = own."""
        h = getattr(stream, "cuda_stream", stream)
        self._check(self.lib.sec_ctx_set_stream(self._ctx, h or None))

    def sync(self) -> None:
        self._check(self.lib.sec_sync(self._ctx))

    def set_timing(self, enable: bool) -> None:
        self._check(self.lib.sec_ctx_set_timing(self._ctx, int(bool(enable))))

    def collect_timing(self, kind: str) -> tuple[float, int]:
        """(summed kernel ms, launch count) recorded since the last collect;
        kind 'encode' | 'decode' | 'sha1' | 'bignum' | 'repair' | 'check' | 'decode_check' |
        'repair_check' | 'decode_correct' (the correcting calls: decode + correct and
        repair + correct, the latter's SHA-1 included)."""
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        self._check(self.lib.sec_timing_collect(self._ctx, _TIMING_KINDS[kind], ctypes.byref(ms),
                                          ctypes.byref(n)))
        return ms.value, n.value

    # -- context options (sec_ctx_set_option) ----------------------------------
    def set_option(self, name: str, value: int) -> None:
        """Force a plan choice on this context (tests, A/B tools); see include/storb_ec.h.
        The library reads no environment variable: an option holds only for this engine."""
        self._check(self.lib.sec_ctx_set_option(self._ctx, name.encode(), int(value)))

    def option(self, name: str) -> int:
        v = ctypes.c_int64(0)
        self._check(self.lib.sec_ctx_get_option(self._ctx, name.encode(), ctypes.byref(v)))
        return v.value

    @contextlib.contextmanager
    def options(self, **opts):
        """``with eng.options(SEC_SYN=0): ...``: the options set for the block, restored after."""
        old = {k: self.option(k) for k in opts}
        try:
            for k, v in opts.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)

    # -- device-resident batches --------------------------------------------
    def encode_batch(self, descs: np.ndarray, src, parity, *, host: bool = False, asynchronous: bool = False,
                     staged: bool = False) -> None:
        """sec_encode_batch.  staged (host only): never page-lock pageable buffers for the call
        (SEC_F_STAGED), for callers whose other threads fault in memory meanwhile."""
        descs = np.ascontiguousarray(descs, dtype=ENC_DTYPE)
        s, _ks = addr(src)
        p, _kp = addr(parity)
        self._check(self.lib.sec_encode_batch(self._ctx, _ptr(descs), len(descs), s or None, p or None,
                                              _flags(host, asynchronous, staged)))

    def decode_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks, out, *,
                     block_avail: np.ndarray | None = None, recover_only: bool = False, host: bool = False,
                     asynchronous: bool = False, staged: bool = False) -> None:
        """sec_decode_batch_ex.  block_avail (per slot, optional): bytes of the block that exist,
        the rest read as zero (zfec's padded last data block read in place: B - padlen).
        recover_only: write just the missing primaries (SEC_F_RECOVER), e*B bytes per chunk.
        staged: as encode_batch."""
        descs = np.ascontiguousarray(descs, dtype=DEC_DTYPE)
        sn = np.ascontiguousarray(sharenums, dtype=np.int32)
        bo = np.ascontiguousarray(block_offs, dtype=np.uint64)
        av = None if block_avail is None else np.ascontiguousarray(block_avail, dtype=np.uint64)
        if av is not None and av.size < bo.size:
            raise ValueError("block_avail needs one entry per slot")
        b, _kb = addr(blocks)
        o, _ko = addr(out)
        self._check(self.lib.sec_decode_batch_ex(self._ctx, _ptr(descs), len(descs), _ptr(sn), _ptr(bo),
                                                 None if av is None else _ptr(av), b or None, o or None,
                                                 _flags(host, asynchronous, staged, recover_only)))

    # -- the repair / check family: shared plumbing ---------------------------
    def _row_call(self, fn, dtype, descs, sharenums, block_offs, block_avail, targets, bufs, *, host, asynchronous,
                  recover_only=False, extra=()) -> None:
        """One call of the repair / check family: fn(ctx, descs, n, sharenums, block_offs,
        block_avail, blocks, [target_nums, target_offs,] *outputs, *extra, flags).  targets:
        (target_nums, target_offs) or None; bufs: (blocks, *outputs), each an address, tensor, array
        or None; extra: integer arguments in front of the flags (the _ex calls' max_errors)."""
        descs = np.ascontiguousarray(descs, dtype=dtype)
        sn = np.ascontiguousarray(sharenums, dtype=np.int32)
        bo = np.ascontiguousarray(block_offs, dtype=np.uint64)
        tn = to = None
        if targets is not None:
            tn = np.ascontiguousarray(targets[0], dtype=np.int32)
            to = np.ascontiguousarray(targets[1], dtype=np.uint64)
        av = None if block_avail is None else np.ascontiguousarray(block_avail, dtype=np.uint64)
        if av is not None and av.size < bo.size:
            raise ValueError("block_avail needs one entry per slot")
        if tn is not None and tn.size != to.size:
            raise ValueError("one target address per target")
        held = [addr(x) for x in bufs]  # (address, keep-alive)
        args = [_ptr(sn) or None, _ptr(bo) or None, None if av is None else _ptr(av), held[0][0] or None]
        if tn is not None:
            args += [_ptr(tn) or None, _ptr(to) or None]
        args += [a or None for a, _ in held[1:]]
        self._check(fn(self._ctx, _ptr(descs), len(descs), *args, *extra,
                       _flags(host, asynchronous, recover_only=recover_only)))

    @staticmethod
    def _lay_out_blocks(items):
        """Every item's blocks (it[2], numbered it[3]) as one sn / bo pair of host addresses:
        (sn, bo, keep, first), first[j] = item j's first slot, keep = what must outlive the call."""
        nslots = sum(len(it[2]) for it in items)
        sn = np.zeros(max(nslots, 1), dtype=np.int32)
        bo = np.zeros(max(nslots, 1), dtype=np.uint64)
        keep, first = [], []
        slot = 0
        for it in items:
            first.append(slot)
            for q, b in enumerate(it[2]):
                a, kp = addr(b)
                keep.append(kp)
                bo[slot + q] = a
                sn[slot + q] = int(it[3][q])
            slot += len(it[2])
        return sn, bo, keep, first

    @staticmethod
    def _recovered_bytes(item) -> int:
        """What a recover-only call writes for a chunk: B bytes per primary missing from its
        first k blocks."""
        k = item[0]
        return sum(1 for x in item[3][:k] if int(x) >= k) * len(item[2][0])

    @staticmethod
    def _join_views(item, rows, o) -> list:
        """A chunk's k*B - padlen bytes as views, in order: its present primaries (among its first
        k blocks) from the caller's blocks, the others from the recovered rows at rows[o:]."""
        k, _m, blocks, sharenums, padlen = item
        B = len(blocks[0])
        prim = {int(x): q for q, x in enumerate(sharenums[:k]) if int(x) < k}  # primary -> its block
        left = k * B - padlen
        views = []
        for row in range(k):
            if left <= 0:
                break
            if row in prim:
                v = memoryview(blocks[prim[row]]).cast("B")
            else:  # the next recovered row (rows come in primary order)
                v = rows[o:o + B]
                o += B
            views.append(v[:left] if left < B else v)
            left -= B
        return views

    @staticmethod
    def _lay_out_targets(items, digests: bool):
        """A new bytes object per target (it[4]) of every item: (tn, to, dig, objs, first, views),
        objs[j] = item j's unfinished targets, first[j] = its first target slot, dig = 20 bytes per
        target slot when digests are asked for, views = what must outlive the call."""
        from ._hostbytes import _new_bytes

        ntg = sum(len(it[4]) for it in items)
        tn = np.zeros(max(ntg, 1), dtype=np.int32)
        to = np.zeros(max(ntg, 1), dtype=np.uint64)
        objs, first, views = [], [], []
        tgt = 0
        for it in items:
            B = len(it[2][0])
            first.append(tgt)
            row = []
            for q, t in enumerate(it[4]):
                b, v = _new_bytes(B)
                row.append(b)
                tn[tgt + q] = int(t)
                to[tgt + q] = v.ctypes.data if B else 0
                views.append(v)
            objs.append(row)
            tgt += len(it[4])
        dig = np.zeros(max(20 * ntg, 1), dtype=np.uint8) if digests else None
        return tn, to, dig, objs, first, views

    @staticmethod
    def _targets_done(objs, dig):
        """The finished targets per item and, with digests, each one's 20 bytes."""
        from ._hostbytes import _finalize

        out = [[_finalize(b) for b in row] for row in objs]
        return out, (None if dig is None else _rows(dig, 20, [len(row) for row in out]))

    @staticmethod
    def _check_results(items, first, res, rb, col):
        """Per item ``(first, bad, column)`` from a check-family call's results."""
        out = []
        for j, it in enumerate(items):
            s0, nb = first[j], len(it[2])
            if int(res[j]["first"]) == _lib.CHK_CONSISTENT:
                out.append((None, [], None))
            else:
                out.append((int(res[j]["first"]), [q for q in range(nb) if rb[s0 + q]], col[s0:s0 + nb].tobytes()))
        return out

    @staticmethod
    def _result_arrays(nitems: int, nslots: int):
        return (np.zeros(nitems, dtype=CHK_RESULT_DTYPE), np.zeros(max(nslots, 1), dtype=np.uint8),
                np.zeros(max(nslots, 1), dtype=np.uint8))

    def repair_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks,
                     target_nums: np.ndarray, target_offs: np.ndarray, out, *, block_avail: np.ndarray | None = None,
                     digests=None, host: bool = False, asynchronous: bool = False) -> None:
        """sec_repair_batch: block target_nums[tgt0 + j] of each chunk (REP_DTYPE descriptors)
        written whole at out + target_offs[tgt0 + j] from the chunk's k source blocks.
        block_avail as decode_batch; digests (optional): 20 bytes per target slot, the repaired
        piece's SHA-1, where the targets live.  host: host buffers, always staged."""
        self._row_call(self.lib.sec_repair_batch, REP_DTYPE, descs, sharenums, block_offs, block_avail,
                       (target_nums, target_offs), (blocks, out, digests), host=host, asynchronous=asynchronous)

    def repair_host(self, items, digests: bool = False):
        """Lost blocks of host chunks, regenerated from k survivors each, in one call.

        items: [(k, m, blocks, sharenums, targets)] with exactly k equal-length blocks per chunk
        and the block numbers to regenerate.  Returns, per chunk, the target blocks as bytes in
        the order of `targets`; with ``digests=True`` also, per chunk, each one's SHA-1 digest
        (20 bytes, GPU-computed on the repaired piece)."""
        for it in items:
            check_repair_item(*it)
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        tn, to, dig, objs, tgt0, _views = self._lay_out_targets(items, digests)
        descs = np.zeros(len(items), dtype=REP_DTYPE)
        for j, (k, m, blocks, _sharenums, targets) in enumerate(items):
            descs[j] = (len(blocks[0]), slot0[j], tgt0[j], len(targets), k, m, 0)
        if any(len(it[4]) for it in items):
            self.repair_batch(descs, sn, bo, 0, tn, to, 0, digests=dig, host=True)
        out, digs = self._targets_done(objs, dig)
        return (out, digs) if digests else out

    def check_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks, results, *,
                    block_avail: np.ndarray | None = None, row_bad=None, column=None, host: bool = False,
                    asynchronous: bool = False) -> None:
        """sec_check_batch: of each chunk's n held blocks (CHK_DTYPE descriptors; entries slot0 ..
        slot0+k-1 the basis, the rest the check rows) every check row is predicted from the basis
        and compared with the stored block.  results: one CHK_RESULT_DTYPE per chunk (first
        differing position or CHK_CONSISTENT, differing rows); row_bad, column (optional): one
        byte per slot entry; all three where the blocks live.  block_avail as decode_batch.
        host: host buffers, always staged."""
        self._row_call(self.lib.sec_check_batch, CHK_DTYPE, descs, sharenums, block_offs, block_avail, None,
                       (blocks, results, row_bad, column), host=host, asynchronous=asynchronous)

    def check_host(self, items):
        """Whether the held blocks of host chunks agree with each other, in one call.

        items: [(k, m, blocks, sharenums)] with n >= k equal-length blocks per chunk, the first k
        the basis, the others the check rows.  Returns, per chunk, ``(first, bad, column)``:
        first = the lowest byte position at which a check row differs from its prediction (None:
        the chunk is consistent), bad = the positions in `blocks` of the check rows that differ
        anywhere, column = the n blocks' bytes at `first` (None when consistent), the input of
        ``check_locate``."""
        for it in items:
            check_check_item(*it)
        if not items:
            return []
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        descs = np.zeros(len(items), dtype=CHK_DTYPE)
        for j, (k, m, blocks, _sharenums) in enumerate(items):
            descs[j] = (len(blocks[0]), slot0[j], len(blocks), k, m, 0)
        res, rb, col = self._result_arrays(len(items), sn.size)
        self.check_batch(descs, sn, bo, 0, res, row_bad=rb, column=col, host=True)
        return self._check_results(items, slot0, res, rb, col)

    def decode_check_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks, out,
                           results, *, block_avail: np.ndarray | None = None, row_bad=None, column=None,
                           host: bool = False, asynchronous: bool = False, recover_only: bool = False) -> None:
        """sec_decode_check_batch: decode_batch on each chunk's first k entries and check_batch on
        all n of them (DCHK_DTYPE descriptors) in one pass over the blocks.  `out` receives what
        decode_batch writes (recover_only: just the missing primaries), consistent or not;
        results, row_bad and column what check_batch reports.  host: host buffers, always staged,
        every entry gathered once."""
        self._row_call(self.lib.sec_decode_check_batch, DCHK_DTYPE, descs, sharenums, block_offs, block_avail, None,
                       (blocks, out, results, row_bad, column), host=host, asynchronous=asynchronous,
                       recover_only=recover_only)

    def decode_check_host(self, items):
        """Reassemble host chunks and check their spare blocks in one call.

        items: [(k, m, blocks, sharenums, padlen)] with n >= k equal-length blocks per chunk: the
        first k are decoded from and are the check's basis, the others are the check rows.
        Returns ``(data, checks)``: data = every chunk's k*B - padlen bytes concatenated, as
        ``decode_host`` returns them; checks = per chunk ``(first, bad, column)`` as
        ``check_host`` returns them.  One recover-only host call stages every block once; only the
        recovered rows and the results come back, and the present primaries are joined from the
        caller's blocks on the library's copy threads.  The bytes are returned whatever the check
        says."""
        for it in items:
            check_decode_check_item(*it)
        if not items:
            return b"", []
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        descs = np.zeros(len(items), dtype=DCHK_DTYPE)
        rec = []
        total = 0
        for j, it in enumerate(items):
            k, m, blocks, _sharenums, padlen = it
            descs[j] = (total, len(blocks[0]), padlen, slot0[j], len(blocks), k, m, 0)
            rec.append(total)
            total += self._recovered_bytes(it)
        buf = self._out_buffer(max(total, 1))
        res, rb, col = self._result_arrays(len(items), sn.size)
        self.decode_check_batch(descs, sn, bo, 0, buf, res, row_bad=rb, column=col, host=True, recover_only=True)
        mv = memoryview(buf)
        views = [v for it, o in zip(items, rec) for v in self._join_views(it, mv, o)]
        return self._joined(views), self._check_results(items, slot0, res, rb, col)

    def decode_correct_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks, out,
                             results, *, block_avail: np.ndarray | None = None, entry_hits=None, host: bool = False,
                             asynchronous: bool = False, max_errors: int = 1) -> None:
        """sec_decode_correct_batch: every byte position's column of each chunk's n entries
        (DCHK_DTYPE descriptors) judged as ``check_locate`` judges it, and `out` what decode_batch
        writes from the first k entries after the one wrong basis byte of a position, if any, is
        put right.  results: one COR_RESULT_DTYPE per chunk; entry_hits (optional): one uint32 per
        slot entry, the positions at which that entry was the one changed; both where the blocks
        live.  host: host buffers, always staged, every entry gathered once.

        max_errors other than 1: sec_decode_correct_ex_batch, which judges a column as
        ``check_correct`` does: up to t = min(max_errors, (n - k) // 2, 16) wrong entries of a
        position are put right (0: the code's limit), each counting a hit; more than t and at most
        n - k - t are always open."""
        if max_errors == 1:
            self._row_call(self.lib.sec_decode_correct_batch, DCHK_DTYPE, descs, sharenums, block_offs, block_avail,
                           None, (blocks, out, results, entry_hits), host=host, asynchronous=asynchronous)
            return
        self._row_call(self.lib.sec_decode_correct_ex_batch, DCHK_DTYPE, descs, sharenums, block_offs, block_avail,
                       None, (blocks, out, results, entry_hits), host=host, asynchronous=asynchronous,
                       extra=(int(max_errors),))

    def decode_correct_host(self, items, max_errors: int = 1):
        """Reassemble host chunks, correcting wrong blocks per byte position, in one call.

        items: [(k, m, blocks, sharenums, padlen)] as ``decode_check_host`` takes them.  Returns
        ``(data, results)``: data = every chunk's k*B - padlen bytes concatenated; results = per
        chunk ``(first, first_open, corrected, open, hits)``: the lowest position whose column is
        no code word and the lowest one left open (None: there is none), the counts of corrected
        and of open positions, and per block of the chunk the positions at which it was changed.
        max_errors as ``decode_correct_batch``: 1 puts one wrong block of a position right."""
        for it in items:
            check_decode_correct_item(*it)
        if not items:
            return b"", []
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        descs = np.zeros(len(items), dtype=DCHK_DTYPE)
        starts = _decoded_starts(items)
        for j, (k, m, blocks, _sharenums, padlen) in enumerate(items):
            descs[j] = (starts[j], len(blocks[0]), padlen, slot0[j], len(blocks), k, m, 0)
        buf = self._out_buffer(max(starts[-1], 1))
        res = np.zeros(len(items), dtype=COR_RESULT_DTYPE)
        hits = np.zeros(sn.size, dtype=np.uint32)
        self.decode_correct_batch(descs, sn, bo, 0, buf, res, entry_hits=hits, host=True, max_errors=max_errors)
        return buf[:starts[-1]].tobytes(), self._correct_results(items, slot0, res, hits)

    def repair_check_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks,
                           target_nums: np.ndarray, target_offs: np.ndarray, out, results, *,
                           block_avail: np.ndarray | None = None, digests=None, row_bad=None, column=None,
                           host: bool = False, asynchronous: bool = False) -> None:
        """sec_repair_check_batch: repair_batch from each chunk's first k entries and check_batch
        on all n of them (RCHK_DTYPE descriptors) in one pass over the blocks.  The targets (and
        digests) receive what repair_batch writes, consistent or not; results, row_bad and column
        what check_batch reports.  host: host buffers, always staged, every entry gathered once."""
        self._row_call(self.lib.sec_repair_check_batch, RCHK_DTYPE, descs, sharenums, block_offs, block_avail,
                       (target_nums, target_offs), (blocks, out, digests, results, row_bad, column), host=host,
                       asynchronous=asynchronous)

    def repair_check_host(self, items, digests: bool = False):
        """Lost blocks of host chunks regenerated and their spare blocks checked, in one call.

        items: [(k, m, blocks, sharenums, targets)] with n >= k equal-length blocks per chunk: the
        first k are repaired from and are the check's basis, the others are the check rows.
        Returns what ``repair_host`` returns (per chunk the target blocks as bytes in the order of
        `targets`; with ``digests=True`` also, per chunk, each one's SHA-1 digest) followed by
        checks = per chunk ``(first, bad, column)`` as ``check_host`` returns them.  One host
        call stages every block once.  The targets are returned whatever the check says."""
        for it in items:
            check_repair_check_item(*it)
        if not items:
            return ([], [], []) if digests else ([], [])
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        tn, to, dig, objs, tgt0, _views = self._lay_out_targets(items, digests)
        descs = np.zeros(len(items), dtype=RCHK_DTYPE)
        for j, (k, m, blocks, _sharenums, targets) in enumerate(items):
            descs[j] = (len(blocks[0]), slot0[j], tgt0[j], len(targets), len(blocks), k, m)
        res, rb, col = self._result_arrays(len(items), sn.size)
        self.repair_check_batch(descs, sn, bo, 0, tn, to, 0, res, digests=dig, row_bad=rb, column=col, host=True)
        out, digs = self._targets_done(objs, dig)
        checks = self._check_results(items, slot0, res, rb, col)
        return (out, digs, checks) if digests else (out, checks)

    def repair_correct_batch(self, descs: np.ndarray, sharenums: np.ndarray, block_offs: np.ndarray, blocks,
                             target_nums: np.ndarray, target_offs: np.ndarray, out, results, *,
                             block_avail: np.ndarray | None = None, digests=None, entry_hits=None,
                             host: bool = False, asynchronous: bool = False, max_errors: int = 1) -> None:
        """sec_repair_correct_batch: every byte position's column of each chunk's n entries
        (RCHK_DTYPE descriptors) judged as ``check_locate`` judges it, and every target written
        whole from the first k entries after the one wrong basis byte of a position, if any, is
        put right.  A target may be a held entry (a heal target).  digests as repair_batch;
        results and entry_hits as decode_correct_batch.  host: host buffers, always staged, every
        entry gathered once.  max_errors other than 1: sec_repair_correct_ex_batch, the columns
        judged as ``decode_correct_batch`` says, every changed basis entry applied to a target."""
        if max_errors == 1:
            self._row_call(self.lib.sec_repair_correct_batch, RCHK_DTYPE, descs, sharenums, block_offs, block_avail,
                           (target_nums, target_offs), (blocks, out, digests, results, entry_hits), host=host,
                           asynchronous=asynchronous)
            return
        self._row_call(self.lib.sec_repair_correct_ex_batch, RCHK_DTYPE, descs, sharenums, block_offs, block_avail,
                       (target_nums, target_offs), (blocks, out, digests, results, entry_hits), host=host,
                       asynchronous=asynchronous, extra=(int(max_errors),))

    def repair_correct_host(self, items, digests: bool = False, max_errors: int = 1):
        """Blocks of host chunks regenerated or healed from the column-corrected code word, in one
        call.

        items: [(k, m, blocks, sharenums, targets)] as ``repair_check_host`` takes them, except
        that a target may be one of the blocks held: it comes back whole with the bytes put right
        at which it was the block changed.  Returns what ``repair_host`` returns (per chunk the
        target blocks as bytes in the order of `targets`; with ``digests=True`` also, per chunk,
        each one's SHA-1 digest) followed by what ``decode_correct_host`` returns per chunk:
        ``(first, first_open, corrected, open, hits)``, hits per block of the chunk in the
        caller's order."""
        for it in items:
            check_repair_correct_item(*it)
        if not items:
            return ([], [], []) if digests else ([], [])
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        tn, to, dig, objs, tgt0, _views = self._lay_out_targets(items, digests)
        descs = np.zeros(len(items), dtype=RCHK_DTYPE)
        for j, (k, m, blocks, _sharenums, targets) in enumerate(items):
            descs[j] = (len(blocks[0]), slot0[j], tgt0[j], len(targets), len(blocks), k, m)
        res = np.zeros(len(items), dtype=COR_RESULT_DTYPE)
        hits = np.zeros(sn.size, dtype=np.uint32)
        self.repair_correct_batch(descs, sn, bo, 0, tn, to, 0, res, digests=dig, entry_hits=hits, host=True,
                                  max_errors=max_errors)
        out, digs = self._targets_done(objs, dig)
        cor = self._correct_results(items, slot0, res, hits)
        return (out, digs, cor) if digests else (out, cor)

    @staticmethod
    def _correct_results(items, first, res, hits):
        """Per item ``(first, first_open, corrected, open, hits)`` from a correcting call's results."""
        none = _lib.CHK_CONSISTENT
        out = []
        for j, it in enumerate(items):
            bad, fopen = int(res[j]["first"]), int(res[j]["first_open"])
            out.append((None if bad == none else bad, None if fopen == none else fopen,
                        int(res[j]["corrected"]), int(res[j]["open"]),
                        [int(h) for h in hits[first[j]:first[j] + len(it[2])]]))
        return out

    def encode_digest_batch(self, descs: np.ndarray, src, parity, digests, *, host: bool = False,
                            asynchronous: bool = False) -> None:
        """Encode + SHA-1 of every block (20 B per block, chunk-major) — sec_encode_digest_batch."""
        descs = np.ascontiguousarray(descs, dtype=ENC_DTYPE)
        s, _ks = addr(src)
        p, _kp = addr(parity)
        g, _kg = addr(digests)
        self._check(self.lib.sec_encode_digest_batch(self._ctx, _ptr(descs), len(descs), s or None, p or None,
                                                     g or None, _flags(host, asynchronous)))

    @staticmethod
    def _key_handle(key):
        """The sec_bn_key of a ``bn.ModKey`` (or a raw handle), for the tagged encode calls."""
        h = getattr(key, "handle", key)
        if not h:
            raise ECRuntimeError("tagged encode needs an open ModKey")
        return h

    def encode_tag_batch(self, descs: np.ndarray, src, parity, tags, key, *, digests=None, host: bool = False,
                         asynchronous: bool = False) -> None:
        """Encode + the APDP tag of every block (256 B big-endian per block, chunk-major, the
        slot numbering of ``encode_digest_batch``) and, with ``digests``, every block's SHA-1:
        one pass over the chunk (sec_encode_tag_batch).  key: a ``bn.ModKey`` of this engine
        with ``set_tag`` done."""
        descs = np.ascontiguousarray(descs, dtype=ENC_DTYPE)
        s, _ks = addr(src)
        p, _kp = addr(parity)
        t, _kt = addr(tags)
        g, _kg = addr(digests) if digests is not None else (0, None)
        self._check(self.lib.sec_encode_tag_batch(self._ctx, self._key_handle(key), _ptr(descs), len(descs),
                                                  s or None, p or None, g or None, t or None,
                                                  _flags(host, asynchronous)))

    @staticmethod
    def _tag_ints(tags: np.ndarray, ms) -> list[list[int]]:
        """Per chunk, its m tags as Python ints (tags: 256 bytes per slot, chunk-major)."""
        return _rows(tags, 256, ms, lambda v: int.from_bytes(v, "big"))

    def sha1_batch(self, msgs: np.ndarray, digests, *, host: bool = False, asynchronous: bool = False) -> None:
        """SHA-1 of each (addr, len, avail) message into 20-byte digests — sec_sha1_batch."""
        msgs = np.ascontiguousarray(msgs, dtype=MSG_DTYPE)
        g, _kg = addr(digests)
        self._check(self.lib.sec_sha1_batch(self._ctx, _ptr(msgs), len(msgs), g or None, _flags(host, asynchronous)))

    # -- pinned host memory: the zero-copy host path ----------------------------
    def host_empty(self, nbytes: int) -> np.ndarray:
        """A page-locked uint8 host array (sec_host_alloc).  ``host=True`` calls whose buffers
        are all pinned run the kernels on them directly over PCIe, with no staging copy.
        Freed when the array and every view of it are gone."""
        n = int(nbytes)
        p = ctypes.c_void_p()
        self._check(self.lib.sec_host_alloc(self._ctx, max(n, 1), ctypes.byref(p)))
        raw = (ctypes.c_uint8 * max(n, 1)).from_address(p.value)
        weakref.finalize(raw, self.lib.sec_host_free, None, p.value).atexit = False  # the OS reclaims at exit
        return np.frombuffer(raw, dtype=np.uint8, count=n)

    def register(self, buf) -> None:
        """Page-lock an existing writable host buffer (hipHostRegister) so ``host=True`` calls
        on it take the zero-copy path.  Call ``unregister`` before the buffer is freed."""
        a, keep = addr(buf)
        self._check(self.lib.sec_host_register(self._ctx, a, keep.nbytes if keep is not None else len(buf)))

    def unregister(self, buf) -> None:
        a, _ = addr(buf)
        self._check(self.lib.sec_host_unregister(None, a))

    def host_paths(self) -> tuple[int, int, int]:
        """(zero-copy on pinned buffers, zero-copy on pages locked for the call, staged) counts
        of the ``host=True`` encode / decode calls so far."""
        z, r, st = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.sec_ctx_host_paths(self._ctx, ctypes.byref(z), ctypes.byref(r), ctypes.byref(st)))
        return z.value, r.value, st.value

    def decode_paths(self) -> tuple[int, int]:
        """(syndrome, direct): chunks with a lost data block decoded so far, by method."""
        syn, direct = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.sec_ctx_decode_paths(self._ctx, ctypes.byref(syn), ctypes.byref(direct)))
        return syn.value, direct.value

    def decode_methods(self) -> tuple[int, int, int, int]:
        """(fused one-wave syndrome kernel, two-wave kernel, two syndrome kernels, direct): chunks
        with a lost data block decoded so far, by kernel."""
        f, p, t, d = (ctypes.c_int64(0) for _ in range(4))
        self._check(self.lib.sec_ctx_decode_methods(self._ctx, ctypes.byref(f), ctypes.byref(p), ctypes.byref(t),
                                                    ctypes.byref(d)))
        return f.value, p.value, t.value, d.value

    def check_methods(self) -> tuple[int, int]:
        """(bit-sliced, direct): chunks with at least one check row that check and decode + check
        calls have checked so far, by kernel (option ``SEC_CHECK_BS``)."""
        b, d = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.sec_ctx_check_methods(self._ctx, ctypes.byref(b), ctypes.byref(d)))
        return b.value, d.value

    def repair_methods(self) -> tuple[int, int]:
        """(bit-sliced, direct): chunks with at least one target that repair and repair + check
        calls have repaired so far, by kernel (option ``SEC_CHECK_BS``; ``repair_method`` says
        which chunks are eligible)."""
        b, d = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.sec_ctx_repair_methods(self._ctx, ctypes.byref(b), ctypes.byref(d)))
        return b.value, d.value

    _SCRATCH_CAP = 256 << 20  # largest result staged in the reusable pinned scratch

    def _out_buffer(self, nbytes: int) -> np.ndarray:
        """Result buffer of encode_host / decode_host: a reusable pinned scratch (so a call on
        pinned inputs stays zero-copy end to end; results are copied out before returning), or
        plain memory past _SCRATCH_CAP."""
        n = max(int(nbytes), 1)
        if n > self._SCRATCH_CAP:
            return np.empty(n, dtype=np.uint8)
        cur = getattr(self, "_scratch", None)
        if cur is None or cur.size < n:
            cur = self._scratch = self.host_empty(max(n, 2 * (cur.size if cur is not None else 0), 1 << 20))
        return cur[:n]

    # -- host batches ---------------------------------------------------------
    def sha1_host(self, datas) -> list[bytes]:
        """SHA-1 digests (20 bytes each) of host byte strings, hashed on the GPU."""
        msgs = np.zeros(len(datas), dtype=MSG_DTYPE)
        keep = []
        for i, d in enumerate(datas):
            a, kp = addr(d)
            keep.append(kp)
            ln = len(kp) if isinstance(kp, np.ndarray) else len(d)
            msgs[i] = (a, ln, ln)
        out = np.empty(max(20 * len(datas), 1), dtype=np.uint8)
        self.sha1_batch(msgs, out, host=True)
        mv = memoryview(out)
        return [bytes(mv[20 * i:20 * (i + 1)]) for i in range(len(datas))]

    @staticmethod
    def _encode_descs(chunks, shapes):
        """ENC_DTYPE descriptors of host chunks (shapes: [(k, m)] per chunk), their parity back
        to back: (descs, layout, total, keep), layout[i] = (offset, B, m - k) of chunk i's parity
        blocks, total = the parity bytes, keep = what must outlive the call."""
        descs = np.zeros(len(chunks), dtype=ENC_DTYPE)
        keep, layout, total = [], [], 0
        for i, (c, (k, m)) in enumerate(zip(chunks, shapes)):
            a, kp = addr(c)
            keep.append(kp)
            ln = len(kp) if isinstance(kp, np.ndarray) else len(c)
            B = -(-ln // k) if ln else 0
            descs[i] = (a, ln, total, max(B, 1), k, m)
            layout.append((total, B, m - k))
            total += (m - k) * B
        return descs, layout, total, keep

    def encode_host_raw(self, chunks, shapes, digests: bool = False, staged: bool = False, tag_key=None):
        """``encode_host`` without the per-block ``bytes``: returns (buf, layout) where buf is
        this engine's pinned result scratch and layout[i] = (offset, B, m - k) of chunk i's
        parity blocks in it, back to back.  buf is reused by the engine's next call.  With
        ``digests=True``: (buf, layout, dig), dig = the SHA-1 of every chunk's m blocks in order,
        20 bytes each (GPU-computed after the encode, sec_encode_digest_batch).  staged: as
        encode_batch.  With ``tag_key`` (a ``bn.ModKey`` with ``set_tag`` done) the result gains a
        last element: per chunk, the APDP tags of its m blocks as Python ints, from the same pass
        (sec_encode_tag_batch)."""
        n = len(chunks)
        descs, layout, total, _keep = self._encode_descs(chunks, shapes)
        out = self._out_buffer(total)
        if tag_key is not None:
            ms = [m for (_, m) in shapes]
            dig = np.empty(max(20 * sum(ms), 1), dtype=np.uint8) if digests else None
            tags = np.empty(max(256 * sum(ms), 1), dtype=np.uint8)
            if n:
                self.encode_tag_batch(descs, 0, out, tags, tag_key, digests=dig, host=True)
            ints = self._tag_ints(tags, ms)
            return (out, layout, dig, ints) if digests else (out, layout, ints)
        if digests:
            dig = np.empty(max(20 * sum(m for (_, m) in shapes), 1), dtype=np.uint8)
            if n:
                self.encode_digest_batch(descs, 0, out, dig, host=True)
            return out, layout, dig
        if n:
            self.encode_batch(descs, 0, out, host=True, staged=staged)
        return out, layout

    def encode_pieces_into(self, chunks, shapes, piece_addrs, digests: np.ndarray | None = None,
                           staged: bool = False, gpu_parity_ids: bool = False, tags: np.ndarray | None = None,
                           tag_key=None) -> None:
        """easyfec's Encoder.encode output for every chunk written to caller buffers
        (sec_encode_pieces): piece_addrs[M_c + j] = the address of a writable B-byte buffer for
        piece j of chunk c (M_c = sum of m over the chunks before c); digests (optional, a
        writable uint8 array of 20 bytes per piece) receives each piece's SHA-1, computed on the
        library's host threads while the GPU encodes (``gpu_parity_ids``: the parity pieces' on
        the GPU, SEC_F_GPU_PARITY_IDS).  shapes: [(k, m)] per chunk.  tags (a writable uint8 array
        of 256 bytes per piece) with tag_key (a ``bn.ModKey`` with ``set_tag`` done): each
        piece's APDP tag, big-endian, from the GPU call that encodes it (sec_encode_pieces_tags)."""
        n = len(chunks)
        descs, _layout, _total, _keep = self._encode_descs(chunks, shapes)
        descs["parity_off"] = 0  # ignored by sec_encode_pieces: the parity goes through the library's scratch
        pa = np.ascontiguousarray(piece_addrs, dtype=np.uint64)
        if pa.size != sum(m for (_, m) in shapes):
            raise ValueError("encode_pieces_into: one piece address per piece")
        if digests is not None and digests.size < 20 * pa.size:
            raise ValueError("encode_pieces_into: digests needs 20 bytes per piece")
        if (tags is None) != (tag_key is None):
            raise ValueError("encode_pieces_into: tags and tag_key go together")
        if tags is not None and tags.size < 256 * pa.size:
            raise ValueError("encode_pieces_into: tags needs 256 bytes per piece")
        flags = _flags(host=True, staged=staged) | (SEC_F_GPU_PARITY_IDS if gpu_parity_ids else 0)
        if n and tags is not None:
            self._check(self.lib.sec_encode_pieces_tags(self._ctx, self._key_handle(tag_key), _ptr(descs), n, None,
                                                        _ptr(pa), None if digests is None else _ptr(digests),
                                                        _ptr(tags), flags))
        elif n:
            self._check(self.lib.sec_encode_pieces(self._ctx, _ptr(descs), n, None, _ptr(pa),
                                                   None if digests is None else _ptr(digests), flags))

    def encode_host(self, chunks, shapes, digests: bool = False, tag_key=None):
        """Parity blocks for each chunk.  chunks: bytes-like list; shapes: [(k, m)] per chunk.

        Returns, per chunk, the m-k secondary blocks (block numbers k..m-1) as bytes; with
        ``digests=True`` also, per chunk, the SHA-1 digests of all m blocks (GPU-computed); with
        ``tag_key`` (a ``bn.ModKey`` with ``set_tag`` done) also, last, per chunk the APDP tags of
        all m blocks as Python ints, from the same pass over the chunk.
        """
        res = self.encode_host_raw(chunks, shapes, digests=digests, tag_key=tag_key)
        mv = memoryview(res[0])
        out = [[[bytes(mv[o + r * B:o + (r + 1) * B]) for r in range(p)] for (o, B, p) in res[1]]]
        if digests:
            out.append(_rows(res[2], 20, [m for (_, m) in shapes]))
        if tag_key is not None:
            out.append(res[-1])
        return out[0] if len(out) == 1 else tuple(out)

    # joins of at least this many bytes go to the library's copy threads (sec_host_copy) instead
    # of a single-threaded b"".join under the GIL
    NATIVE_JOIN_MIN = 1 << 20

    def _join_into(self, views, base: int) -> int:
        """Copy `views` back to back to the host address `base` on the copy threads; returns the
        bytes written."""
        jobs = np.zeros(len(views), dtype=COPY_DTYPE)
        off = 0
        keep = []
        for i, v in enumerate(views):
            a = np.frombuffer(v, dtype=np.uint8)
            keep.append(a)
            n = a.size
            jobs[i] = (base + off, a.ctypes.data if n else 0, n)
            off += n
        if len(views):
            self._check(self.lib.sec_host_copy(self._ctx, _ptr(jobs), len(views)))
        return off

    def _joined(self, views) -> bytes:
        from ._hostbytes import _finalize, _new_bytes

        total = sum(len(v) for v in views)
        if total < self.NATIVE_JOIN_MIN:
            return b"".join(views)
        b, dst = _new_bytes(total)
        self._join_into(views, dst.ctypes.data)
        return _finalize(b)

    # A host reassembly in ONE library call (sec_decode_batch_ex's host join, api.cpp decode_core
    # / join_staged): chunks with every data piece present are copied by the library's task
    # threads and never reach the GPU; the others are recovered on the GPU beside those copies,
    # only the recovered rows crossing PCIe.  False: round 4's form (a recover-only call into a
    # pinned scratch, then the join; A/B in tools/stream_rate.py).
    LIBRARY_JOIN = True

    def _reassemble(self, items, outs) -> None:
        """Every chunk's k*B - padlen bytes written to the host address outs[i], one call."""
        for it in items:
            check_decode_item(*it)
        sn, bo, _keep, slot0 = self._lay_out_blocks(items)
        descs = np.zeros(len(items), dtype=DEC_DTYPE)
        for j, (k, m, blocks, _sharenums, padlen) in enumerate(items):
            descs[j] = (int(outs[j]), len(blocks[0]), padlen, slot0[j], k, m)
        if len(items):
            # (not staged=True: when the pieces are too scattered to page-lock, the library
            # copies the present ones into the output first and a large call's kernels read
            # them back from there, the output page-locked for the call)
            self.decode_batch(descs, sn, bo, 0, 0, host=True)

    def decode_host(self, items) -> bytes:
        """Reassemble chunks from host blocks, concatenated in order.

        items: [(k, m, blocks, sharenums, padlen)] with exactly k equal-length blocks each.
        Returns the concatenation of every chunk's k*B - padlen bytes.
        """
        if not self.LIBRARY_JOIN:
            return self._joined(self._decode_parts(items, per_chunk=False))
        from ._hostbytes import _finalize, _new_bytes

        starts = _decoded_starts(items)
        b, dst = _new_bytes(starts[-1])
        if dst.size:
            self._reassemble(items, [dst.ctypes.data + o for o in starts[:-1]])
        return _finalize(b)

    def decode_host_into(self, items, dst: np.ndarray) -> int:
        """``decode_host`` written into `dst` (a writable uint8 array) instead of a new bytes
        object: the output of a share of a multi-device call lands straight in the caller's
        result.  Returns the bytes written; ValueError when `dst` is too small."""
        if not self.LIBRARY_JOIN:
            views = self._decode_parts(items, per_chunk=False)
            if sum(len(v) for v in views) > dst.size:
                raise ValueError("decode_host_into: destination too small")
            return self._join_into(views, dst.ctypes.data) if dst.size else 0
        starts = _decoded_starts(items)
        if starts[-1] > dst.size:
            raise ValueError("decode_host_into: destination too small")
        if starts[-1]:
            self._reassemble(items, [dst.ctypes.data + o for o in starts[:-1]])
        return starts[-1]

    def decode_host_chunks(self, items) -> list[bytes]:
        """``decode_host``, one bytes object per chunk."""
        if not self.LIBRARY_JOIN:
            return [self._joined(p) for p in self._decode_parts(items, per_chunk=True, views=True)]
        from ._hostbytes import _finalize, _new_bytes

        objs = [_new_bytes(_decoded_len(it)) for it in items]
        live = [(it, v.ctypes.data) for it, (_, v) in zip(items, objs) if v.size]
        if live:
            self._reassemble([it for it, _ in live], [a for _, a in live])
        return [_finalize(b) for b, _ in objs]

    def _decode_parts(self, items, per_chunk: bool, views: bool = False) -> list:
        """Chunks with a missing primary go to the GPU in ONE sec_decode_batch_ex call (recover-only);
        a chunk whose k blocks are its k primaries needs no field arithmetic at all (zfec's fec_decode writes
        nothing for present primaries and easyfec joins them, /root/reference/storb/util/
        piece.py:196-197), so it is the join of its blocks, taken as views with no staging or
        PCIe round trip.  Returns per chunk either that chunk's bytes (per_chunk; with `views`
        the list of its buffers instead) or a list of buffers whose concatenation is the output."""
        gpu = []  # indices of chunks with a missing primary
        for i, item in enumerate(items):
            check_decode_item(*item)
            k, sharenums = item[0], item[3]
            if any(int(x) >= k for x in sharenums):
                gpu.append(i)
        # The GPU only recovers (SEC_F_RECOVER: zfec fec_decode's own output, the e missing
        # primaries, B bytes each, in primary order); the chunk is then the join of its present
        # primaries and those rows, so only e * B bytes per chunk come back over PCIe instead of
        # the whole reassembled chunk.
        rec, mv = {}, None
        if gpu:
            lost = [items[i] for i in gpu]
            sn, bo, _keep, slot0 = self._lay_out_blocks(lost)
            descs = np.zeros(len(gpu), dtype=DEC_DTYPE)
            total = 0
            for j, (i, it) in enumerate(zip(gpu, lost)):
                k, m, blocks, _sharenums, padlen = it
                descs[j] = (total, len(blocks[0]), padlen, slot0[j], k, m)
                rec[i] = total
                total += self._recovered_bytes(it)
            buf = self._out_buffer(total)
            self.decode_batch(descs, sn, bo, 0, buf, host=True, recover_only=True)
            mv = memoryview(buf)
        parts = []
        for i, it in enumerate(items):
            chunk = self._join_views(it, mv, rec.get(i))
            if per_chunk:
                parts.append(chunk if views else b"".join(chunk))
            else:
                parts.extend(chunk)
        return parts

def _check_blocks(k: int, m: int, blocks, sharenums, *, spares: bool, targets=(), padlen=None,
                  held_targets: bool = False) -> None:
    """The core of the check_*_item preconditions, in the library's order: the block count
    (exactly k, or with `spares` any n with k <= n <= m), equal lengths, 1 <= k <= m <= 256,
    sharenums and targets in [0, m) and all distinct (with `held_targets`: each of the two
    distinct in itself), and with `padlen` 0 <= padlen <= k*B."""
    n = len(blocks)
    if len(sharenums) != n or (n != k and not spares):
        raise Error(_lib.strerror(_lib.SEC_ENBLOCKS))
    B = len(blocks[0]) if blocks else 0
    for b in blocks:
        if len(b) != B:
            raise Error(_lib.strerror(_lib.SEC_EBLOCKLEN))
    if not (1 <= k <= m <= 256):
        raise Error(_lib.strerror(_lib.SEC_EKM))
    if not (k <= n <= m):
        raise Error(_lib.strerror(_lib.SEC_ENBLOCKS))
    nums = [int(x) for x in sharenums] + [int(x) for x in targets]
    if any(x < 0 or x >= m for x in nums):
        raise Error(_lib.strerror(_lib.SEC_ESHARENUM))
    if held_targets:
        groups = [nums[:n], nums[n:]]
    else:
        groups = [nums]
    if any(len(set(g)) != len(g) for g in groups):
        raise Error(_lib.strerror(_lib.SEC_EDUPSHARE))
    if padlen is not None and not (0 <= padlen <= k * B):
        raise Error(_lib.strerror(_lib.SEC_EPADLEN))


def check_decode_item(k: int, m: int, blocks, sharenums, padlen: int) -> None:
    """zfec's decode preconditions for one chunk (the library's own checks, raised before any
    GPU work): exactly k blocks and sharenums, equal lengths, 1 <= k <= m <= 256, sharenums in
    [0, m) and distinct, 0 <= padlen <= k*B.  Raises Error."""
    _check_blocks(k, m, blocks, sharenums, spares=False, padlen=padlen)


def check_repair_item(k: int, m: int, blocks, sharenums, targets) -> None:
    """The repair preconditions for one chunk (the library's own checks, raised before any GPU
    work): exactly k equal-length blocks and k sharenums, 1 <= k <= m <= 256, sources and
    targets in [0, m), all distinct, no target among the sources.  Raises Error."""
    _check_blocks(k, m, blocks, sharenums, spares=False, targets=targets)


def check_check_item(k: int, m: int, blocks, sharenums) -> None:
    """The check preconditions for one chunk (the library's own checks, raised before any GPU
    work): n equal-length blocks and n sharenums, 1 <= k <= m <= 256, k <= n <= m, sharenums in
    [0, m) and distinct.  Raises Error."""
    _check_blocks(k, m, blocks, sharenums, spares=True)


def check_decode_check_item(k: int, m: int, blocks, sharenums, padlen: int) -> None:
    """The decode + check preconditions for one chunk (the library's own checks, raised before any
    GPU work): n equal-length blocks and n sharenums, 1 <= k <= m <= 256, k <= n <= m, sharenums
    in [0, m) and distinct, 0 <= padlen <= k*B.  Raises Error."""
    _check_blocks(k, m, blocks, sharenums, spares=True, padlen=padlen)


def check_decode_correct_item(k: int, m: int, blocks, sharenums, padlen: int) -> None:
    """The decode + correct preconditions for one chunk: check_decode_check_item's, in its order
    (the library's own checks, raised before any GPU work).  Raises Error."""
    check_decode_check_item(k, m, blocks, sharenums, padlen)


def check_decode_ids_item(k: int, m: int, blocks, sharenums, padlen: int, ids) -> None:
    """The id-checked decode's preconditions for one chunk (``piece.decode_chunks_id_checked``):
    check_decode_check_item's, in its order (Error), then one 20-byte id per block (ValueError)."""
    check_decode_check_item(k, m, blocks, sharenums, padlen)
    if len(ids) != len(blocks):
        raise ValueError("one recorded id per block")
    if any(len(x) != 20 for x in ids):
        raise ValueError("a piece id is 20 bytes")


def check_repair_check_item(k: int, m: int, blocks, sharenums, targets) -> None:
    """The repair + check preconditions for one chunk (the library's own checks, raised before any
    GPU work): n equal-length blocks and n sharenums, 1 <= k <= m <= 256, k <= n <= m, sharenums
    and targets in [0, m), all distinct, no target among the blocks held.  Raises Error."""
    _check_blocks(k, m, blocks, sharenums, spares=True, targets=targets)


def check_repair_correct_item(k: int, m: int, blocks, sharenums, targets) -> None:
    """The repair + correct preconditions for one chunk: check_repair_check_item's, in its order,
    except that a target may be one of the blocks held (a heal target); the targets are distinct
    among themselves.  Raises Error."""
    _check_blocks(k, m, blocks, sharenums, spares=True, targets=targets, held_targets=True)


# -- matrices (host arithmetic; no device needed) ------------------------------
def check_locate(k: int, m: int, sharenums, column) -> int:
    """Which single entry explains an inconsistent column (sec_check_locate): sharenums = the n
    held block numbers, the first k the basis, column = their n bytes at one position (what a
    check returns).  -1: the column is a code word; i: changing entry i alone makes it one; -2:
    no single entry explains it (always so with fewer than two check rows)."""
    lib = _lib.load()
    sn = np.ascontiguousarray([int(x) for x in sharenums], dtype=np.int32)
    col = np.frombuffer(bytes(column), dtype=np.uint8)
    if col.size != sn.size:
        raise ValueError("check_locate: one column byte per sharenum")
    who = ctypes.c_int32(0)
    check(lib.sec_check_locate(int(k), int(m), _ptr(sn) or None, sn.size, _ptr(col) or None, ctypes.byref(who)), lib)
    return who.value


def check_correct(k: int, m: int, sharenums, column, max_errors: int = 0):
    """The code word within t entries of a column (sec_check_correct), the one-column model of the
    correcting calls: sharenums = the n held block numbers, the first k the basis, column = their
    n bytes at one position; t = min(max_errors, (n - k) // 2, 16), max_errors 0 = the code's
    limit.  Returns ``(fixed, nchanged)``: the n corrected bytes, and 0 for a code word, 1 .. t
    for that many entries changed, -2 for an open column (fixed = column)."""
    lib = _lib.load()
    sn = np.ascontiguousarray([int(x) for x in sharenums], dtype=np.int32)
    col = np.frombuffer(bytes(column), dtype=np.uint8)
    if col.size != sn.size:
        raise ValueError("check_correct: one column byte per sharenum")
    if max_errors < 0:
        raise ValueError("check_correct: max_errors is 0 (the code's limit) or a positive bound")
    fixed = np.zeros(max(col.size, 1), dtype=np.uint8)
    changed = ctypes.c_int32(0)
    check(lib.sec_check_correct(int(k), int(m), _ptr(sn) or None, sn.size, _ptr(col) or None, int(max_errors),
                                _ptr(fixed), ctypes.byref(changed)), lib)
    return fixed[:col.size].tobytes(), changed.value


def repair_method(k: int, m: int, sharenums, targets, B: int, avail=None) -> bool:
    """Whether a chunk of a repair (len(sharenums) == k) or a repair + check is eligible for the
    bit-sliced repair kernel (sec_repair_method): a bit-sliced shape, B >= 16, a target or a check
    row, the first k sharenums the data blocks 0 .. k-1 in any order, and every entry but data
    block k-1 readable to B (avail: one length per sharenum, or None = all B).  Eligibility alone:
    option ``SEC_CHECK_BS`` decides whether an eligible chunk takes that kernel."""
    lib = _lib.load()
    sn = np.ascontiguousarray([int(x) for x in sharenums], dtype=np.int32)
    tg = np.ascontiguousarray([int(x) for x in targets], dtype=np.int32)
    av = None if avail is None else np.ascontiguousarray([int(x) for x in avail], dtype=np.uint64)
    if av is not None and av.size != sn.size:
        raise ValueError("repair_method: one avail per sharenum")
    out = ctypes.c_int(0)
    check(lib.sec_repair_method(int(k), int(m), _ptr(sn) or None, sn.size, _ptr(tg) or None, tg.size, int(B),
                                None if av is None else (_ptr(av) or None), ctypes.byref(out)), lib)
    return bool(out.value)


def repair_matrix(k: int, m: int, sharenums, targets) -> bytes:
    """len(targets) x k bytes, row-major: block targets[r] = XOR_j row[r][j] * block
    sharenums[j] (sec_repair_matrix; columns in the order of `sharenums`)."""
    lib = _lib.load()
    sn = np.ascontiguousarray([int(x) for x in sharenums], dtype=np.int32)
    tg = np.ascontiguousarray([int(x) for x in targets], dtype=np.int32)
    if sn.size != k:
        raise Error(_lib.strerror(_lib.SEC_ENBLOCKS))
    out = np.zeros(max(tg.size * k, 1), dtype=np.uint8)
    check(lib.sec_repair_matrix(int(k), int(m), _ptr(sn) or None, _ptr(tg) or None, tg.size, _ptr(out)), lib)
    return out[: tg.size * k].tobytes()



def encode_matrix(k: int, m: int) -> bytes:
    """Rows k..m-1 of zfec's systematic encode matrix, as produced by libstorbec."""
    lib = _lib.load()
    out = np.zeros(max((m - k) * k, 1), dtype=np.uint8)
    check(lib.sec_encode_matrix(k, m, _ptr(out)))
    return out[: (m - k) * k].tobytes()


def choose_blocks(k: int, m: int, sharenums) -> list[int] | None:
    """Positions (ascending sharenum) of the k blocks to decode from when more are at hand
    (sec_decode_choose: every present primary, then parity rows from as few of the decode
    kernels' row groups as possible), or None when fewer than k distinct valid sharenums."""
    lib = _lib.load()
    sn = np.ascontiguousarray([int(x) for x in sharenums], dtype=np.int32)
    pick = np.zeros(max(k, 1), dtype=np.int32)
    rc = lib.sec_decode_choose(int(k), int(m), sn.size, _ptr(sn), _ptr(pick))
    if rc == _lib.SEC_ENBLOCKS:
        return None
    check(rc, lib)
    return pick[:k].tolist()


def pinned_bytes() -> tuple[int, int]:
    """(loaned, idle): the process's pinned staging memory lent to host-mode calls in progress,
    and kept idle for the next call (sec_host_pinned_bytes; contexts hold none between calls)."""
    lib = _lib.load()
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.sec_host_pinned_bytes(ctypes.byref(a), ctypes.byref(b))
    if rc:
        raise ECRuntimeError(f"sec_host_pinned_bytes: {rc}")
    return a.value, b.value


def option_names() -> list[str]:
    """Every context option the library knows (sec_option_name)."""
    lib = _lib.load()
    out, i = [], 0
    while (n := lib.sec_option_name(i)) is not None:
        out.append(n.decode())
        i += 1
    return out


def option_default(name: str) -> int:
    lib = _lib.load()
    v = ctypes.c_int64(0)
    check(lib.sec_ctx_get_option(None, name.encode(), ctypes.byref(v)))
    return v.value


def decode_matrix(k: int, m: int, sharenums) -> tuple[bytes, list[int]]:
    lib = _lib.load()
    sn = np.ascontiguousarray(sharenums, dtype=np.int32)
    if sn.size != k:
        raise Error(_lib.strerror(_lib.SEC_ENBLOCKS))
    out = np.zeros(k * k, dtype=np.uint8)
    idx = np.zeros(k, dtype=np.int32)
    check(lib.sec_decode_matrix(k, m, _ptr(sn), _ptr(out), _ptr(idx)))
    return out.tobytes(), idx.tolist()


_tls = threading.local()
_spread = {"devices": None, "next": 0}
_spread_lock = threading.Lock()


def spread_threads(devices) -> None:
    """Give each host thread that first asks for an engine without naming a device (and is not
    an EngineGroup worker) the next device of `devices`, round robin; None: every thread uses
    default_device().  A multi-threaded caller (the validator serves uploads and downloads on
    executor threads) then spreads its per-chunk calls over the GPUs.  A thread keeps the
    device it was given."""
    with _spread_lock:
        _spread["devices"] = None if devices is None else [int(d) for d in devices]
        _spread["next"] = 0


def _thread_device():
    devs = _spread["devices"]
    if devs is None:
        return None
    mine = getattr(_tls, "spread", None)
    if mine is not None and mine[0] is devs:
        return mine[1]
    with _spread_lock:
        d = devs[_spread["next"] % len(devs)]
        _spread["next"] += 1
    _tls.spread = (devs, d)
    return d


def get_engine(device: int | None = None) -> Engine:
    """The calling thread's engine for `device` (default: the engine of the EngineGroup worker
    this thread is, else STORB_EC_DEVICE / LOCAL_RANK / 0)."""
    if device is None:
        bound = getattr(_tls, "bound", None)
        if bound is not None:
            return bound
        device = _thread_device()
    dev = default_device() if device is None else int(device)
    engines = getattr(_tls, "engines", None)
    if engines is None:
        engines = _tls.engines = {}
    eng = engines.get(dev)
    if eng is None:
        eng = engines[dev] = Engine(dev)
    return eng


class EngineGroup:
    """Several devices driven from ONE process: one worker thread per
    entry of `devices`, each holding its own Engine (its own libstorbec context and streams on
    that device).  Chunks are independent (/root/reference/storb/validator/validator.py:1352-1431
    handles them one by one), so a batch is split into contiguous ranges balanced by bytes
    (``dist.partition``), each range runs on its worker, and the results come back in chunk
    order.  No collective and no peer traffic: every device reads and writes only its own share.

    ``devices=None`` uses every visible device.  An entry may repeat (``[0, 0]``: two contexts
    on one GPU, each with its own worker), so the split, the threads and the reassembly can be
    tested on a one-GPU box.  Inside a worker, ``get_engine()`` (no argument) returns that
    worker's engine, so the piece-level batch functions run unchanged on each share.

    ``engine_factory(device)`` (tests only) builds the per-worker engine instead of Engine.
    """

    def __init__(self, devices=None, engine_factory=None):
        from concurrent.futures import ThreadPoolExecutor

        if devices is None:
            devices = list(range(device_count()))
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise ECRuntimeError("EngineGroup: no HIP device available")
        make = engine_factory or (lambda d: Engine(d))
        self._workers = []
        self._engines = []
        try:
            for i, d in enumerate(self.devices):
                w = ThreadPoolExecutor(1, thread_name_prefix=f"storb_amd_dev{d}_{i}")
                self._workers.append(w)
                # the engine is created on its own worker thread and bound there
                self._engines.append(w.submit(self._bind, make, d).result())
        except BaseException:
            self.close()
            raise

    @staticmethod
    def _bind(make, d):
        eng = make(d)
        _tls.bound = eng
        return eng

    def __len__(self) -> int:
        return len(self.devices)

    @property
    def engines(self) -> list:
        return list(self._engines)

    def submit(self, i: int, fn, *args, **kw):
        """Run fn(*args, **kw) on worker i (whose ``get_engine()`` is engine i); a Future."""
        return self._workers[i].submit(fn, *args, **kw)

    def shares(self, sizes) -> list[tuple[int, int]]:
        """Contiguous [lo, hi) ranges of the items, one per worker, balanced by `sizes`."""
        from .dist import partition

        return partition(sizes, len(self.devices))

    def map_shares(self, fn, items, sizes) -> list:
        """fn(items[lo:hi], lo) on every worker's share at once; returns the per-share results
        in share (= item) order.  Every share runs to completion; then the error of the FIRST
        failing share (the one holding the earliest chunk) is raised, as a single-device call
        over the whole batch would raise for that chunk."""
        futs = [(self.submit(i, fn, items[lo:hi], lo) if hi > lo else None)
                for i, (lo, hi) in enumerate(self.shares(sizes))]
        res, err = [], None
        for f in futs:
            if f is None:
                res.append(None)
                continue
            try:
                res.append(f.result())
            except BaseException as e:  # noqa: BLE001 - re-raised below, in chunk order
                res.append(None)
                if err is None:
                    err = e
        if err is not None:
            raise err
        return res

    def sync(self) -> None:
        for f in [self.submit(i, e.sync) for i, e in enumerate(self._engines)]:
            f.result()

    def close(self) -> None:
        for i, w in enumerate(self._workers):
            eng = self._engines[i] if i < len(self._engines) else None
            if eng is not None:
                try:
                    w.submit(eng.close).result()
                except Exception:  # noqa: BLE001 - closing: best effort
                    pass
            w.shutdown(wait=True)
        self._workers, self._engines = [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
