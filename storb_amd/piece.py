"""Drop-in for /root/reference/storb/util/piece.py on the MI355X engine.

Same names, models, signatures and error behaviour as the reference module; the
Reed–Solomon arithmetic runs in libstorbec.so's HIP kernels instead of zfec.

Deliberate differences (documented in DESIGN.md §Boundary):

* ``decode_chunk`` passes each piece's true ``piece_idx`` as its zfec sharenum.  The
  reference passes list positions (piece.py:189-194), which returns wrong bytes whenever
  the pieces handed over are not exactly blocks 0..k-1.  On every input where the reference
  is correct both give identical bytes.  ``decode_chunk(..., positional_sharenums=True)``
  reproduces the reference's behaviour exactly.
* ``reconstruct_data`` decodes all chunks in ONE batched GPU call instead of one zfec call
  per chunk (same output; the "not enough pieces" ValueError is raised before any decode).
* handed more than k pieces, ``decode_chunk`` decodes from the k the library picks
  (``sec_decode_choose``: every present primary, then parity pieces from as few of the decode
  kernels' row groups as possible) instead of the first k (piece.py:189-191); any k distinct
  pieces give the same bytes, the choice only sets the decode's cost.
* the two ``print()`` calls per piece in ``encode_chunk`` (piece.py:140,151) are debug
  logs here.
* extra batch entry points ``encode_chunks`` / ``decode_chunks`` for callers that can hand
  over many chunks at once (the validator's upload loop, validator.py:1352-1431).
* ``repair_chunks`` / ``repair_pieces`` (no reference counterpart) regenerate lost pieces, data
  or parity, from a chunk's surviving pieces, with their piece ids on request: what a validator
  needs to seed a failed miner's pieces elsewhere without reconstructing and re-encoding.
* ``check_chunks`` / ``check_pieces`` (no reference counterpart) tell whether the pieces held of
  a chunk agree with each other and, with two pieces beyond k, which one does not: the code's own
  check, read once on the GPU, where the reference can only hash every piece.
* ``decode_chunks_checked`` / ``reconstruct_data_checked`` (no reference counterpart) reassemble
  the chunks and run that check in the same pass over the pieces: a download verified by the code
  word itself, where the validator hashes every fetched piece on one core (validator.py:1556-1604).
* ``repair_chunks_checked`` / ``repair_pieces_checked`` (no reference counterpart) regenerate lost
  pieces and run that check on every surviving piece in the same pass: a corrupt survivor is
  found, and named, before it is turned into new pieces.
* ``reconstruct_data_stream`` decodes window w+1 on a worker thread (its own HIP context)
  while the caller consumes window w's chunks; ``encode_chunks_stream`` does the same for the
  upload loop's produce/consume pattern (validator.py:1338-1446, 1630-1638).
* ``encode_chunk`` starts the SHA-1 of its pieces on a small thread pool (hashlib, as
  ``piece_hash``), data pieces while the parity is on the GPU; ``piece_hash(data)`` returns
  that digest when ``data`` is one of those very piece objects (identity, not equality), so
  the validator's ``piece_hash`` right after ``encode_chunk`` (validator.py:1081) does not
  hash serially.  Same digests either way; ``PREFETCH_PIECE_IDS = False`` turns it off.
* several GPUs in one process: the batch and stream functions take ``devices=`` (or the
  module default ``use_devices(...)``) and split their chunks over those devices
  (``engine.EngineGroup``: one worker thread and HIP context per device, chunks partitioned
  by bytes, results in chunk order).  Same bytes as one device.
"""

from __future__ import annotations

import ctypes
import functools
import hashlib
import logging
import math
import os
import platform
import threading
import typing
from collections import OrderedDict, deque
from collections.abc import Iterable, Iterator
from concurrent.futures import Future, ThreadPoolExecutor
from enum import IntEnum

import numpy as np
from pydantic import BaseModel, ConfigDict, Field

from .constants import MAX_PIECE_SIZE, MIN_PIECE_SIZE, PIECE_LENGTH_OFFSET, PIECE_LENGTH_SCALING
from .easyfec import Decoder, Encoder, Error
from .engine import (Engine, EngineGroup, _decoded_len, _decoded_starts, check_decode_check_item,
                     check_decode_correct_item, check_decode_ids_item, check_decode_item, check_locate,
                     check_repair_check_item, check_repair_correct_item, choose_blocks, device_count, get_engine,
                     spread_threads)

logger = logging.getLogger(__name__)

__all__ = [
    "PieceType", "Piece", "EncodedChunk", "ProcessedPieceInfo", "EncodedPieces", "piece_hash", "piece_length",
    "encode_chunk", "decode_chunk", "reconstruct_data", "reconstruct_data_stream", "encode_chunks",
    "decode_chunks", "chunk_shape", "piece_hashes", "encode_chunks_with_ids", "encode_chunks_with_tags",
    "encode_chunks_stream", "Encoder",
    "Decoder", "Error", "use_devices", "repair_chunks", "repair_pieces", "ChunkCheck", "check_chunks", "check_pieces",
    "decode_chunks_checked", "reconstruct_data_checked", "PieceCheckError", "repair_chunks_checked",
    "repair_pieces_checked", "ChunkIdCheck", "PieceIdError",
    "decode_chunks_id_checked", "reconstruct_data_id_checked", "reconstruct_data_stream_id_checked",
    "ChunkCorrection", "PieceCorrectionError", "decode_chunks_corrected", "reconstruct_data_corrected",
    "reconstruct_data_stream_corrected", "repair_chunks_corrected", "repair_pieces_corrected",
]

PREFETCH_PIECE_IDS = True  # encode_chunk hashes its pieces on a thread pool (see module doc)
# decode_chunk & co. handed more than k pieces decode from the k that sec_decode_choose picks
# (False: the first k in piece order, as the reference's piece.py:189-191; same bytes either way)
CHOOSE_BLOCKS = True
# ... for chunks of at least this many bytes.  The validator's pattern (encode_chunk, then
# piece_hash of every piece; tools/prefetch_study.py, profiles/r02_prefetch_study.json), us per
# chunk without / with: 256 KiB 217 / 217, 512 KiB 395 / 303, 1 MiB 744 / 411, 4 MiB 2754 / 918.
# Below 512 KiB each hand-off to a hashing thread (GIL + wake-up) costs what the hash saves.
PREFETCH_MIN_CHUNK = 512 << 10
# Pieces of at least this many bytes are copied on the thread pool too (_pieces_parallel):
# 8 MiB chunks (512 KiB pieces) 1.79 -> 2.1-2.7 GiB/s per chunk, 3.47 -> 4.1-5.3 streamed
# (tools/stream_rate.py); with 128 KiB pieces the hand-offs cost more than the copies (C1's
# 4 MiB object fell from 1236-1289 to 811 MiB/s per chunk, 1327-1469 to 868 streamed).
PARALLEL_COPY_MIN = 256 << 10
HASH_ON_FILL = True  # encode_chunk: each large piece's id hashing starts as soon as that piece is filled
# The pieces (easyfec's k slices + the parity) and their SHA-1 ids made by the library in one call
# (sec_encode_pieces: copies and OpenSSL SHA-1 on its own host threads, the data pieces while
# the GPU encodes), instead of Python slicing / numpy fills and hashlib on the thread pool.
# False: the round-4 paths (A/B: tools/c1_loopback.py, tools/small_call_profile.py).
HOST_PIECES = True

# The library never retunes the host process's allocator.  A validator that drops each chunk's
# pieces after sending them can keep glibc from trimming the freed heap back to the kernel (so the
# next chunk's pieces do not fault their pages in again) by starting the process with
# MALLOC_MMAP_THRESHOLD_=33554432 MALLOC_TRIM_THRESHOLD_=268435456 ("Host
# allocator"; measured in DESIGN.md §5 Round 4).
STREAM_WINDOW_BYTES = 64 << 20  # chunk bytes per GPU call in the *_stream pipelines
# encode_chunks_stream(piece_ids=True) over windows whose pieces are all >= PARALLEL_COPY_MIN:
# the ids come from the GPU SHA-1 kernel, fused after the window's encode, instead of hashlib
# on the thread pool, in windows of STREAM_WINDOW_IDS_BYTES (when window_bytes is not given).
# The kernel is one lane per piece, so a window's hashing takes about one piece's chain
# whatever the window size: 1 GiB object, 8 MiB chunks, zfec(16,24): 7.1 / 9.1 GiB/s with
# 256 / 512 MiB windows against 3.2-5.3 hashing on the host (profiles/r02_stream_rate.json).
# Round 5: the host ids from sec_encode_pieces (OpenSSL on the library's threads, HOST_PIECES)
# beat them at every window: 8.1-8.3 GiB/s at 64-256 MiB against 4.6-7.1 for GPU ids
# (profiles/r05_stream_rate.json), at the 64 MiB window (lower latency to the first chunk), so
# the GPU ids are off by default.
GPU_PIECE_IDS = False
STREAM_WINDOW_IDS_BYTES = 256 << 20
# Round 6: with the host ids, the parity pieces' ids from the GPU instead
# (sec_encode_pieces SEC_F_GPU_PARITY_IDS: the SHA-1 kernel on the device-resident parity, one
# lane per piece, while the library's host threads hash only the data pieces), in windows of
# STREAM_WINDOW_PARITY_IDS_BYTES so that hundreds of parity pieces share one chain time.
# Measured on the 1 GiB upload (8 MiB chunks, zfec(16,24); profiles/r06_parity_ids.json): 3.96 /
# 6.21 / 6.70 / 7.13 GiB/s at 64 / 256 / 512 / 1024 MiB windows against 5.97 / 6.82 / 6.82 / 6.91
# with every id on the host threads.  Taking a third of the hashing off the host buys nothing:
# the upload is bound by the host's memory work on the fresh piece buffers (first touch, copies),
# and the GPU path adds a staged 512 MiB slab per window.  Off (F1 closed as host-only for the
# upload; the flag stays in the ABI, tested).
GPU_PARITY_IDS = False
STREAM_WINDOW_PARITY_IDS_BYTES = 512 << 20
STREAM_WORKERS = 4  # single-thread workers (one engine each) the *_stream pipelines are spread over


class PieceType(IntEnum):  # piece.py:21-23
    Data = 0
    Parity = 1


class Piece(BaseModel):  # piece.py:26-33
    model_config = ConfigDict(use_enum_values=True)

    chunk_idx: int
    piece_idx: int
    piece_type: PieceType
    data: bytes


class EncodedChunk(BaseModel):  # piece.py:36-43
    pieces: list[Piece] = Field(default=None)
    chunk_idx: int
    k: int  # Number of data blocks
    m: int  # Total blocks (data + parity)
    chunk_size: int
    padlen: int
    original_chunk_size: int


class ProcessedPieceInfo(Piece):  # piece.py:46-47
    piece_id: typing.Optional[str] = Field(default=None)


class EncodedPieces(BaseModel):  # piece.py:50-51
    pieces: list[Piece]


_pools: dict = {}
_pools_lock = threading.Lock()
# at most this many hash-pool threads (piece copies and hashlib SHA-1); STORB_HASH_WORKERS overrides
HASH_WORKERS = int(os.environ.get("STORB_HASH_WORKERS", "16") or 16)


def _cgroup_cpus() -> int | None:
    """The CPU quota of this process's cgroup (cgroup v2 cpu.max "quota period"), rounded up, or
    None when unlimited or unknown: a container's CPU share is often a quota, not an affinity
    mask, and threads beyond it are throttled rather than run."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota == "max":
            return None
        return max(1, -(-int(quota) // int(period)))
    except (OSError, ValueError):
        return None


def _usable_cpus() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 2
    q = _cgroup_cpus()
    return min(n, q) if q else n


def _pool(name: str) -> ThreadPoolExecutor:
    """Module thread pools: "hash" (piece copies and hashlib SHA-1, which release the GIL) and
    "stream<i>" (_stream_pool)."""
    with _pools_lock:
        p = _pools.get(name)
        if p is None:
            # half the CPUs: SHA-1 on 8 threads of a 16-CPU quota ran at 15.3 GB/s, on 16 at 14.1, and
            # the per-chunk upload at 4.9 against 3.4 GiB/s (r03_upload_ab.jsonl)
            n = 1 if name.startswith("stream") else max(1, min(HASH_WORKERS, _usable_cpus() // 2))
            p = _pools[name] = ThreadPoolExecutor(n, thread_name_prefix=f"storb_amd_{name}")
        return p


_stream_rr = [0]


def _stream_pool() -> ThreadPoolExecutor:
    """The worker a new *_stream pipeline runs its GPU calls on: one of STREAM_WORKERS
    single-thread workers (each with its own engine), round robin.  A stream keeps its windows
    on its one worker (window w + 1 decodes while the caller consumes window w), and concurrent
    streams (downloads served on several request threads) do not queue behind one another.
    (All windows of one stream on 4 shared workers measured 2-7 % slower: tools/stream_rate.py
    --ab, profiles/r03_stream_ab.json.)"""
    with _pools_lock:
        i = _stream_rr[0] % max(1, STREAM_WORKERS)
        _stream_rr[0] += 1
    return _pool(f"stream{i}")


_ONE = "one"  # devices=_ONE: the calling thread's own engine (inside an EngineGroup worker: its device)
_default_devices = None  # use_devices()
_groups: dict = {}


def use_devices(devices) -> None:
    """Module default of the batch and stream functions' ``devices=``: None (one device, the
    calling thread's engine: the default), "all" (every visible device), a list of device ids,
    or an EngineGroup.  A single-process validator (/root/reference/storb/validator/
    __main__.py:10-24) calls this once at start-up and then drives every GPU through the
    unchanged names: encode_chunks / decode_chunks / reconstruct_data split each batch by bytes
    over the devices, the *_stream pipelines send windows round robin to them, and the per-chunk
    calls (encode_chunk, decode_chunk) of different host threads are spread over them
    (engine.spread_threads)."""
    global _default_devices
    grp = _group(devices) if devices is not None else None
    _default_devices = grp
    spread_threads(grp.devices if grp is not None else None)


def _group(devices):
    """The EngineGroup for a ``devices=`` argument (None: the module default), or None for the
    one-device path.  Groups are created once per device list and kept (each holds a HIP
    context and a worker thread per device)."""
    if devices is _ONE:
        return None
    if devices is None:
        devices = _default_devices
        if devices is None:
            return None
    if isinstance(devices, EngineGroup):
        return devices
    key = "all" if isinstance(devices, str) and devices == "all" else tuple(int(d) for d in devices)
    with _pools_lock:
        g = _groups.get(key)
        if g is None:
            g = _groups[key] = EngineGroup(list(range(device_count())) if key == "all" else list(key))
    return g


def _sha1_hex(b) -> str:
    return hashlib.sha1(b).hexdigest()


class _PieceIdMemo:
    """Digests encode_chunk started for its pieces, keyed by the piece's bytes object.  A hit
    requires the very object (``is``), which the memo keeps alive while it holds it, so an id
    cannot be reused under it.

    Retention is bounded (the validator hashes a chunk's pieces right after its encode_chunk,
    validator.py:1380 -> 1081, so nothing older is ever asked for): entries leave on first use,
    when they belong to an encode_chunk call more than `keep_calls` calls ago, or oldest-first
    past `max_bytes`.  A call whose pieces alone exceed `max_bytes` is not prefetched.  When
    `idle_calls` calls in a row were evicted with none of their ids asked for (a caller that
    does not hash, or hashes copies), prefetching pauses, except for one probe call in every
    `probe_every`, so a caller that does not use the ids costs almost no hashing."""

    def __init__(self, max_bytes: int = 128 << 20, keep_calls: int = 2, idle_calls: int = 4, probe_every: int = 64):
        self.max_bytes = max_bytes
        self.keep_calls = keep_calls
        self.idle_calls = idle_calls
        self.probe_every = probe_every
        self._d: OrderedDict = OrderedDict()  # id -> (obj, future, call number)
        self._bytes = 0
        self._call = 0
        self._calls: dict[int, list[int]] = {}  # call number -> [entries held, ids taken]
        self._idle = 0  # consecutive evicted calls with no id taken
        self._lock = threading.Lock()

    def _drop(self, c: int, taken: bool) -> None:
        st = self._calls.get(c)
        if st is None:
            return
        st[0] -= 1
        st[1] += taken
        if st[0] <= 0:  # that call's last entry
            del self._calls[c]
            self._idle = 0 if st[1] else self._idle + 1

    def _evict_oldest(self) -> None:
        _, (o, f, c) = self._d.popitem(last=False)
        self._bytes -= len(o)
        f.cancel()  # not started yet: no hashing for an id nobody will ask for
        self._drop(c, False)

    def begin(self, nbytes: int) -> int | None:
        """Start an encode_chunk call's prefetch of `nbytes` of pieces: its call number, or None
        when it should not prefetch."""
        with self._lock:
            self._call += 1
            c = self._call
            if nbytes > self.max_bytes:
                return None
            if self._idle >= self.idle_calls and c % self.probe_every:
                return None
            while self._d and (next(iter(self._d.values()))[2] <= c - self.keep_calls
                               or self._bytes + nbytes > self.max_bytes):
                self._evict_oldest()
            return c

    def put(self, obj: bytes, fut: Future, call: int) -> None:
        with self._lock:
            old = self._d.pop(id(obj), None)
            if old is not None:  # the same object twice: counted once
                self._bytes -= len(old[0])
                self._drop(old[2], False)
            self._d[id(obj)] = (obj, fut, call)
            self._bytes += len(obj)
            self._calls.setdefault(call, [0, 0])[0] += 1
            while self._bytes > self.max_bytes and self._d:
                self._evict_oldest()

    def take(self, obj):
        with self._lock:
            e = self._d.get(id(obj))
            if e is None or e[0] is not obj:
                return None
            del self._d[id(obj)]
            self._bytes -= len(obj)
            self._idle = 0
            self._drop(e[2], True)
        try:
            return e[1].result()
        except Exception:  # noqa: BLE001 - cancelled or failed: hash here instead
            return None

    def held_bytes(self) -> int:
        with self._lock:
            return self._bytes


_memo = _PieceIdMemo()


def piece_hash(data: bytes) -> str:
    """SHA-1 hex digest of a piece (piece.py:54-68)."""
    d = _memo.take(data) if type(data) is bytes else None
    return d if d is not None else hashlib.sha1(data).hexdigest()


def piece_hashes(datas: typing.Sequence[bytes]) -> list[str]:
    """``[piece_hash(d) for d in datas]`` computed by the GPU SHA-1 kernel in one call."""
    if not datas:
        return []
    return [d.hex() for d in get_engine().sha1_host(list(datas))]


def piece_length(content_length: int, min_size: int = MIN_PIECE_SIZE, max_size: int = MAX_PIECE_SIZE) -> int:
    """Piece size for a content length, clamped to [min_size, max_size] (piece.py:71-100)."""
    exponent = int((math.log2(content_length) * PIECE_LENGTH_SCALING) + PIECE_LENGTH_OFFSET)
    length = 1 << exponent
    if length < min_size:
        return min_size
    elif length > max_size:
        return max_size
    return length


def chunk_shape(chunk_size: int) -> tuple[int, int, int, int]:
    """(k, m, B, padlen) encode_chunk uses for a chunk of `chunk_size` bytes (piece.py:116-134)."""
    piece_size = piece_length(chunk_size)
    expected_data_pieces = math.ceil(chunk_size / piece_size)
    expected_parity_pieces = math.ceil(expected_data_pieces / 2)
    k = expected_data_pieces
    m = k + expected_parity_pieces
    zfec_chunk_size = (chunk_size + (k - 1)) // k
    padlen = (zfec_chunk_size * k) - chunk_size
    return k, m, zfec_chunk_size, padlen


def _split(chunk, k: int, B: int) -> list[bytes]:
    mv = memoryview(chunk).cast("B")
    prim = [bytes(mv[i * B:(i + 1) * B]) for i in range(k)]
    if len(prim[-1]) != B:
        prim[-1] = prim[-1] + b"\x00" * (B - len(prim[-1]))
    return prim


# New bytes objects filled in place before anyone else sees them: storb_amd/_hostbytes.py.
from ._hostbytes import _FILL_IN_PLACE, _PendingBytes, _finalize, _new_bytes  # noqa: E402,F401


def _fill(dst: np.ndarray, src: np.ndarray) -> None:
    dst[:len(src)] = src
    if len(src) < len(dst):
        dst[len(src):] = 0


def _hash_filled(fill: Future | None, view: np.ndarray, piece) -> str:
    """SHA-1 hex of a piece once its fill (an earlier task of the same FIFO pool) is done.

    `piece` is the bytes object (or _PendingBytes) `view` looks into.  The task holds it so the
    piece outlives the hash: on CPython `view` is a raw view of the object's buffer with no
    reference to it, and the memo may drop its own reference (eviction) while this task is
    queued or running, after the caller dropped the piece too."""
    if fill is not None:
        fill.result()
    assert piece is not None
    return hashlib.sha1(view).hexdigest()


def _pieces_parallel(chunks: list, shapes: list, digests: bool = False, hash_ids: bool = False):
    """Every chunk's m pieces as bytes (k zero-padded data slices, then the parity): one GPU
    call for all chunks; the piece copies run on the hash pool, the data slices beside the GPU
    call.  Returns once every piece is filled.  ``digests=True``: (pieces, ids), ids[i] = the
    piece ids (SHA-1 hex) of chunk i's m pieces, hashed on the GPU after the encode.
    ``hash_ids=True``: (pieces, futures), futures[i][j] = the hashlib SHA-1 hex of piece j of
    chunk i, each started as soon as that piece is filled (data pieces beside the GPU call) and
    still running when this returns."""
    _short_middle(shapes, chunks)
    hp = _pool("hash")
    out, jobs, hfut = [], [], []
    for c, (k, m, B, _) in zip(chunks, shapes):
        src = np.frombuffer(memoryview(c).cast("B"), dtype=np.uint8)
        ps, views = [], []
        for j in range(k):
            b, v = _new_bytes(B)
            ps.append(b)
            views.append(v)
            jobs.append(hp.submit(_fill, v, src[j * B:min((j + 1) * B, len(src))]))
        out.append(ps)
        if hash_ids:  # queued behind this chunk's data fills (FIFO), so they never wait long
            hfut.append([hp.submit(_hash_filled, f, v, b) for f, v, b in zip(jobs[-k:], views, ps)])
    # staged, not page-locked: the pool is faulting in the new pieces meanwhile, and locking
    # waits on the same memory-map lock (6.4 against 0.55 ms for one 8 MiB chunk on MI355X,
    # profiles/r03_upload_ab.jsonl)
    res = get_engine().encode_host_raw(list(chunks), _km(shapes), digests=digests, staged=True)
    buf, layout = res[0], res[1]
    for i, (ps, (o, B, p)) in enumerate(zip(out, layout)):
        pj = []
        for r in range(p):
            b, v = _new_bytes(B)
            ps.append(b)
            if hash_ids:  # the pool's queue holds the data pieces' hashes: the caller, idle
                # until its pieces exist, copies the parity itself (r03_upload_timeline.json)
                _fill(v, buf[o + r * B:o + (r + 1) * B])
                hfut[i].append(hp.submit(_hash_filled, None, v, b))
            else:
                jobs.append(hp.submit(_fill, v, buf[o + r * B:o + (r + 1) * B]))
                pj.append((jobs[-1], v))
    ids = _hex_rows(res[2], shapes) if digests else None
    for f in jobs:  # the pieces must be complete before anyone sees them (and buf is reused)
        f.result()
    if not _FILL_IN_PLACE:
        out = [[_finalize(p) for p in ps] for ps in out]
    if hash_ids:
        return out, hfut
    return (out, ids) if digests else out


class _Done:
    """A finished result in the memo's future slot (the library computed the digest already)."""

    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v

    def result(self):
        return self.v

    def cancel(self):
        return False


def _encode_pieces(chunks: list, shapes: list, ids: bool, gpu_parity_ids: bool = False, tag_key=None):
    """Every chunk's m pieces as new bytes objects, filled by the library (sec_encode_pieces:
    the k data slices, zero-padded, then the parity), and with `ids` each piece's SHA-1 hex
    (the library's host threads, OpenSSL: hashlib's bytes; with `gpu_parity_ids` the parity
    pieces' from the GPU SHA-1 kernel).  Returns (pieces, ids or None); with `tag_key` (a
    ``ModKey`` ready for tags) also, third, each chunk's m APDP tag values as ints, computed by
    the GPU call that encodes the chunk (sec_encode_pieces_tags)."""
    objs, addrs = [], []
    for (k, m, B, _) in shapes:
        row = []
        for _ in range(m):
            b, v = _new_bytes(B)
            row.append((b, v))
            addrs.append(v.ctypes.data if B else 0)
        objs.append(row)
    dig = np.empty(max(20 * len(addrs), 1), dtype=np.uint8) if ids else None
    # staged, not page-locked: the library's threads fault in the new pieces meanwhile, and locking
    # waits on the same memory-map lock (6.4 against 0.55 ms for one 8 MiB chunk on MI355X,
    # profiles/r03_upload_ab.jsonl)
    tagged = {}
    if tag_key is not None:
        tagged = {"tags": np.empty(max(256 * len(addrs), 1), dtype=np.uint8), "tag_key": tag_key}
    get_engine().encode_pieces_into(chunks, _km(shapes), addrs, dig, staged=True,
                                    gpu_parity_ids=ids and gpu_parity_ids, **tagged)
    pieces = [[_finalize(b) for b, _ in row] for row in objs]
    hexes = _hex_rows(dig, shapes) if ids else None
    if tag_key is not None:
        return pieces, hexes, Engine._tag_ints(tagged["tags"], [m for (_, m, _, _) in shapes])
    return pieces, hexes


def _shapes(chunks) -> list:
    """``chunk_shape`` of every chunk, after encode_chunk's ValueError for an empty one."""
    shapes = []
    for c in chunks:
        n = len(c)
        piece_length(n)  # same ValueError as encode_chunk for n == 0
        shapes.append(chunk_shape(n))
    return shapes


def _km(shapes) -> list:
    return [(k, m) for (k, m, _, _) in shapes]


def _short_middle(shapes, chunks) -> None:
    for c, (k, m, B, _) in zip(chunks, shapes):
        if k > 1 and (k - 1) * B > len(c):  # easyfec's short middle slice, as Encoder.encode
            raise Error("Precondition violation: Input blocks are required to be all the same length.")


def _hex_rows(dig: np.ndarray, shapes) -> list[list[str]]:
    """A digest array (20 bytes per piece, chunk-major) as per-chunk rows of SHA-1 hex."""
    hx, rows, f = dig.tobytes().hex(), [], 0
    for (_, m, _, _) in shapes:
        rows.append([hx[40 * (f + j):40 * (f + j + 1)] for j in range(m)])
        f += m
    return rows


def _build(chunk_idx: int, k: int, m: int, B: int, padlen: int, n: int, blocks: list[bytes]) -> EncodedChunk:
    pieces = []
    for i, block in enumerate(blocks):
        piece_type = PieceType.Data if i < k else PieceType.Parity
        logger.debug("Encoding piece %d with length %d", i, len(block))
        pieces.append(Piece(piece_type=piece_type, data=block, chunk_idx=chunk_idx, piece_idx=i))
    return EncodedChunk(pieces=pieces, chunk_idx=chunk_idx, k=k, m=m, chunk_size=B, padlen=padlen,
                        original_chunk_size=n)


def _split_and_parity(chunks, shapes, parity) -> list[list[bytes]]:
    """Every chunk's m pieces: its k data slices cut on the caller's thread, then its parity."""
    return [_split(c, k, B) + par for c, (k, _, B, _), par in zip(chunks, shapes, parity)]


def _build_all(first_chunk_idx: int, chunks, shapes, pieces) -> list[EncodedChunk]:
    """``_build`` of every chunk from its pieces; chunk i gets index first_chunk_idx + i."""
    return [_build(first_chunk_idx + i, k, m, B, padlen, len(c), ps)
            for i, (c, (k, m, B, padlen), ps) in enumerate(zip(chunks, shapes, pieces))]


def encode_chunk(chunk: bytes, chunk_idx: int) -> EncodedChunk:
    """Encode one chunk into k data + ceil(k/2) parity pieces (piece.py:103-166)."""
    chunk_size = len(chunk)
    piece_size = piece_length(chunk_size)  # ValueError for an empty chunk, as the reference
    logger.debug("[encode_chunk] chunk %d: %d bytes, piece_size = %d", chunk_idx, chunk_size, piece_size)
    k, m, B, padlen = chunk_shape(chunk_size)
    enc_ = Encoder(k, m)
    if HOST_PIECES:  # pieces and (prefetched) ids from the library in one call
        call = _memo.begin(m * B) if PREFETCH_PIECE_IDS else None
        _short_middle([(k, m, B, padlen)], [chunk])
        pieces, ids = _encode_pieces([chunk], [(k, m, B, padlen)], call is not None)
        if call is not None:
            for b, h in zip(pieces[0], ids[0]):
                _memo.put(b, _Done(h), call)
        return _build(chunk_idx, k, m, B, padlen, chunk_size, pieces[0])
    call = _memo.begin(m * B) if PREFETCH_PIECE_IDS and chunk_size >= PREFETCH_MIN_CHUNK else None
    if call is None:
        encoded_pieces = enc_.encode(chunk)
    else:  # piece ids hashed on the pool: data pieces beside the GPU call, parity right after
        hp = _pool("hash")
        if B >= PARALLEL_COPY_MIN and HASH_ON_FILL:  # large pieces: copies on the pool too, each hashed once filled
            pieces, hf = _pieces_parallel([chunk], [(k, m, B, padlen)], hash_ids=True)
            encoded_pieces, futs = pieces[0], hf[0]
        elif B >= PARALLEL_COPY_MIN:  # (A/B: every piece hashed after all are filled)
            encoded_pieces = _pieces_parallel([chunk], [(k, m, B, padlen)])[0]
            futs = [hp.submit(_sha1_hex, b) for b in encoded_pieces]
        else:
            prim = _split(chunk, k, B)
            futs = [hp.submit(_sha1_hex, b) for b in prim]
            parity = enc_.encode_parity(chunk) if m > k and B else [b""] * (m - k)
            futs += [hp.submit(_sha1_hex, b) for b in parity]
            encoded_pieces = prim + parity
        for b, f in zip(encoded_pieces, futs):
            _memo.put(b, f, call)
    enc = _build(chunk_idx, k, m, B, padlen, chunk_size, encoded_pieces)
    logger.debug("[encode_chunk] chunk %d: k=%d, m=%d, encoded %d blocks", chunk_idx, k, m, len(enc.pieces))
    return enc


def encode_chunks(chunks: typing.Sequence[bytes], first_chunk_idx: int = 0, *, devices=None) -> list[EncodedChunk]:
    """Batched ``encode_chunk`` over many chunks in ONE GPU call; chunk i gets index first+i.

    devices (or the module default set by ``use_devices``): the chunks are split by bytes over
    those devices' workers (``EngineGroup``), one GPU call per device, results in chunk order."""
    shapes = _shapes(chunks)
    if not chunks:
        return []
    grp = _group(devices)
    if grp is not None:
        parts = grp.map_shares(lambda share, lo: encode_chunks(share, first_chunk_idx + lo, devices=_ONE),
                               list(chunks), [len(c) for c in chunks])
        return [ec for p in parts if p for ec in p]
    if HOST_PIECES:
        _short_middle(shapes, chunks)
        pieces, _ = _encode_pieces(list(chunks), shapes, False)
    elif min(B for (_, _, B, _) in shapes) >= PARALLEL_COPY_MIN:  # piece copies in parallel
        pieces = _pieces_parallel(list(chunks), shapes)
    else:
        pieces = _split_and_parity(chunks, shapes, get_engine().encode_host(list(chunks), _km(shapes)))
    return _build_all(first_chunk_idx, chunks, shapes, pieces)


def encode_chunks_with_ids(chunks: typing.Sequence[bytes],
                           first_chunk_idx: int = 0) -> tuple[list[EncodedChunk], list[list[str]]]:
    """``encode_chunks`` plus every piece's id (``piece_hash``, the SHA-1 the validator computes
    right after encoding, validator.py:1081), hashed on the GPU while the pieces are still there."""
    shapes = _shapes(chunks)
    if not chunks:
        return [], []
    parity, digs = get_engine().encode_host(list(chunks), _km(shapes), digests=True)
    out = _build_all(first_chunk_idx, chunks, shapes, _split_and_parity(chunks, shapes, parity))
    return out, [[d.hex() for d in ds] for ds in digs]


def encode_chunks_with_tags(chunks: typing.Sequence[bytes], challenge_system, first_chunk_idx: int = 0, *,
                            piece_ids: bool = True):
    """``encode_chunks`` plus, from the same pass over each chunk, every piece's APDP tag (what
    the validator's ``process_tag`` computes per stored piece, validator.py:945-947) and, with
    ``piece_ids``, every piece's id: the chunk is staged to the GPU once, and its pieces are not
    staged again for ``generate_tags``.

    challenge_system: an ``apdp.ChallengeSystem`` (anything with its ``tag_key()`` and
    ``wrap_tags(values)``).  Returns (chunks, ids or None, tags): tags[i] = the ``APDPTag`` of
    each of chunk i's m pieces, equal to ``challenge_system.generate_tags`` over those pieces'
    data; chunks and ids as ``encode_chunks_with_ids``.  Errors as ``encode_chunks``."""
    shapes = _shapes(chunks)
    if not chunks:
        return [], ([] if piece_ids else None), []
    _short_middle(shapes, chunks)
    pieces, ids, values = _encode_pieces(list(chunks), shapes, piece_ids, GPU_PARITY_IDS,
                                         tag_key=challenge_system.tag_key())
    return (_build_all(first_chunk_idx, chunks, shapes, pieces), ids,
            [challenge_system.wrap_tags(v) for v in values])


def _sharenums(encoded_chunk: EncodedChunk, positional: bool):
    k = encoded_chunk.k
    pieces = encoded_chunk.pieces
    if positional:  # the reference's own behaviour, piece.py:189-194
        if len(pieces) > k:
            use = pieces[:k]
            return [p.data for p in use], list(range(k))
        return [p.data for p in pieces], list(range(len(pieces)))
    if len(pieces) > k and CHOOSE_BLOCKS:
        # the validator hands over every piece it fetched (validator.py:1556-1604, 1631): decode
        # from the k the library picks (every present primary, then parity rows of one decode
        # row group where possible: the fused syndrome kernel), not the first k; same bytes
        pick = choose_blocks(k, encoded_chunk.m, [p.piece_idx for p in pieces])
        if pick is not None:
            use = [pieces[i] for i in pick]
            return [p.data for p in use], [p.piece_idx for p in use]
    use = pieces[:k] if len(pieces) > k else pieces
    return [p.data for p in use], [p.piece_idx for p in use]


def decode_chunk(encoded_chunk: EncodedChunk, *, positional_sharenums: bool = False) -> bytes:
    """Decode one chunk from its pieces (piece.py:169-198); see module doc for sharenums."""
    blocks, sharenums = _sharenums(encoded_chunk, positional_sharenums)
    decoder = Decoder(encoded_chunk.k, encoded_chunk.m)
    return decoder.decode(blocks, sharenums, encoded_chunk.padlen)


def decode_chunks(encoded_chunks: typing.Sequence[EncodedChunk], *, positional_sharenums: bool = False,
                  devices=None) -> bytes:
    """Batched ``decode_chunk``: the concatenation of every chunk's bytes, one GPU call.

    devices (or the module default set by ``use_devices``): the chunks are split by bytes over
    those devices' workers, each share decoded by its own device straight into its slice of the
    result (one copy, as on one device)."""
    items = []
    for ch in encoded_chunks:
        if not (1 <= ch.k <= ch.m <= 256):
            raise Error(f"Precondition violation: 1 <= k <= m <= 256 required (k={ch.k}, m={ch.m})")
        blocks, sharenums = _sharenums(ch, positional_sharenums)
        B = len(blocks[0]) if blocks else 0
        if not (0 <= ch.padlen <= ch.k * B):
            # out-of-range padlen: keep easyfec's slicing semantics on the per-chunk path
            return b"".join(decode_chunk(c, positional_sharenums=positional_sharenums) for c in encoded_chunks)
        items.append((ch.k, ch.m, blocks, sharenums, ch.padlen))
    if not items:
        return b""
    grp = _group(devices)
    if grp is None:
        return get_engine().decode_host(items)
    for it in items:  # zfec's preconditions for every chunk before any device starts
        check_decode_item(*it)
    starts = _decoded_starts(items)
    out, view = _new_bytes(starts[-1])

    def share(its, lo):
        return get_engine().decode_host_into(its, view[starts[lo]:starts[lo + len(its)]])

    grp.map_shares(share, items, [_decoded_len(it) for it in items])
    return _finalize(out)


def _by_chunk(pieces: Iterable[Piece]) -> dict[int, list[Piece]]:
    """The pieces handed over, per ``chunk_idx``, in the order given."""
    by_chunk: dict[int, list[Piece]] = {}
    for p in pieces:
        by_chunk.setdefault(p.chunk_idx, []).append(p)
    return by_chunk


def _take_pieces(chunk: EncodedChunk, by_chunk: dict) -> None:
    """``reconstruct_data``'s step for one chunk: it gets its pieces in ascending piece_idx, or the
    reference's ValueError."""
    relevant = sorted(by_chunk.get(chunk.chunk_idx, []), key=lambda p: p.piece_idx)
    if len(relevant) < chunk.k:
        raise ValueError(f"Not enough pieces to reconstruct chunk {chunk.chunk_idx}")
    chunk.pieces = relevant


def _group_pieces(pieces: list[Piece], chunks: list[EncodedChunk]) -> None:
    """``reconstruct_data``'s grouping: ``_take_pieces`` for every chunk, in order."""
    by_chunk = _by_chunk(pieces)
    for chunk in chunks:
        _take_pieces(chunk, by_chunk)


def reconstruct_data(pieces: list[Piece], chunks: list[EncodedChunk], *, devices=None) -> bytes:
    """Reconstruct the original bytes from pieces (piece.py:201-236), one batched decode (per
    device with `devices` / ``use_devices``: see decode_chunks)."""
    _group_pieces(pieces, chunks)
    return decode_chunks(chunks, devices=devices)


def repair_chunks(chunks: typing.Sequence[EncodedChunk], targets=None, *, piece_ids: bool = False) -> list[list[Piece]]:
    """Regenerate lost pieces, data or parity, from each chunk's surviving pieces: one GPU call.

    ``chunk.pieces`` holds the survivors, at least k of them (with more, the k that
    ``choose_blocks`` picks are read).  targets: per chunk the piece indices to regenerate, or
    None for every ``piece_idx`` in ``range(m)`` that is absent (``targets=None``: that for all
    chunks).  Returns, per chunk, the regenerated pieces in target order, each keeping the
    chunk's ``chunk_idx``; with ``piece_ids=True`` they are ``ProcessedPieceInfo`` carrying the
    piece's id (its SHA-1, hashed on the GPU while the piece is there), to be checked against
    the id recorded at upload.  No reference counterpart: piece.py would reconstruct the chunk
    and encode it again."""
    if targets is not None and len(targets) != len(chunks):
        raise ValueError("repair_chunks: one target list (or None) per chunk")
    items = []
    for i, ch in enumerate(chunks):
        held = _held_pieces(ch, "repair")
        items.append(_basis_item(ch, held, _targets_of(targets, i, ch, held)))
    if not items:
        return []
    res = get_engine().repair_host(items, digests=piece_ids)
    blocks, digs = res if piece_ids else (res, None)
    return _repaired_pieces(chunks, [it[4] for it in items], blocks, digs)


def repair_pieces(chunk: EncodedChunk, targets=None, *, piece_ids: bool = False) -> list[Piece]:
    """``repair_chunks`` for one chunk: its lost pieces (`targets`, default every absent one)."""
    return repair_chunks([chunk], None if targets is None else [targets], piece_ids=piece_ids)[0]


class ChunkCheck(BaseModel):
    """What ``check_chunks`` found for one chunk."""

    chunk_idx: int
    checked: int  # pieces checked (the distinct pieces held)
    consistent: bool  # every held piece agrees with the others
    first_bad_offset: typing.Optional[int] = None  # lowest byte offset at which a piece disagrees
    bad_piece_idx: list[int] = Field(default_factory=list)  # the pieces named corrupt so far
    located: bool = False  # bad_piece_idx is every corrupt piece: the rest was checked consistent


def _check_item(ch: EncodedChunk, held: list[Piece]):
    """(k, m, blocks, sharenums) of a check over `held` (ascending piece_idx, at least k): the
    basis is the pick of ``choose_blocks`` (every held primary first, so with all primaries held
    the check rows are plain encode rows), the other pieces are the check rows."""
    basis = held[:ch.k]
    if len(held) > ch.k:
        pick = choose_blocks(ch.k, ch.m, [p.piece_idx for p in held])
        if pick is not None:
            basis = [held[j] for j in pick]
    took = {p.piece_idx for p in basis}
    use = basis + [p for p in held if p.piece_idx not in took]
    return ch.k, ch.m, [p.data for p in use], [p.piece_idx for p in use]


def _basis_item(ch: EncodedChunk, held: list[Piece], tail):
    """(k, m, blocks, sharenums, tail) over the basis of ``_check_item`` alone: the k pieces a
    decode or a repair reads, and its padlen or targets."""
    k, m, blocks, sharenums = _check_item(ch, held)
    return k, m, blocks[:k], sharenums[:k], tail


def _targets_of(targets, i: int, ch: EncodedChunk, held: list[Piece]) -> list[int]:
    """The pieces to regenerate for chunk i: targets[i], or every ``piece_idx`` absent from `held`."""
    tg = targets[i] if targets is not None and targets[i] is not None else None
    if tg is None:
        have = {p.piece_idx for p in held}
        tg = [t for t in range(ch.m) if t not in have]
    return [int(t) for t in tg]


def _repaired_pieces(chunks, tgs, blocks, digs) -> list[list[Piece]]:
    """Per chunk its regenerated pieces in target order (tgs[i]), from the blocks, and with `digs`
    the digests, that the engine returned: ``ProcessedPieceInfo`` with ids, else ``Piece``."""
    out = []
    for i, ch in enumerate(chunks):
        row = []
        for j, t in enumerate(tgs[i]):
            kind = PieceType.Data if t < ch.k else PieceType.Parity
            if digs is not None:
                row.append(ProcessedPieceInfo(chunk_idx=ch.chunk_idx, piece_idx=t, piece_type=kind,
                                              data=blocks[i][j], piece_id=digs[i][j].hex()))
            else:
                row.append(Piece(chunk_idx=ch.chunk_idx, piece_idx=t, piece_type=kind, data=blocks[i][j]))
        out.append(row)
    return out


def _begin_check(ch: EncodedChunk, what: str, held: list, out: list) -> list[Piece]:
    """A check's bookkeeping for one more chunk: its held pieces appended to `held`, and a
    ``ChunkCheck`` that says consistent until the rounds say otherwise to `out`."""
    use = _held_pieces(ch, what)
    held.append(use)
    out.append(ChunkCheck(chunk_idx=ch.chunk_idx, checked=len(use), consistent=True))
    return use


def _held_pieces(ch: EncodedChunk, what: str) -> list[Piece]:
    """The distinct pieces held of a chunk in ascending piece_idx (the first of any repeat)."""
    if not (1 <= ch.k <= ch.m <= 256):
        raise Error(f"Precondition violation: 1 <= k <= m <= 256 required (k={ch.k}, m={ch.m})")
    have: dict[int, Piece] = {}
    for p in ch.pieces or []:
        have.setdefault(p.piece_idx, p)
    use = sorted(have.values(), key=lambda p: p.piece_idx)
    if len(use) < ch.k:
        raise ValueError(f"Not enough pieces to {what} chunk {ch.chunk_idx}")
    return use


def _check_rounds(chunks, held: list[list[Piece]], out: list[ChunkCheck], locate: bool, first=None) -> None:
    """The check, locate, re-check rounds of ``check_chunks`` over `held` (per chunk its distinct
    pieces, ascending; a located piece is taken out of its list), filling `out`.  first: the
    ``(items, results)`` of round one when the caller has run it already (the fused decode +
    check of ``decode_chunks_checked``); the later rounds are plain checks, one call each."""
    todo = list(range(len(chunks)))  # chunks checked in the next call
    first_round = True
    while todo:
        if first_round and first is not None:
            items, res = first
        else:
            items = [_check_item(chunks[i], held[i]) for i in todo]
            res = get_engine().check_host(items)
        again = []
        for i, it, (first_at, _bad, column) in zip(todo, items, res):
            ck = out[i]
            if first_round:
                ck.consistent = first_at is None
                ck.first_bad_offset = first_at
            if first_at is None:
                ck.located = not first_round
                continue
            if not locate:
                continue
            who = check_locate(it[0], it[1], it[3], column) if len(it[3]) - it[0] >= 2 else -2
            if who < 0:  # no single piece explains the column: bad_piece_idx is what was named so far
                continue
            ck.bad_piece_idx.append(it[3][who])
            held[i] = [p for p in held[i] if p.piece_idx != it[3][who]]
            again.append(i)
        todo = again
        first_round = False


def check_chunks(chunks: typing.Sequence[EncodedChunk], *, locate: bool = True) -> list[ChunkCheck]:
    """Whether each chunk's held pieces agree with each other, and which piece does not: GPU calls
    that read every held piece once and hash nothing.

    ``chunk.pieces`` holds at least k pieces.  k of them (``choose_blocks``' pick) predict every
    other one, which is compared with what is held: any corruption confined to at most n - k of
    the n held pieces is detected with certainty (a chunk with exactly k pieces has nothing to
    compare and is reported consistent).  With ``locate`` an inconsistent chunk goes on: the bytes
    of all pieces at the first bad offset name the one piece whose change explains them
    (``check_locate``; needs two pieces beyond k), the chunk is checked again without that piece
    (all such re-checks of a round in one call), and so on until the rest is consistent
    (``located=True``: ``bad_piece_idx`` are the corrupt pieces, ready for
    ``repair_pieces(rest, targets=bad_piece_idx)``) or no single piece explains what is left
    (``located=False``, ``bad_piece_idx`` what was named so far).  No reference counterpart: the
    reference's only integrity check is the SHA-1 piece id."""
    out: list[ChunkCheck] = []
    held: list[list[Piece]] = []
    for ch in chunks:
        _begin_check(ch, "check", held, out)
    _check_rounds(chunks, held, out, locate)
    return out


def check_pieces(chunk: EncodedChunk, *, locate: bool = True) -> ChunkCheck:
    """``check_chunks`` for one chunk."""
    return check_chunks([chunk], locate=locate)[0]


class PieceCheckError(ValueError):
    """``reconstruct_data_checked``: some chunk's held pieces disagree and the corrupt ones could
    not be named, so its bytes cannot be trusted.  ``checks``: every chunk's ``ChunkCheck``."""

    def __init__(self, message: str, checks: list[ChunkCheck]):
        super().__init__(message)
        self.checks = checks


def decode_chunks_checked(encoded_chunks: typing.Sequence[EncodedChunk], *,
                          locate: bool = True) -> tuple[bytes, list[ChunkCheck]]:
    """``decode_chunks`` and ``check_chunks`` in one pass over the pieces: the concatenation of
    every chunk's bytes, and per chunk what the code word says about the pieces held.

    Every distinct piece held of a chunk is used, ordered as ``check_chunks`` orders them:
    ``choose_blocks``' pick is decoded from and predicts the others, which are compared with what
    is held; ONE fused GPU call reads each piece once (``Engine.decode_check_host``) and hashes
    nothing.  Chunks reported inconsistent go on through ``check_chunks``' rounds (locate, re-check
    without the named piece, in batches); those that end up ``located`` are decoded again from
    their remaining pieces, all in one ``decode_host`` call, and spliced into the result.

    The bytes of a chunk are trustworthy exactly when its ``ChunkCheck`` is ``consistent or
    located``; otherwise they are what its first k pieces decode to, corrupt piece included.
    What "trustworthy" means: corruption confined to at most n - k of a chunk's n held pieces is
    always detected, and a chunk with exactly k pieces is not checked at all; more than n - k
    pieces altered together can form another code word, which only the recorded piece ids
    exclude.  ``devices=`` / ``EngineGroup`` splitting is not provided: one device, one call; the
    streaming form is ``reconstruct_data_stream_checked``.  With every piece of a chunk held,
    ``choose_blocks`` picks the k data pieces (every present primary first, for every shape), so
    the fused call may take the one-pass bit-sliced check kernel (option ``SEC_CHECK_BS``)."""
    chunks = list(encoded_chunks)
    out: list[ChunkCheck] = []
    held: list[list[Piece]] = []
    items = []
    for ch in chunks:
        items.append(_check_item(ch, _begin_check(ch, "reconstruct", held, out)))
    if not chunks:
        return b"", []
    full = [it + (ch.padlen,) for it, ch in zip(items, chunks)]
    for it in full:  # every chunk's preconditions before any device work
        check_decode_check_item(*it)
    data, res = get_engine().decode_check_host(full)
    _check_rounds(chunks, held, out, locate, first=(items, res))
    redo = [i for i, ck in enumerate(out) if ck.located]
    if not redo:
        return data, out
    # from the pieces that passed the last re-check
    fixed = get_engine().decode_host([_basis_item(chunks[i], held[i], chunks[i].padlen) for i in redo])
    starts = _decoded_starts(full)
    parts, at, f = [], 0, 0
    view = memoryview(data)
    for i in redo:
        n = starts[i + 1] - starts[i]
        parts.append(view[at:starts[i]])
        parts.append(memoryview(fixed)[f:f + n])
        f += n
        at = starts[i + 1]
    parts.append(view[at:])
    return b"".join(parts), out


def repair_chunks_checked(chunks: typing.Sequence[EncodedChunk], targets=None, *, piece_ids: bool = False,
                          locate: bool = True) -> tuple[list[list[Piece]], list[ChunkCheck]]:
    """``repair_chunks`` and ``check_chunks`` in one pass over the surviving pieces: per chunk the
    regenerated pieces, and what the code word says about the pieces they were made from.

    Every distinct piece held of a chunk is used, ordered as ``check_chunks`` orders them:
    ``choose_blocks``' pick is repaired from and predicts the others, which are compared with what
    is held; ONE fused GPU call reads each piece once (``Engine.repair_check_host``).  targets: as
    ``repair_chunks``' (default: every absent ``piece_idx``); ``piece_ids`` as there.  Chunks
    reported inconsistent go on through ``check_chunks``' rounds (locate, re-check without the
    named piece, in batches); those that end up ``located`` are repaired again from the pieces
    that passed, all in one ``repair_host`` call, which regenerates the requested targets followed
    by the pieces named in ``bad_piece_idx``, in the order named: the caller then holds a full
    healthy set.

    The pieces of a chunk are trustworthy exactly when its ``ChunkCheck`` is ``consistent or
    located``; otherwise they are what its first k pieces give, corrupt piece included.  What
    "trustworthy" means: corruption confined to at most n - k of a chunk's n held pieces is always
    detected, and a chunk with exactly k pieces is not checked at all; more than n - k pieces
    altered together can form another code word, which only the recorded piece ids exclude.
    ``devices=`` / ``EngineGroup`` splitting is not provided: one device, one call.
    ``repair_chunks`` is unchanged."""
    chunks = list(chunks)
    if targets is not None and len(targets) != len(chunks):
        raise ValueError("repair_chunks_checked: one target list (or None) per chunk")
    out: list[ChunkCheck] = []
    held: list[list[Piece]] = []
    items, tgs = [], []
    for i, ch in enumerate(chunks):
        use = _begin_check(ch, "repair", held, out)
        items.append(_check_item(ch, use))
        tgs.append(_targets_of(targets, i, ch, use))
    if not chunks:
        return [], []
    full = [it + (tg,) for it, tg in zip(items, tgs)]
    for it in full:  # every chunk's preconditions before any device work
        check_repair_check_item(*it)
    res = get_engine().repair_check_host(full, digests=piece_ids)
    blocks, digs, checks = res if piece_ids else (res[0], None, res[1])
    _check_rounds(chunks, held, out, locate, first=(items, checks))
    redo = [i for i, ck in enumerate(out) if ck.located]
    if redo:
        again = []
        for i in redo:  # from the pieces that passed the last re-check
            tgs[i] = tgs[i] + [b for b in out[i].bad_piece_idx if b not in tgs[i]]
            again.append(_basis_item(chunks[i], held[i], tgs[i]))
        fixed = get_engine().repair_host(again, digests=piece_ids)
        fblocks, fdigs = fixed if piece_ids else (fixed, None)
        for j, i in enumerate(redo):
            blocks[i] = fblocks[j]
            if piece_ids:
                digs[i] = fdigs[j]
    return _repaired_pieces(chunks, tgs, blocks, digs), out


def repair_pieces_checked(chunk: EncodedChunk, targets=None, *, piece_ids: bool = False,
                          locate: bool = True) -> tuple[list[Piece], ChunkCheck]:
    """``repair_chunks_checked`` for one chunk."""
    pieces, checks = repair_chunks_checked([chunk], None if targets is None else [targets], piece_ids=piece_ids,
                                           locate=locate)
    return pieces[0], checks[0]


def reconstruct_data_checked(pieces: list[Piece], chunks: list[EncodedChunk]) -> tuple[bytes, list[ChunkCheck]]:
    """``reconstruct_data`` verified by the code word in the same pass (``decode_chunks_checked``
    over every piece handed over, grouped as ``reconstruct_data`` groups them).  Raises
    ``ValueError("Not enough pieces to reconstruct chunk N")`` as ``reconstruct_data`` does, before
    any decode, and ``PieceCheckError`` (carrying ``.checks``) when some chunk is neither
    consistent nor located; otherwise returns the bytes, all trustworthy in
    ``decode_chunks_checked``'s sense, and the checks.  One device, one call: objects too large
    for that stream through ``reconstruct_data_stream_checked``."""
    _group_pieces(pieces, chunks)
    data, checks = decode_chunks_checked(chunks)
    bad = [ck.chunk_idx for ck in checks if not (ck.consistent or ck.located)]
    if bad:
        raise PieceCheckError(f"Held pieces disagree and no corrupt piece could be named in chunk(s) {bad}", checks)
    return data, checks


def _windows(chunks, nbytes, size_of) -> Iterator[list]:
    """Consecutive groups of chunks totalling at most `nbytes` (at least one chunk each)."""
    win, acc = [], 0
    for c in chunks:
        sz = size_of(c)
        if win and acc + sz > nbytes:
            yield win
            win, acc = [], 0
        win.append(c)
        acc += sz
    if win:
        yield win


def _stream_windows(pieces, items, window_bytes, chunk_of):
    """The set-up of the reconstruct_data_stream* family: (the pieces per chunk, `items` in windows
    of about `window_bytes`, default STREAM_WINDOW_BYTES, of output); chunk_of(item) = its chunk."""
    wb = STREAM_WINDOW_BYTES if window_bytes is None else window_bytes
    return _by_chunk(pieces), _windows(items, wb, lambda it: max(chunk_of(it).original_chunk_size, 1))


def _decode_window(window: list, by_chunk: dict):
    """Worker side of reconstruct_data_stream: (per-chunk bytes, error) for one window.  The
    window's chunks up to the first one that cannot be decoded are decoded (one GPU call for
    those with a missing primary); that chunk's error is returned, to be raised in order."""
    items, err = [], None
    for chunk in window:
        try:
            _take_pieces(chunk, by_chunk)
            blocks, sharenums = _sharenums(chunk, False)
            B = len(blocks[0]) if blocks else 0
            if not (1 <= chunk.k <= chunk.m <= 256) or not (0 <= chunk.padlen <= chunk.k * B):
                # easyfec's own slicing semantics: the per-chunk path, decoded here
                items.append(("bytes", decode_chunk(chunk)))
                continue
            item = (chunk.k, chunk.m, blocks, sharenums, chunk.padlen)
            check_decode_item(*item)  # zfec's preconditions, before any chunk of the window decodes
        except Exception as e:  # noqa: BLE001 - re-raised on the caller's thread after the chunks before it
            err = e
            break
        items.append(item)
    try:
        batch = [it for it in items if it[0] != "bytes"]
        outs = iter(get_engine().decode_host_chunks(batch) if batch else [])
        res = [it[1] if it[0] == "bytes" else next(outs) for it in items]
    except Exception as e:  # noqa: BLE001 - a device failure: nothing of the window is trusted
        return [], e
    return res, err


def reconstruct_data_stream(pieces: list[Piece], chunks: list[EncodedChunk], *,
                            window_bytes: int | None = None, devices=None) -> Iterator[bytes]:
    """Yield the reconstructed bytes chunk by chunk (piece.py:239-263).

    Chunks go in windows of about `window_bytes` (default STREAM_WINDOW_BYTES) of output; each
    window is one batched decode on a worker thread, and window w+1's decode runs while the
    caller consumes window w (the validator streams them into the HTTP response,
    validator.py:1630-1638).  With `devices` (or ``use_devices``) the windows go round robin to
    those devices' workers, two per device in flight.  Chunks come out in order; a chunk without
    enough pieces raises the reference's ValueError when the stream reaches it, after every
    earlier chunk."""
    by_chunk, wins = _stream_windows(pieces, chunks, window_bytes, lambda c: c)
    for outs, err in _pipeline(wins, _decode_window, (by_chunk,), _group(devices)):
        yield from outs
        if err is not None:
            raise err


def _decode_verified_window(window: list, by_chunk: dict, decode):
    """Worker side of reconstruct_data_stream_checked and reconstruct_data_stream_id_checked: (per-chunk
    ``(bytes, check)``, error) for one window of ``(chunk, *more)`` rows.  The window's rows up to the
    first chunk without enough pieces go through one ``decode(chunks, *more columns)``:
    ``decode_chunks_checked`` (one fused GPU call, then the locate rounds and the second decode of
    the located chunks) or ``decode_chunks_id_checked``, all confined to this window; that chunk's
    error is returned, to be raised in order."""
    good, err = [], None
    for row in window:
        try:
            _take_pieces(row[0], by_chunk)
        except ValueError as e:
            err = e
            break
        good.append(row)
    if not good:
        return [], err
    try:
        data, checks = decode(*map(list, zip(*good)))
    except Exception as e:  # noqa: BLE001 - a precondition or device failure: nothing of the window is trusted
        return [], e
    view, at, pairs = memoryview(data), 0, []
    for (chunk, *_), ck in zip(good, checks):
        n = _decoded_len((chunk.k, chunk.m, [chunk.pieces[0].data], (), chunk.padlen))
        pairs.append((bytes(view[at:at + n]), ck))
        at += n
    return pairs, err


def _stream_verified(pieces, rows, window_bytes, decode, trusted, refuse) -> Iterator[tuple]:
    """The generator of both verified streams: `rows` of ``(chunk, *more)`` in windows through
    ``_decode_verified_window`` on the stream worker, each chunk yielded as ``(bytes, check)`` once
    trusted(check); else refuse(check, the checks seen so far) is raised."""
    by_chunk, wins = _stream_windows(pieces, rows, window_bytes, lambda row: row[0])
    seen: list = []
    for pairs, err in _pipeline(wins, _decode_verified_window, (by_chunk, decode), None):
        for data, ck in pairs:
            seen.append(ck)
            if not trusted(ck):
                raise refuse(ck, list(seen))
            yield data, ck
        if err is not None:
            raise err


def reconstruct_data_stream_checked(pieces: list[Piece], chunks: list[EncodedChunk], *,
                                    window_bytes: int | None = None) -> Iterator[tuple[bytes, ChunkCheck]]:
    """``reconstruct_data_checked``'s contract, delivered as ``reconstruct_data_stream`` delivers:
    yield ``(bytes, ChunkCheck)`` chunk by chunk, in order.

    Chunks go in windows of about `window_bytes` (default STREAM_WINDOW_BYTES) of output.  Each
    window is one ``decode_chunks_checked`` on the stream worker (one fused GPU call over every
    piece handed over, then the locate rounds and the second decode of located chunks, confined to
    that window), and window w+1 runs while the caller consumes window w.  With every piece of a
    chunk held, ``choose_blocks`` picks its k data pieces (every present primary is taken first,
    for every shape), so the check rows are zfec's own parity rows and the fused call may take the
    one-pass bit-sliced check kernel (``Engine.check_methods``, option ``SEC_CHECK_BS``).

    A yielded chunk's bytes are trustworthy in ``decode_chunks_checked``'s sense: its check is
    ``consistent or located``.  Errors are raised when the stream reaches the chunk, after every
    earlier chunk has been yielded: ``ValueError("Not enough pieces to reconstruct chunk N")``, and
    ``PieceCheckError`` (``.checks``: the checks of the chunks seen so far, that chunk's last) for
    a chunk that is neither consistent nor located.  Closing the generator early cancels the
    windows not yet started.  One device: ``devices=`` is not provided, as for the whole check
    family."""
    yield from _stream_verified(
        pieces, list(zip(chunks)), window_bytes, decode_chunks_checked, lambda ck: ck.consistent or ck.located,
        lambda ck, seen: PieceCheckError(
            f"Held pieces disagree and no corrupt piece could be named in chunk {ck.chunk_idx}", seen))


class ChunkCorrection(BaseModel):
    """What ``decode_chunks_corrected`` found, and put right, for one chunk."""

    chunk_idx: int
    checked: int  # pieces checked (the distinct pieces held)
    consistent: bool  # every held piece agrees with the others: nothing was corrected
    first_bad_offset: typing.Optional[int] = None  # lowest byte offset at which the pieces disagree
    corrected_positions: int = 0  # offsets at which changing one piece's byte gave a code word
    open_positions: int = 0  # offsets that disagree and that no single piece's change explains
    first_open_offset: typing.Optional[int] = None  # the lowest of them
    # piece_idx -> offsets at which that piece was the one changed; the keys are the pieces to
    # heal: repair_pieces_corrected(chunk) returns each of them whole and corrected, from the same
    # held pieces, even where fewer than k of them are undamaged
    damaged: dict[int, int] = Field(default_factory=dict)


def _note_correction(ck: ChunkCorrection, piece_idx, found) -> None:
    """One chunk's result of a correcting engine call (``(first, first_open, corrected, open,
    hits)``, hits in the order of `piece_idx`) into its ``ChunkCorrection``."""
    first, first_open, corrected, opened, hits = found
    ck.consistent = first is None
    ck.first_bad_offset = first
    ck.corrected_positions = corrected
    ck.open_positions = opened
    ck.first_open_offset = first_open
    ck.damaged = {int(idx): h for idx, h in zip(piece_idx, hits) if h}


def _per_offset(max_errors) -> str:
    return "one piece per offset" if max_errors == 1 else "the pieces correctable per offset"


class PieceCorrectionError(ValueError):
    """``reconstruct_data_corrected``: at some offset of some chunk the held pieces disagree and no
    single piece's change explains it, so those bytes cannot be trusted.  ``checks``: every chunk's
    ``ChunkCorrection``."""

    def __init__(self, message: str, checks: list[ChunkCorrection]):
        super().__init__(message)
        self.checks = checks


def _max_errors_kw(max_errors) -> dict:
    """The engine keyword of a piece-layer ``max_errors`` (None: the code's limit, the engine's 0).
    The default, 1, passes nothing: the call is the one made before the keyword existed."""
    if max_errors is None:
        return {"max_errors": 0}
    if int(max_errors) < 1:
        raise ValueError("max_errors is None (the code's limit) or a positive bound")
    return {} if int(max_errors) == 1 else {"max_errors": int(max_errors)}


def decode_chunks_corrected(encoded_chunks: typing.Sequence[EncodedChunk], *,
                            max_errors: int | None = 1) -> tuple[bytes, list[ChunkCorrection]]:
    """``decode_chunks_checked`` that corrects instead of dropping: the concatenation of every
    chunk's bytes with one corrupt piece per byte offset put right, and per chunk what was found.

    Round one is ``decode_chunks_checked``'s fused call (``Engine.decode_check_host``), with the
    pieces ordered as there, so a clean download costs exactly what it costs there.  The chunks
    it reports inconsistent, and only those, go through ONE ``Engine.decode_correct_host`` call,
    which judges every byte offset's column of pieces as ``check_locate`` does and decodes from
    the corrected column; their bytes are spliced into the result.  Where ``decode_chunks_checked``
    names one piece per round and gives up once fewer than two spare pieces are left, damage to any
    number of pieces is corrected here as long as no two of them are damaged at the same offset.

    A chunk's bytes are trustworthy exactly when its ``open_positions`` is 0.  What that means:
    with two or more pieces beyond k, an offset where at most one piece is wrong is always put
    right; with three or more, an offset where two are wrong is always reported open; with exactly
    two, two wrong bytes at one offset may be attributed to a third piece, which only the recorded
    piece ids exclude.  With fewer than two spare pieces nothing can be corrected and every bad
    offset is open.  One device, one call; the streaming form is
    ``reconstruct_data_stream_corrected``.

    max_errors (default 1: all of the above, byte for byte): how many wrong pieces per byte offset
    are put right, t = min(max_errors, r // 2, 16) with r the pieces held beyond k; None is the
    code's limit.  Round one is unchanged, so clean input launches nothing new; the second call
    then judges a column as ``engine.check_correct`` does.  At most t wrong bytes at an offset are
    always put right; more than t and at most r - t are always reported open; beyond r - t the
    column may be corrected to another code word, which only the recorded piece ids exclude.  An
    offset with several pieces changed counts once in ``corrected_positions`` and once per piece
    in ``damaged``."""
    kw = _max_errors_kw(max_errors)
    chunks = list(encoded_chunks)
    out: list[ChunkCorrection] = []
    full = []
    for ch in chunks:
        use = _held_pieces(ch, "reconstruct")
        out.append(ChunkCorrection(chunk_idx=ch.chunk_idx, checked=len(use), consistent=True))
        full.append(_check_item(ch, use) + (ch.padlen,))
    if not chunks:
        return b"", []
    for it in full:  # every chunk's preconditions before any device work
        check_decode_correct_item(*it)
    data, res = get_engine().decode_check_host(full)
    redo = [i for i, (first_at, _bad, _column) in enumerate(res) if first_at is not None]
    if not redo:
        return data, out
    fixed, cor = get_engine().decode_correct_host([full[i] for i in redo], **kw)
    starts = _decoded_starts(full)
    parts, at, f = [], 0, 0
    view = memoryview(data)
    for i, found in zip(redo, cor):
        _note_correction(out[i], full[i][3], found)
        n = starts[i + 1] - starts[i]
        parts.append(view[at:starts[i]])
        parts.append(memoryview(fixed)[f:f + n])
        f += n
        at = starts[i + 1]
    parts.append(view[at:])
    return b"".join(parts), out


def reconstruct_data_corrected(pieces: list[Piece], chunks: list[EncodedChunk], *,
                               max_errors: int | None = 1) -> tuple[bytes, list[ChunkCorrection]]:
    """``reconstruct_data`` with one corrupt piece per byte offset put right
    (``decode_chunks_corrected`` over every piece handed over, grouped as ``reconstruct_data``
    groups them).  Raises ``ValueError("Not enough pieces to reconstruct chunk N")`` as
    ``reconstruct_data`` does, before any decode, and ``PieceCorrectionError`` (carrying
    ``.checks``) when some chunk has open positions; otherwise returns the bytes, all trustworthy
    in ``decode_chunks_corrected``'s sense, and the checks.  max_errors: as
    ``decode_chunks_corrected``'s (None: up to (pieces beyond k) // 2 corrupt pieces per offset)."""
    _group_pieces(pieces, chunks)
    data, checks = decode_chunks_corrected(chunks, max_errors=max_errors)
    bad = [ck.chunk_idx for ck in checks if ck.open_positions]
    if bad:
        raise PieceCorrectionError(f"Held pieces disagree beyond what {_per_offset(max_errors)} explains "
                                   f"in chunk(s) {bad}", checks)
    return data, checks


def reconstruct_data_stream_corrected(pieces: list[Piece], chunks: list[EncodedChunk], *,
                                      window_bytes: int | None = None,
                                      max_errors: int | None = 1) -> Iterator[tuple[bytes, ChunkCorrection]]:
    """``reconstruct_data_corrected``'s contract, delivered as ``reconstruct_data_stream_checked``
    delivers: yield ``(bytes, ChunkCorrection)`` chunk by chunk, in order, each window one
    ``decode_chunks_corrected`` on the stream worker.  ``PieceCorrectionError`` (``.checks``: the
    checks of the chunks seen so far, that chunk's last) is raised when the stream reaches a chunk
    with open positions, after every earlier chunk has been yielded.  max_errors: as
    ``decode_chunks_corrected``'s."""
    _max_errors_kw(max_errors)  # a bad bound is refused here, not on the stream worker
    decode = decode_chunks_corrected if max_errors == 1 else functools.partial(decode_chunks_corrected,
                                                                               max_errors=max_errors)
    yield from _stream_verified(
        pieces, list(zip(chunks)), window_bytes, decode, lambda ck: not ck.open_positions,
        lambda ck, seen: PieceCorrectionError(
            f"Held pieces disagree beyond what {_per_offset(max_errors)} explains in chunk {ck.chunk_idx}", seen))


def repair_chunks_corrected(chunks: typing.Sequence[EncodedChunk], targets=None, *, piece_ids: bool = False,
                            heal: bool = True,
                            max_errors: int | None = 1) -> tuple[list[list[Piece]], list[ChunkCorrection]]:
    """``repair_chunks_checked`` that corrects instead of dropping: per chunk the regenerated
    pieces, the damaged held pieces healed, and what was found.

    Round one is ``repair_chunks_checked``'s fused call (``Engine.repair_check_host``), with the
    pieces ordered as there, so clean input costs exactly what it costs there and launches nothing
    new.  The chunks it reports inconsistent, and only those, go through ONE
    ``Engine.repair_correct_host`` call, which judges every byte offset's column of pieces as
    ``check_locate`` does and makes every piece from the corrected column.  targets: as
    ``repair_chunks``' (default: every absent ``piece_idx``; explicit targets must be absent).
    With ``heal`` that call's targets are followed by every held piece, so damage is healed even
    where fewer than k undamaged pieces are left, as long as no two pieces are damaged at the same
    offset; healing is never in place, the held pieces are not written.

    A chunk returns its requested targets in order, then, with ``heal``, the held pieces whose
    hit count is nonzero, in ascending ``piece_idx``, each the whole corrected piece (regenerated
    copies of undamaged held pieces are dropped); with ``piece_ids`` every returned piece is a
    ``ProcessedPieceInfo`` carrying the id the GPU hashed from it.  The ``ChunkCorrection`` is
    filled as ``decode_chunks_corrected`` fills it; with ``heal`` the keys of ``damaged`` are
    exactly the healed pieces returned.

    A chunk's pieces are trustworthy exactly when its ``open_positions`` is 0.  What that means:
    with two or more pieces beyond k, an offset where at most one piece is wrong is always put
    right; with three or more, an offset where two are wrong is always reported open; with exactly
    two, two wrong bytes at one offset may be attributed to a third piece, which only the recorded
    piece ids exclude.  With fewer than two spare pieces nothing can be corrected and every bad
    offset is open; at an open offset a piece holds what the first k pieces as held predict.
    One device, one call; ``repair_chunks`` and ``repair_chunks_checked`` are unchanged.

    max_errors (default 1: all of the above, byte for byte): as ``decode_chunks_corrected``'s.  With
    t = min(max_errors, r // 2, 16), None the code's limit, up to t wrong pieces per offset are put
    right and every piece is made from the column with all of them corrected; more than t and at
    most r - t are always open; beyond r - t a column may be corrected to another code word."""
    kw = _max_errors_kw(max_errors)
    chunks = list(chunks)
    if targets is not None and len(targets) != len(chunks):
        raise ValueError("repair_chunks_corrected: one target list (or None) per chunk")
    out: list[ChunkCorrection] = []
    full = []
    for i, ch in enumerate(chunks):
        use = _held_pieces(ch, "repair")
        out.append(ChunkCorrection(chunk_idx=ch.chunk_idx, checked=len(use), consistent=True))
        full.append(_check_item(ch, use) + (_targets_of(targets, i, ch, use),))
    if not chunks:
        return [], []
    for it in full:  # every chunk's preconditions before any device work
        check_repair_check_item(*it)
    res = get_engine().repair_check_host(full, digests=piece_ids)
    blocks, digs, checks = res if piece_ids else (res[0], None, res[1])
    tgs = [it[4] for it in full]
    redo = [i for i, (first_at, _bad, _column) in enumerate(checks) if first_at is not None]
    if redo:
        again = [full[i][:4] + (tgs[i] + (sorted(full[i][3]) if heal else []),) for i in redo]
        for it in again:
            check_repair_correct_item(*it)
        fixed = get_engine().repair_correct_host(again, digests=piece_ids, **kw)
        fblocks, fdigs, cor = fixed if piece_ids else (fixed[0], None, fixed[1])
        for j, i in enumerate(redo):
            ck = out[i]
            _note_correction(ck, full[i][3], cor[j])
            asked = again[j][4]
            keep = [q for q, t in enumerate(asked) if q < len(tgs[i]) or t in ck.damaged]
            tgs[i] = [asked[q] for q in keep]
            blocks[i] = [fblocks[j][q] for q in keep]
            if piece_ids:
                digs[i] = [fdigs[j][q] for q in keep]
    return _repaired_pieces(chunks, tgs, blocks, digs), out


def repair_pieces_corrected(chunk: EncodedChunk, targets=None, *, piece_ids: bool = False, heal: bool = True,
                            max_errors: int | None = 1) -> tuple[list[Piece], ChunkCorrection]:
    """``repair_chunks_corrected`` for one chunk."""
    pieces, checks = repair_chunks_corrected([chunk], None if targets is None else [targets], piece_ids=piece_ids,
                                             heal=heal, max_errors=max_errors)
    return pieces[0], checks[0]


class ChunkIdCheck(BaseModel):
    """What ``decode_chunks_id_checked`` found for one chunk."""

    chunk_idx: int
    checked: int  # pieces hashed (the distinct pieces held)
    ok: bool  # every held piece matches its recorded id
    bad_piece_idx: list[int] = Field(default_factory=list)  # the pieces whose SHA-1 is not their id
    decodable: bool = True  # at least k held pieces match: the chunk's bytes come from such pieces only


class PieceIdError(ValueError):
    """``reconstruct_data_id_checked``: fewer than k of some chunk's held pieces match their recorded
    ids, so its bytes cannot be trusted.  ``checks``: every chunk's ``ChunkIdCheck``."""

    def __init__(self, message: str, checks: list[ChunkIdCheck]):
        super().__init__(message)
        self.checks = checks


# Who hashes the held pieces of an id-checked download: the library's SHA-1 kernel in one staged call
# (``Engine.sha1_host``: one lane per piece, so a call costs about one piece's chain, 7-9 ms for a
# 512 KiB piece, whatever the number of pieces), or ``hashlib`` on the hashing thread pool.  The
# kernel is taken for calls (stream windows) of at least ID_CHECK_GPU_MIN_PIECES pieces of at most
# ID_CHECK_GPU_MAX_PIECE_BYTES each.  Not measured on the download; the upload's measurements
# (GPU_PIECE_IDS, GPU_PARITY_IDS above) ended on the host for every id, so the default is the
# thread pool everywhere, and the kernel stays behind _ids_on_gpu, tested.
ID_CHECK_GPU_MIN_PIECES: int | None = None  # None: never
ID_CHECK_GPU_MAX_PIECE_BYTES = 1 << 62


def _ids_on_gpu(npieces: int, piece_bytes: int) -> bool:
    """Whether an id-checked call over `npieces` pieces, the largest of `piece_bytes`, hashes them
    with the SHA-1 kernel (else on the hashing thread pool)."""
    return (ID_CHECK_GPU_MIN_PIECES is not None and npieces >= ID_CHECK_GPU_MIN_PIECES
            and piece_bytes <= ID_CHECK_GPU_MAX_PIECE_BYTES)


def _recorded_id(ids, ch: EncodedChunk, piece_idx: int) -> bytes:
    """The id recorded for piece `piece_idx` of chunk ch, 20 bytes, from its 40-hex or 20-byte form."""
    try:
        v = ids[piece_idx]
    except (IndexError, KeyError, TypeError):
        v = None
    if v is None:
        raise ValueError(f"No recorded id for piece {piece_idx} of chunk {ch.chunk_idx}")
    v = bytes.fromhex(v) if isinstance(v, str) else bytes(v)
    if len(v) != 20:
        raise ValueError(f"The id of piece {piece_idx} of chunk {ch.chunk_idx} is not a SHA-1 digest")
    return v


def decode_chunks_id_checked(encoded_chunks: typing.Sequence[EncodedChunk],
                             piece_ids: typing.Sequence) -> tuple[bytes, list[ChunkIdCheck]]:
    """``decode_chunks`` with the reference's own integrity step before it: every held piece is
    hashed and compared with the id recorded for it at upload (validator.py:1556-1604 hashes each
    piece it receives and drops one whose SHA-1 is not its id, piece.py:54-68), and each chunk is
    reassembled from pieces that passed.

    ``piece_ids[c]`` holds the ids recorded for ``encoded_chunks[c]``, indexed by ``piece_idx``
    (what ``ChunkDHTValue.piece_hashes`` holds: 40-hex strings, or 20-byte values); only the held
    pieces' entries are read, and a held piece without one is a ``ValueError``.  Every distinct
    piece held of a chunk is hashed, all chunks' pieces in ONE batch (``_ids_on_gpu`` picks who
    hashes: the SHA-1 kernel in one ``sha1_host`` call, or ``hashlib`` on the hashing thread
    pool); then every chunk is decoded in ONE ``decode_host`` call from k of its good pieces
    (``choose_blocks``' pick among them), or, where fewer than k are good, from the first k held.

    A chunk's bytes are trustworthy exactly when its ``ChunkIdCheck`` is ``decodable``: then they
    come from pieces whose SHA-1 is the recorded id, whatever the other pieces hold and however
    many miners act together (which the code-word check of ``decode_chunks_checked`` cannot say,
    and it cannot check a chunk with exactly k pieces at all).  Otherwise they are what its first
    k pieces decode to.  The pieces are read twice (hashed, then decoded from); a fused native
    call is not built.  One device; the streaming form is ``reconstruct_data_stream_id_checked``."""
    chunks = list(encoded_chunks)
    if len(piece_ids) != len(chunks):
        raise ValueError("decode_chunks_id_checked: one list of recorded ids per chunk")
    held, want = [], []
    for ch, ids in zip(chunks, piece_ids):
        use = _held_pieces(ch, "reconstruct")
        held.append(use)
        want.append([_recorded_id(ids, ch, p.piece_idx) for p in use])
    if not chunks:
        return b"", []
    for ch, use, ids in zip(chunks, held, want):  # every chunk's preconditions before any hashing
        check_decode_ids_item(ch.k, ch.m, [p.data for p in use], [p.piece_idx for p in use], ch.padlen, ids)
    flat = [p.data for use in held for p in use]
    if _ids_on_gpu(len(flat), max(len(d) for d in flat)):
        got = iter(get_engine().sha1_host(flat))
    else:
        got = iter(_pool("hash").map(lambda d: hashlib.sha1(d).digest(), flat))
    out, items = [], []
    for ch, use, ids in zip(chunks, held, want):
        bad = [p.piece_idx for p, w in zip(use, ids) if next(got) != w]
        good = [p for p in use if p.piece_idx not in bad]
        ck = ChunkIdCheck(chunk_idx=ch.chunk_idx, checked=len(use), ok=not bad, bad_piece_idx=bad,
                          decodable=len(good) >= ch.k)
        out.append(ck)
        items.append(_basis_item(ch, good if ck.decodable else use, ch.padlen))
    return get_engine().decode_host(items), out


def reconstruct_data_id_checked(pieces: list[Piece], chunks: list[EncodedChunk],
                                piece_ids: typing.Sequence) -> tuple[bytes, list[ChunkIdCheck]]:
    """``reconstruct_data`` with every piece handed over checked against its recorded id in the same
    pass (``decode_chunks_id_checked``, grouped as ``reconstruct_data`` groups them; ``piece_ids[c]``
    belongs to ``chunks[c]``).  Raises ``ValueError("Not enough pieces to reconstruct chunk N")`` as
    ``reconstruct_data`` does, before any decode, and ``PieceIdError`` (carrying ``.checks``) when
    some chunk is not ``decodable``; otherwise returns the bytes, all from pieces that match their
    ids, and the checks."""
    _group_pieces(pieces, chunks)
    data, checks = decode_chunks_id_checked(chunks, piece_ids)
    bad = [ck.chunk_idx for ck in checks if not ck.decodable]
    if bad:
        raise PieceIdError(f"Fewer than k held pieces match their recorded ids in chunk(s) {bad}", checks)
    return data, checks


def reconstruct_data_stream_id_checked(pieces: list[Piece], chunks: list[EncodedChunk], piece_ids: typing.Sequence, *,
                                       window_bytes: int | None = None) -> Iterator[tuple[bytes, ChunkIdCheck]]:
    """``reconstruct_data_id_checked``'s contract, delivered as ``reconstruct_data_stream`` delivers:
    yield ``(bytes, ChunkIdCheck)`` chunk by chunk, in order.

    Chunks go in windows of about `window_bytes` (default STREAM_WINDOW_BYTES) of output.  Each
    window is one ``decode_chunks_id_checked`` on the stream worker (every piece handed over hashed
    in one batch, then one decode from good pieces; ``_ids_on_gpu`` picks who hashes, per window),
    and window w+1 runs while the caller consumes window w.  A yielded chunk is ``decodable``.  Errors are raised when the stream
    reaches the chunk, after every earlier chunk has been yielded: ``ValueError("Not enough pieces
    to reconstruct chunk N")``, a ``ValueError`` for a held piece without a recorded id, and
    ``PieceIdError`` (``.checks``: the checks of the chunks seen so far, that chunk's last).
    Closing the generator early cancels the windows not yet started.  One device: ``devices=`` is
    not provided, as for the whole check family."""
    if len(piece_ids) != len(chunks):
        raise ValueError("reconstruct_data_stream_id_checked: one list of recorded ids per chunk")
    yield from _stream_verified(
        pieces, list(zip(chunks, piece_ids)), window_bytes, decode_chunks_id_checked, lambda ck: ck.decodable,
        lambda ck, seen: PieceIdError(
            f"Fewer than k held pieces match their recorded ids in chunk {ck.chunk_idx}", seen))


def _pipeline(windows: Iterator[list], fn, args: tuple, grp) -> Iterator:
    """fn(window, *args) of each window on the stream workers, results in window order.

    One device (grp None): one _stream_pool worker, window w + 1 running while the caller
    consumes window w.  EngineGroup: window i on worker i mod D, 2 D windows in flight.  Windows
    are pulled from `windows` (on the caller's thread) only as slots free up; an error, or the
    consumer closing the stream early, cancels the windows not yet started."""
    if grp is None:
        pool = _stream_pool()
        depth, submit = 2, (lambda i, w: pool.submit(fn, w, *args))
    else:
        depth, submit = 2 * len(grp), (lambda i, w: grp.submit(i % len(grp), fn, w, *args))
    q: deque = deque()
    nxt = [0]

    def fill():
        while len(q) < depth:
            w = next(windows, None)
            if w is None:
                return
            q.append(submit(nxt[0], w))
            nxt[0] += 1

    try:
        fill()
        while q:
            fut = q.popleft()
            res = fut.result()
            yield res
            fill()
    finally:
        for f in q:
            f.cancel()


def _window_shapes(window: list):
    """(shapes of the window's chunks up to the first one encode_chunk would reject, that
    chunk's error or None): piece_length's ValueError for an empty chunk, easyfec's short middle
    slice (zfec Error)."""
    shapes = []
    for c in window:
        try:
            shape = _shapes([c])
            _short_middle(shape, [c])
        except Exception as e:  # noqa: BLE001 - raised on the caller's thread after the chunks before it
            return shapes, e
        shapes += shape
    return shapes, None


def _encode_window(window: list, first_idx: int, piece_ids: bool, tags=None):
    """Worker side of encode_chunks_stream: one batched GPU encode for the window (+ SHA-1 piece
    ids: on the GPU for large pieces, else on the hash pool, data pieces starting before the GPU
    call and parity pieces after it).  Returns (results, error): a chunk encode_chunk would
    reject ends the window there, and the chunks before it are still encoded and returned.
    tags (a challenge system): the results are (chunk, ids or None, tags), from the tagged
    encode; this worker thread's key and table are built on its first window."""
    shapes, err = _window_shapes(window)
    window = window[:len(shapes)]
    if not window:
        return [], err
    try:
        if tags is not None:
            out, ids, tgs = encode_chunks_with_tags(window, tags, first_idx, piece_ids=piece_ids)
            return list(zip(out, ids if piece_ids else [None] * len(out), tgs)), err
        if not piece_ids:
            return [(c, None) for c in encode_chunks(window, first_idx)], err
        hp = _pool("hash")
        if GPU_PIECE_IDS and min(B for (_, _, B, _) in shapes) >= PARALLEL_COPY_MIN:
            pieces, ids = _pieces_parallel(window, shapes, digests=True)
            return list(zip(_build_all(first_idx, window, shapes, pieces), ids)), err
        if HOST_PIECES:  # ids by the library's host threads (OpenSSL; parity ids on the GPU), pieces in the same call
            pieces, ids = _encode_pieces(list(window), shapes, True, GPU_PARITY_IDS)
            return list(zip(_build_all(first_idx, window, shapes, pieces), ids)), err
        if min(B for (_, _, B, _) in shapes) >= PARALLEL_COPY_MIN:
            pieces = _pieces_parallel(window, shapes)
            futs = [[hp.submit(_sha1_hex, b) for b in ps] for ps in pieces]
        else:  # small pieces: caller-thread copies; data pieces hash while the GPU runs
            prims = [_split(c, k, B) for c, (k, _, B, _) in zip(window, shapes)]
            futs = [[hp.submit(_sha1_hex, b) for b in prim] for prim in prims]
            parity = get_engine().encode_host(list(window), _km(shapes))
            pieces = [prim + par for prim, par in zip(prims, parity)]
            for fs, par in zip(futs, parity):
                fs.extend(hp.submit(_sha1_hex, b) for b in par)
        out = _build_all(first_idx, window, shapes, pieces)
        return [(ec, [f.result() for f in fs]) for ec, fs in zip(out, futs)], err
    except Exception as e:  # noqa: BLE001 - a device failure: nothing of the window is trusted
        return [], e


def encode_chunks_stream(chunks: Iterable[bytes], first_chunk_idx: int = 0, *, piece_ids: bool = False,
                         window_bytes: int | None = None, devices=None, tags=None) -> Iterator:
    """``encode_chunk`` over a stream of chunks (the validator's upload loop: chunks read from
    the request, encoded, handed to the miners, validator.py:1338-1446), pipelined.

    Chunks are pulled from `chunks` on the caller's thread into windows of about
    `window_bytes` (default STREAM_WINDOW_BYTES); each window is one batched GPU encode on a
    worker thread, running while the caller consumes the previous window's results (with
    `devices` / ``use_devices``: windows round robin over those devices, two per device in
    flight).  Yields ``EncodedChunk`` per chunk in order (chunk i gets index first_chunk_idx + i),
    or with ``piece_ids=True`` ``(EncodedChunk, [piece_hash of each of its m pieces])``; those ids
    come from the library's host threads for the data pieces and from the GPU for the parity
    pieces (GPU_PARITY_IDS; default window STREAM_WINDOW_PARITY_IDS_BYTES), or all from the GPU
    (GPU_PIECE_IDS) for windows of large pieces, whose default window is then
    STREAM_WINDOW_IDS_BYTES.

    tags (an ``apdp.ChallengeSystem``): yields ``(EncodedChunk, ids or None, [APDPTag of each of
    its m pieces])``, ids and tags from the window's one GPU pass (``encode_chunks_with_tags``).
    Not with `devices`: a tag key lives on one context."""
    if tags is not None and devices is not None:
        raise ValueError("encode_chunks_stream: tags= cannot be combined with devices= (a tag key lives on one "
                         "device)")
    return _encode_stream(chunks, first_chunk_idx, piece_ids, window_bytes, devices, tags)


def _encode_stream(chunks, first_chunk_idx, piece_ids, window_bytes, devices, tags) -> Iterator:
    """encode_chunks_stream's generator (its argument check runs at the call, not at the first item)."""
    wb = window_bytes
    if wb is None:
        wb = (STREAM_WINDOW_IDS_BYTES if piece_ids and GPU_PIECE_IDS else
              STREAM_WINDOW_PARITY_IDS_BYTES if piece_ids and HOST_PIECES and GPU_PARITY_IDS else STREAM_WINDOW_BYTES)

    def numbered():  # (window, index of its first chunk)
        idx = first_chunk_idx
        for win in _windows(chunks, wb, lambda c: max(len(c), 1)):
            yield win, idx
            idx += len(win)

    def run(wi, pid):
        return _encode_window(wi[0], wi[1], pid, tags)

    # (tagged windows run on the one stream worker, whatever use_devices set)
    for outs, err in _pipeline(numbered(), run, (piece_ids,), None if tags is not None else _group(devices)):
        for res in outs:
            yield res if tags is not None else (res if piece_ids else res[0])
        if err is not None:
            raise err
