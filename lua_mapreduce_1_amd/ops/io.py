"""Input staging: files / byte strings -> (pinned) host -> device tensors.

The bulk path is the native split loader (``csrc/host/loader.cpp``,
``_lib/libmrhost.so``): a pool of threads ``pread``s a rank's split files (or
byte ranges of one file) straight into the pinned staging buffer, publishing
a ready flag per split so the host->HBM copy of a chunk starts while later
splits are still being read.  The reference's map job reads its own split
file (examples/WordCount/mapfn.lua:4); here a rank reads only the splits it
owns, in parallel, without a bounce buffer.
"""
from __future__ import annotations

import ctypes
import os
import threading
import time

import numpy as np
import torch

_HOST = None
_HOST_LOCK = threading.Lock()


def host_lib():
    """The native host library (built in-tree by ``_build.build_all``)."""
    global _HOST
    with _HOST_LOCK:
        if _HOST is None:
            from .. import _build
            if not os.path.exists(_build.HOST_LIB):
                _build.build_cxx("host", "host", _build.HOST_LIB)
            L = ctypes.CDLL(_build.HOST_LIB)
            P, I64 = ctypes.c_void_p, ctypes.c_int64
            L.mrh_load_start.argtypes = [ctypes.c_int, P, P, P, P, P, P, P, ctypes.c_int, I64]
            L.mrh_load_start.restype = P
            L.mrh_load_done.argtypes = [P]
            L.mrh_load_done.restype = ctypes.c_int
            L.mrh_load_wait.argtypes = [P]
            L.mrh_load_wait.restype = ctypes.c_int
            L.mrh_drop_cache.argtypes = [ctypes.c_char_p]
            L.mrh_drop_cache.restype = ctypes.c_int
            L.mrh_pack_plan.argtypes = [ctypes.c_int, P, P, ctypes.c_int, P, P, P, P]
            L.mrh_pack_plan.restype = I64
            L.mrh_pack_run.argtypes = [ctypes.c_int, P, P, P, P, P, P, ctypes.c_int]
            L.mrh_pack_run.restype = ctypes.c_int
            L.mrh_dict_build.argtypes = [ctypes.c_int, P, P, ctypes.c_int, I64]
            L.mrh_dict_build.restype = P
            L.mrh_dict_entries.argtypes = [P]
            L.mrh_dict_entries.restype = I64
            L.mrh_dict_slots.argtypes = [P, P]
            L.mrh_dict_slots.restype = ctypes.c_int
            L.mrh_dict_plan.argtypes = [P, ctypes.c_int, P, P, ctypes.c_int, P, P]
            L.mrh_dict_plan.restype = ctypes.c_int
            L.mrh_dict_run.argtypes = [P, ctypes.c_int, P, P, P, P, ctypes.c_int]
            L.mrh_dict_run.restype = ctypes.c_int
            L.mrh_dict_free.argtypes = [P]
            L.mrh_dict_free.restype = None
            _HOST = L
    return _HOST


PACK_TABLE = 128  # bytes of one split's code table (code -> byte)


class PackedSplits:
    """Bit-packed copy of the splits of one host buffer (csrc/host/pack.cpp):
    ``buffer`` holds split i as ``k[i]``-bit codes at ``offsets[i]`` (16-byte
    aligned), ``nbytes[i]`` bytes long; ``tables[i]`` maps code -> byte.  A
    split with more than 128 distinct byte values is raw: ``k[i] == 8``,
    ``nbytes[i] == 0``, and it is read from the unpacked buffer."""

    __slots__ = ("buffer", "offsets", "nbytes", "k", "tables")

    def __init__(self, buffer, offsets, nbytes, k, tables):
        self.buffer, self.offsets, self.nbytes, self.k, self.tables = buffer, offsets, nbytes, k, tables


def pack_splits(buffer: torch.Tensor, offsets, threads: int = 8, pinned: bool = False) -> PackedSplits:
    """Pack the splits ``buffer[offsets[i]:offsets[i+1]]`` of a host buffer
    with the native packer.  ``pinned``: the packed buffer is allocated in
    pinned memory of its exact size (:func:`pinned_empty`)."""
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(off) - 1
    if n < 0 or (n and (off[0] < 0 or off[-1] > buffer.numel())):
        raise ValueError("pack_splits: split offsets outside the buffer")
    poff, pbytes = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    k = np.zeros(max(n, 1), dtype=np.int32)
    tables = np.zeros((max(n, 1), PACK_TABLE), dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L = host_lib()
    src = ctypes.c_void_p(buffer.data_ptr())
    total = int(L.mrh_pack_plan(n, src, ptr(off), int(threads), ptr(poff), ptr(pbytes), ptr(k), ptr(tables)))
    if total < 0:
        raise RuntimeError("mrh_pack_plan failed")
    out = pinned_empty(total) if pinned else torch.empty(total, dtype=torch.uint8)
    if L.mrh_pack_run(n, src, ptr(off), ptr(poff), ptr(k), ptr(tables), ctypes.c_void_p(out.data_ptr()),
                      int(threads)) != 0:
        raise RuntimeError("mrh_pack_run failed")
    return PackedSplits(out, poff[:n], pbytes[:n], k[:n], tables[:n])


DICT_SLOT = 32  # bytes of one dictionary entry on the device (bytes 0..30 the entry, byte 31 its length)
DICT_MAX_ENTRIES = 1 << 20
DICT_TILE_UNITS, DICT_TILE_BYTES = 4096, 8192


class DictSplits:
    """Dictionary-coded copy of the splits of one host buffer (csrc/host/
    dictpack.cpp).  ``slots`` is the dictionary (``[entries, 32]`` uint8).
    Split i is in this form when ``nbytes[i] > 0``: ``buffer`` holds its
    ``units[i]`` 16-bit code units at ``offsets[i]`` (16-byte aligned), and rows
    ``trow[i] .. trow[i] + tiles[i]`` (inclusive: one closing row) of ``tix``
    (``[rows, 2]`` uint32: first unit, first output byte) are its tile index.
    Every other split has ``nbytes[i] == 0`` and is shipped k-bit or raw."""

    __slots__ = ("buffer", "offsets", "nbytes", "units", "tiles", "trow", "tix", "slots", "seconds")

    def __init__(self, buffer, offsets, nbytes, units, tiles, trow, tix, slots, seconds=0.0):
        self.buffer, self.offsets, self.nbytes, self.units = buffer, offsets, nbytes, units
        self.tiles, self.trow, self.tix, self.slots, self.seconds = tiles, trow, tix, slots, seconds


def dict_pack_splits(buffer: torch.Tensor, offsets, other_bytes=None, threads: int = 16, pinned: bool = False,
                     max_entries: int = DICT_MAX_ENTRIES, force: bool = False) -> DictSplits:
    """Code the splits ``buffer[offsets[i]:offsets[i+1]]`` against one
    dictionary of their own tokens.  ``other_bytes[i]`` is what split i costs
    in its smallest other form (default: its raw size); a split is kept in the
    dictionary form only where that is strictly smaller (``force``: every
    non-empty split is kept, whatever it costs: the decoder's tests).
    ``pinned``: the code buffer is allocated in pinned memory of its exact
    size."""
    t0 = time.perf_counter()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(off) - 1
    if n < 0 or (n and (off[0] < 0 or off[-1] > buffer.numel())):
        raise ValueError("dict_pack_splits: split offsets outside the buffer")
    size = off[1:] - off[:-1]
    other = size if other_bytes is None else np.minimum(np.asarray(other_bytes, dtype=np.int64), size)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L = host_lib()
    src = ctypes.c_void_p(buffer.data_ptr())
    h = L.mrh_dict_build(n, src, ptr(off), int(threads), int(max_entries))
    if not h:
        raise RuntimeError("mrh_dict_build failed")
    try:
        slots = np.zeros((int(L.mrh_dict_entries(h)), DICT_SLOT), dtype=np.uint8)
        units, tiles = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        if L.mrh_dict_slots(h, ptr(slots)) != 0 or L.mrh_dict_plan(h, n, src, ptr(off), int(threads), ptr(units),
                                                                    ptr(tiles)) != 0:
            raise RuntimeError("mrh_dict_plan failed")
        units, tiles = units[:n], tiles[:n]
        take = (units > 0) if force else (units >= 0) & (2 * units < other)
        nbytes = np.where(take, 2 * units, 0)
        uoff = np.zeros(n, dtype=np.int64)
        np.cumsum(((nbytes + 15) & ~15)[:-1], out=uoff[1:])
        total = int(uoff[-1] + ((nbytes[-1] + 15) & ~15)) if n else 0
        rows = np.where(take, tiles + 1, 0)
        trow = np.zeros(n, dtype=np.int64)
        np.cumsum(rows[:-1], out=trow[1:])
        tix = np.zeros((max(int(rows.sum()), 1), 2), dtype=np.uint32)
        out = pinned_empty(total) if pinned else torch.empty(total, dtype=torch.uint8)
        u_arg = np.ascontiguousarray(np.where(take, uoff, -1), dtype=np.int64)
        t_arg = np.ascontiguousarray(trow, dtype=np.int64)
        if L.mrh_dict_run(h, n, ptr(u_arg), ptr(t_arg), ctypes.c_void_p(out.data_ptr()), ptr(tix),
                          int(threads)) != 0:
            raise RuntimeError("mrh_dict_run failed")
    finally:
        L.mrh_dict_free(h)
    return DictSplits(out, uoff, nbytes, np.where(take, units, 0), np.where(take, tiles, 0), trow, tix, slots,
                      time.perf_counter() - t0)


class AsyncLoad:
    """Reads in flight: ``paths[i]`` bytes ``[file_off[i], file_off[i]+length[i])``
    land at ``dst[dst_off[i]:]`` (+ a ``\\n`` when ``pad[i]``); ``ready[i]`` turns
    1 when job i is complete.  ``dst`` must stay alive until :meth:`wait`."""

    def __init__(self, paths, file_off, length, dst_off, pad, dst: torch.Tensor, threads: int = 8,
                 piece: int = 8 << 20):
        n = len(paths)
        self.n = n
        self._keep = (dst, [p.encode() if isinstance(p, str) else p for p in paths])
        cpaths = (ctypes.c_char_p * max(n, 1))(*self._keep[1])
        self._arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (file_off, length, dst_off)]
        self._pad = np.ascontiguousarray(pad, dtype=np.int32)
        self.ready = np.zeros(max(n, 1), dtype=np.int32)
        self._cpaths = cpaths
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        self._h = host_lib().mrh_load_start(n, ctypes.cast(cpaths, ctypes.c_void_p), *(ptr(a) for a in self._arrs),
                                            ptr(self._pad), ctypes.c_void_p(dst.data_ptr()), ptr(self.ready),
                                            int(threads), int(piece))
        if not self._h:
            raise RuntimeError("mrh_load_start failed")

    def done(self) -> int:
        return self.n if self._h is None else int(host_lib().mrh_load_done(self._h))

    def wait_jobs(self, j0: int, j1: int, poll: float = 20e-6) -> None:
        """Block until jobs [j0, j1) are complete (raises on a read error)."""
        r = self.ready
        while True:
            seg = r[j0:j1]
            if seg.min(initial=1) >= 1:
                return
            if (seg < 0).any():
                self.wait()
                raise OSError(f"split read failed (jobs {j0}..{j1})")
            time.sleep(poll)

    def wait(self) -> None:
        if self._h is not None:
            h, self._h = self._h, None
            rc = host_lib().mrh_load_wait(h)
            if rc != 0:
                raise OSError(-rc, os.strerror(-rc))

    def __del__(self):
        try:
            self.wait()
        except Exception:  # noqa: BLE001
            pass


def drop_page_cache(path: str) -> bool:
    """Evict a file's clean pages (posix_fadvise DONTNEED): the next read comes
    from the storage device (best effort; True when the call succeeded)."""
    return host_lib().mrh_drop_cache(path.encode()) == 0


def pinned_empty(nbytes: int) -> torch.Tensor:
    """Uninitialised uint8 host tensor in pinned memory of exactly ``nbytes``
    (csrc/hip/sort.hip mr_host_alloc).  torch's pinned allocator rounds a
    request up to a power of two, and pinning is paid per page: the 291 MB
    split buffer cost 22 ms as a 512 MB block (tools/cold_probe.py).  The
    memory is freed when the last tensor viewing it is gone."""
    import ctypes
    import weakref
    from . import _hip
    n = max(int(nbytes), 1)
    lib = _hip.lib()
    ptr = lib.mr_host_alloc(n)
    if not ptr:
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    arr = (ctypes.c_uint8 * n).from_address(ptr)
    f = weakref.finalize(arr, lib.mr_host_free, ptr)
    f.atexit = False  # at interpreter exit the process releases it (the HIP runtime may be gone)
    return torch.frombuffer(arr, dtype=torch.uint8)[:nbytes]


def read_file_bytes(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def bytes_to_device(data: bytes, device=None, pin: bool = True) -> torch.Tensor:
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else torch.zeros(0, dtype=torch.uint8)
    if device is None or torch.device(device).type == "cpu":
        return t
    if pin:
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def load_file(path: str, device=None) -> torch.Tensor:
    """Whole file as a uint8 tensor on ``device`` (host tensor when None/cpu),
    read by the native loader into (pinned) host memory first."""
    n = os.path.getsize(path)
    gpu = device is not None and torch.device(device).type != "cpu"
    host = torch.empty(n, dtype=torch.uint8, pin_memory=gpu)
    if n:
        AsyncLoad([path], [0], [n], [0], [0], host, threads=max(1, min(8, n >> 23))).wait()
    return host.to(device, non_blocking=True) if gpu else host
