"""ctypes bindings to libhiprag.so (the HIP/gfx950 vector index).

Declarations: include/hiprag.h.  ctypes releases the GIL for the duration of
every foreign call, so a blocking search does not stall other Python threads.
There is no CPU fallback: if the shared library or a GPU is missing, the
constructors raise.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhiprag.so")

DTYPES = {"f32": 0, "float32": 0, "fp32": 0, "bf16": 1, "bfloat16": 1, "f16": 2, "float16": 2, "fp16": 2}
METRICS = {"cosine": 0, "ip": 1, "dot": 1, "euclidean": 2, "l2": 2}
HR_MAX_K = 128   # include/hiprag.h
HR_MAX_KC = 256
HR_RANGE_MAX_HITS = 65536  # largest max_hits of search_range
HR_BOOST_MAX_COLS = 4  # boost columns of an index (set_boost / search_boosted)
HR_BOOST_MAX_WINDOW = 8192  # largest window of search_boosted
HR_EX_MAX = 32  # examples of one query of search_examples
HR_EX_KEEP = 1  # search_examples flag: the examples stay candidates
HR_FUSE_MAX_MEMBERS = 16  # lists of one group of search_fused / fuse_lists
FUSE_MODES = {"rrf": 0, "max": 1}  # HR_FUSE_RRF, HR_FUSE_MAX
HR_CREATE_NO_SHADOWS = 1
HR_LEX_TERM_BITS = 22    # term id = crc32(token) % 2**22
HR_LEX_MAX_QTERMS = 64
HR_LEX_MAX_K = 1024


def kc_for_k(k: int, dim: int = 0) -> int:
    """Per-shard candidate count for top-k (hr_kc_for_k_dim): k + max(16, k // 2) rounded up to 32 (32
    for k <= 16), the margin max(20, k) from 2048 dims on, at most HR_MAX_KC (tests/test_native_abi.py
    checks it against the library)."""
    wide = 2 if (dim + 63) // 64 * 64 >= 2048 else 1
    return min(HR_MAX_KC, (k + max(20 if wide == 2 else 16, wide * k // 2) + 31) // 32 * 32)


CAND_DTYPE = np.dtype([("score", "<f8"), ("row", "<i8")])  # matches hr::Cand

E_INVALID, E_HIP, E_UNSUPPORTED, E_OVERFLOW, E_IO, E_BUSY = -1, -2, -3, -4, -5, -6

# every symbol include/hiprag.h declares (checked by tests/test_native_abi.py)
EXPORTS = [
    "hr_index_create", "hr_index_reserve", "hr_index_add", "hr_index_add_synthetic", "hr_index_add_device",
    "hr_index_remove", "hr_index_search", "hr_index_search_device", "hr_index_size", "hr_index_get_rows",
    "hr_index_save", "hr_index_load", "hr_index_destroy", "hr_index_search_shard", "hr_index_search_shard_collect",
    "hr_merge_candidates", "hr_pool_normalize", "hr_pool_normalize_packed", "hr_hash_words", "hr_index_set_scan_timing", "hr_index_take_scan_times", "hr_index_last_scan_ms",
    "hr_device_count", "hr_index_debug_approx", "hr_index_last_candidates", "hr_last_error", "hr_abi_version",
    "hr_kc_for_k", "hr_merge_candidates_strided", "hr_index_search_shard_async", "hr_index_add_device_at",
    "hr_gen_rows_device", "hr_ivf_search", "hr_topk_records", "hr_index_search_shard_async_ev", "hr_index_stats",
    "hr_add_layernorm", "hr_index_info", "hr_index_graph_replays", "hr_index_wide_launches", "hr_kc_for_k_dim",
    "hr_index_search_submit", "hr_index_search_finalize", "hr_index_host_us", "hr_index_search_submit_host",
    "hr_index_search_collect", "hr_index_search_poll", "hr_index_set_persist", "hr_index_persist_close",
    "hr_index_persist_stats", "hr_index_persist_trace", "hr_index_wave_tiles", "hr_index_set_cu_mask",
    "hr_stream_create_cu_mask", "hr_stream_destroy", "hr_index_set_q256", "hr_index_q256_launches",
    "hr_index_search_shard_exact", "hr_merge_sorted", "hr_memcpy_async", "hr_attn_varlen", "hr_gelu_erf",
    "hr_lex_pack", "hr_lex_create", "hr_lex_destroy", "hr_lex_add", "hr_lex_remove", "hr_lex_size", "hr_lex_stats",
    "hr_lex_df", "hr_lex_search", "hr_lex_last_ms", "hr_index_set_shadow8", "hr_index_debug_approx8",
    "hr_index_shadow8_stats", "hr_index_create_ex", "hr_index_load_ex", "hr_index_copy_rows", "hr_ivf_search_ext",
    "hr_ivf_position_mask", "hr_index_set_groups", "hr_index_search_collapsed", "hr_index_search_collapsed_device",
    "hr_index_collapse_stats", "hr_index_set_collapse_timing", "hr_index_collapse_last_ms",
    "hr_index_search_masks", "hr_index_search_masks_device", "hr_index_qmask_launches",
    "hr_index_set_qmask_timing", "hr_index_qmask_last_ms",
    "hr_index_search_mmr", "hr_index_search_mmr_device", "hr_index_set_mmr_timing", "hr_index_mmr_last_ms",
    "hr_index_search_range", "hr_index_search_range_device", "hr_index_range_stats",
    "hr_index_range_wave_tiles",
    "hr_index_set_boost", "hr_index_search_boosted", "hr_index_search_boosted_device", "hr_index_boost_stats",
    "hr_index_build_queries", "hr_index_build_queries_device", "hr_index_search_examples",
    "hr_index_search_examples_device",
    "hr_fuse_lists", "hr_index_search_fused", "hr_index_search_fused_device",
]

_lib = None
_lib_lock = threading.Lock()


def cu_mask_words(cus) -> np.ndarray:
    """uint32 mask words of a CU list (bit i of word j = CU 32 j + i)."""
    cus = [int(c) for c in cus]
    words = np.zeros(max(cus) // 32 + 1, np.uint32)
    for c in cus:
        words[c // 32] |= np.uint32(1 << (c % 32))
    return words


def create_cu_stream(device: int, cus) -> int:
    """A raw HIP stream of `device` restricted to the CUs in `cus` (wrap it with torch.cuda.ExternalStream); release
    it with destroy_stream."""
    lib = load_library()
    words = cu_mask_words(cus)
    out = ctypes.c_void_p()
    _check(lib.hr_stream_create_cu_mask(int(device), words.ctypes.data, len(words), ctypes.byref(out)))
    return int(out.value)


def destroy_stream(stream: int) -> None:
    """Wait for the stream's work and destroy it (hr_stream_destroy).  Free first every pinned host tensor that a
    non_blocking torch copy ran on this stream for: torch's pinned-memory allocator records those streams and uses
    them again when the tensor is freed (a destroyed stream there crashed the interpreter at exit)."""
    _check(load_library().hr_stream_destroy(ctypes.c_void_p(stream)))


def memcpy_async(dst_ptr: int, src_ptr: int, nbytes: int, stream: int = 0) -> None:
    """Asynchronous copy on `stream` (hr_memcpy_async), outside torch's allocators' stream bookkeeping."""
    _check(load_library().hr_memcpy_async(ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), int(nbytes),
                                          ctypes.c_void_p(stream or None)))


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hiprag error {code}: {msg}")
        self.code = code


class BusyError(NativeError):
    """hr_index_search_submit_host found the handle held by another call (it never waits)."""


def load_library(path: str | None = None):
    """Load libhiprag.so (raises OSError if it was not built: run __graft_entry__.build())."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as
        # /opt/rocm's).  Loading torch first makes libhiprag.so bind to that same runtime, so
        # torch tensors, streams and RCCL interoperate with our kernels.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        p = path or os.environ.get("HIPRAG_LIB_OVERRIDE") or LIB_PATH  # override: A/B timing builds only
        if not os.path.exists(p):
            raise OSError(f"{p} not found; build it with `make -C youtu-rag_amd/csrc` or __graft_entry__.build()")
        L = ctypes.CDLL(p)
        vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
        pp = ctypes.POINTER(ctypes.c_void_p)
        sig = {
            "hr_index_create": [i32, i32, i32, i32, vp, pp],
            "hr_index_create_ex": [i32, i32, i32, i32, vp, i32, pp],
            "hr_index_load_ex": [ctypes.c_char_p, i32, vp, i32, pp],
            "hr_index_copy_rows": [vp, vp, vp, vp, i64, i64, vp],
            "hr_ivf_search_ext": [vp, vp, i32, vp, vp, vp, i64, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp],
            "hr_ivf_position_mask": [vp, i64, vp, i64, vp, vp],
            "hr_index_reserve": [vp, i64],
            "hr_index_add": [vp, vp, i64, vp],
            "hr_index_add_synthetic": [vp, u64, i64, i64, vp],
            "hr_index_add_device": [vp, vp, i64, vp, vp],
            "hr_index_remove": [vp, vp, i64],
            "hr_index_search": [vp, vp, i32, i32, vp, vp, vp],
            "hr_index_search_device": [vp, vp, i32, i32, vp, vp, vp, vp],
            "hr_index_search_submit": [vp, vp, i32, i32, vp, vp, vp, vp],
            "hr_index_search_finalize": [vp, i64],
            "hr_index_host_us": [vp, vp],
            "hr_index_search_submit_host": [vp, vp, i32, i32, i32, vp],
            "hr_index_search_collect": [vp, i64, vp, vp],
            "hr_index_search_poll": [vp, i64, vp],
            "hr_index_set_persist": [vp, i32],
            "hr_index_persist_close": [vp],
            "hr_index_set_shadow8": [vp, i32],
            "hr_index_debug_approx8": [vp, vp, i32, vp, vp],
            "hr_index_shadow8_stats": [vp, vp, vp],
            "hr_index_persist_stats": [vp, vp],
            "hr_index_persist_trace": [vp, ctypes.c_int, vp, vp],
            "hr_index_wave_tiles": [vp, vp, i32, vp],
            "hr_index_set_cu_mask": [vp, vp, i32],
            "hr_stream_create_cu_mask": [i32, vp, i32, pp],
            "hr_stream_destroy": [vp],
            "hr_memcpy_async": [vp, vp, i64, vp],
            "hr_attn_varlen": [vp, i32, vp, i32, i32, i32, i32, ctypes.c_float, vp, vp],
            "hr_gelu_erf": [vp, i32, i64, vp],
            "hr_index_set_q256": [vp, i32],
            "hr_index_q256_launches": [vp, vp],
            "hr_index_size": [vp, vp, vp],
            "hr_index_info": [vp, vp, vp, vp, vp],
            "hr_index_get_rows": [vp, vp, i64, vp],
            "hr_index_save": [vp, ctypes.c_char_p],
            "hr_index_load": [ctypes.c_char_p, i32, vp, pp],
            "hr_index_search_shard": [vp, vp, i32, i32, i32, vp, i64, vp, vp, vp],
            "hr_index_search_shard_async": [vp, vp, i32, i32, i32, vp, i64, vp, vp, vp, vp],
            "hr_index_search_shard_async_ev": [vp, vp, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp],
            "hr_index_add_device_at": [vp, vp, i64, vp, i64, vp],
            "hr_gen_rows_device": [u64, i64, i64, i32, vp, vp],
            "hr_topk_records": [vp, vp, i64, i32, i32, vp, vp],
            "hr_ivf_search": [vp, vp, i32, vp, i64, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp],
            "hr_index_search_shard_collect": [vp, vp, i32, vp, i32, vp, i64, vp, vp, vp],
            "hr_index_search_shard_exact": [vp, vp, i32, i32, vp, i64, vp, vp],
            "hr_merge_sorted": [i32, vp, i64, i32, i32, i32, i32, vp, vp, vp],
            "hr_merge_candidates": [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp],
            "hr_merge_candidates_strided": [i32, vp, vp, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp],
            "hr_pool_normalize": [vp, i32, vp, i32, i32, i32, i32, vp, vp],
            "hr_pool_normalize_packed": [vp, i32, vp, i32, i32, i32, vp, vp],
            "hr_hash_words": [vp, vp, i64, i64, i64, i64, i64, i64, vp, i64, vp],
            "hr_index_last_scan_ms": [vp, vp, vp],
            "hr_index_take_scan_times": [vp, vp, vp, i32, vp],
            "hr_index_set_scan_timing": [vp, i32],
            "hr_device_count": [vp],
            "hr_index_debug_approx": [vp, vp, i32, vp, vp],
            "hr_index_last_candidates": [vp, vp, vp],
            "hr_index_stats": [vp, vp],
            "hr_index_graph_replays": [vp, vp],
            "hr_index_wide_launches": [vp, vp],
            "hr_add_layernorm": [vp, vp, vp, vp, vp, i64, i32, ctypes.c_float, i32, vp],
            "hr_lex_pack": [vp, vp, i64, vp, i64, vp, vp],
            "hr_lex_create": [i32, pp],
            "hr_lex_add": [vp, vp, vp, i64, vp],
            "hr_lex_remove": [vp, vp, i64],
            "hr_lex_size": [vp, vp, vp],
            "hr_lex_stats": [vp, vp, vp],
            "hr_lex_df": [vp, vp, i64, vp],
            "hr_lex_search": [vp, vp, vp, i32, i32, ctypes.c_double, ctypes.c_double, vp, vp, vp],
            "hr_lex_last_ms": [vp, vp],
            "hr_index_set_groups": [vp, i64, i64, vp],
            "hr_index_search_collapsed": [vp, vp, i32, i32, i32, vp, vp, vp],
            "hr_index_search_collapsed_device": [vp, vp, i32, i32, i32, vp, vp, vp, vp],
            "hr_index_collapse_stats": [vp, vp],
            "hr_index_set_collapse_timing": [vp, i32],
            "hr_index_collapse_last_ms": [vp, vp],
            "hr_index_search_masks": [vp, vp, i32, i32, vp, i32, i64, vp, vp, vp],
            "hr_index_search_masks_device": [vp, vp, i32, i32, vp, i32, i64, vp, vp, vp, vp],
            "hr_index_qmask_launches": [vp, vp],
            "hr_index_set_qmask_timing": [vp, i32],
            "hr_index_qmask_last_ms": [vp, vp],
            "hr_index_search_mmr": [vp, vp, i32, i32, i32, ctypes.c_double, vp, vp, vp],
            "hr_index_search_mmr_device": [vp, vp, i32, i32, i32, ctypes.c_double, vp, vp, vp, vp],
            "hr_index_set_mmr_timing": [vp, i32],
            "hr_index_mmr_last_ms": [vp, vp],
            "hr_index_search_range": [vp, vp, i32, vp, i32, vp, vp, vp, vp],
            "hr_index_search_range_device": [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp],
            "hr_index_range_stats": [vp, vp],
            "hr_index_range_wave_tiles": [vp, vp, i32, vp],
            "hr_index_set_boost": [vp, i32, i64, i64, vp],
            "hr_index_search_boosted": [vp, vp, i32, i32, ctypes.c_double, vp, i32, i32, i32, vp, vp, vp, vp],
            "hr_index_search_boosted_device": [vp, vp, i32, i32, ctypes.c_double, vp, i32, i32, i32, vp, vp, vp, vp,
                                               vp],
            "hr_index_boost_stats": [vp, vp],
            "hr_index_build_queries": [vp, vp, vp, vp, i32, vp, vp],
            "hr_index_build_queries_device": [vp, vp, vp, vp, i32, vp, vp, vp],
            "hr_index_search_examples": [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp],
            "hr_index_search_examples_device": [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp],
            "hr_fuse_lists": [i32, vp, vp, i32, vp, vp, i32, i32, i32, ctypes.c_double, vp, vp, vp, vp],
            "hr_index_search_fused": [vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_double, vp, i32, i64, vp, vp, vp,
                                      vp],
            "hr_index_search_fused_device": [vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_double, vp, i32, i64, vp, vp,
                                             vp, vp, vp],
        }
        for name, args in sig.items():
            if p != (path or LIB_PATH) and not hasattr(L, name):
                continue  # an A/B timing build of an older source (HIPRAG_LIB_OVERRIDE) may lack newer entry points
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = i32
        L.hr_index_destroy.argtypes = [vp]
        L.hr_index_destroy.restype = None
        if hasattr(L, "hr_lex_destroy"):
            L.hr_lex_destroy.argtypes = [vp]
            L.hr_lex_destroy.restype = None
        L.hr_last_error.argtypes = []
        L.hr_last_error.restype = ctypes.c_char_p
        L.hr_abi_version.restype = i32
        L.hr_kc_for_k.argtypes = [i32]
        L.hr_kc_for_k.restype = i32
        L.hr_kc_for_k_dim.argtypes = [i32, i32]
        L.hr_kc_for_k_dim.restype = i32
        _lib = L
        return L


def _check(rc: int):
    if rc != 0:
        msg = (load_library().hr_last_error() or b"").decode(errors="replace")
        if rc == E_INVALID:
            raise ValueError(msg)
        if rc == E_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == E_BUSY:
            raise BusyError(rc, msg)
        raise NativeError(rc, msg)


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(load_library().hr_device_count(ctypes.byref(n)))
    return n.value


class NativeIndex:
    """One device shard of the vector index (an hr_index handle)."""

    def __init__(self, dim: int, dtype: str = "bf16", metric: str = "cosine", device: int = 0,
                 devices: list[int] | None = None, _handle=None, no_shadows: bool = False):
        """One index handle.  ``devices`` (GPU ids, repeats allowed) shards its rows over several
        GPUs inside the handle (hr_index_create with n_dev > 1); default: the single ``device``.
        ``no_shadows``: keep no 16-bit / 8-bit scan shadow (HR_CREATE_NO_SHADOWS: an index that is
        never scanned by the exact search, such as IVF lists)."""
        self.lib = load_library()
        self.devices = [int(d) for d in devices] if devices else [int(device)]
        self.dim, self.dtype, self.metric, self.device = int(dim), dtype, metric, self.devices[0]
        if _handle is not None:
            self._h = _handle
            return
        if dtype not in DTYPES:
            raise ValueError(f"unknown dtype {dtype!r}")
        if metric not in METRICS:
            raise ValueError(f"unknown metric {metric!r}")
        h = ctypes.c_void_p()
        dev = (ctypes.c_int * len(self.devices))(*self.devices)
        _check(self.lib.hr_index_create_ex(self.dim, DTYPES[dtype], METRICS[metric], len(self.devices), dev,
                                           HR_CREATE_NO_SHADOWS if no_shadows else 0, ctypes.byref(h)))
        self._h = h

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self.lib.hr_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data
    def reserve(self, rows: int):
        _check(self.lib.hr_index_reserve(self._h, int(rows)))

    def add(self, rows: np.ndarray) -> int:
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be (n, {self.dim}) float32")
        first = ctypes.c_int64(0)
        _check(self.lib.hr_index_add(self._h, _ptr(rows), rows.shape[0], ctypes.byref(first)))
        return first.value

    def add_device(self, rows_ptr: int, n: int, stream: int = 0) -> int:
        """Add n fp32 rows (row-major, dim wide) already in device memory; ordered after `stream`."""
        first = ctypes.c_int64(0)
        _check(self.lib.hr_index_add_device(self._h, ctypes.c_void_p(int(rows_ptr)), int(n), ctypes.byref(first),
                                            ctypes.c_void_p(int(stream))))
        return first.value

    def add_device_at(self, rows_ptr: int, n: int, dest_ptr: int, n_rows_after: int, stream: int = 0) -> None:
        """Store n fp32 device rows at the int64 device positions dest (IVF list placement)."""
        _check(self.lib.hr_index_add_device_at(self._h, ctypes.c_void_p(int(rows_ptr)), int(n),
                                               ctypes.c_void_p(int(dest_ptr)), int(n_rows_after),
                                               ctypes.c_void_p(int(stream))))

    def ivf_search(self, centroids_ptr: int, nlist: int, list_tiles_ptr: int, max_list_tiles: int, ids_ptr: int,
                   q_ptr: int, B: int, nprobe: int, k: int, cand_ptr: int, bound_ptr: int, probes_ptr: int = 0,
                   mask_ptr: int = 0, stream: int = 0) -> None:
        """IVF-flat search of the list-ordered rows of this index (hr_ivf_search)."""
        _check(self.lib.hr_ivf_search(self._h, ctypes.c_void_p(centroids_ptr), int(nlist),
                                      ctypes.c_void_p(list_tiles_ptr), int(max_list_tiles), ctypes.c_void_p(ids_ptr),
                                      ctypes.c_void_p(q_ptr), int(B), int(nprobe), int(k),
                                      ctypes.c_void_p(mask_ptr or None), ctypes.c_void_p(cand_ptr),
                                      ctypes.c_void_p(bound_ptr), ctypes.c_void_p(probes_ptr or None),
                                      ctypes.c_void_p(stream or None)))

    def ivf_search_ext(self, centroids_ptr: int, nlist: int, ext_off_ptr: int, ext_ptr: int, list_ntiles_ptr: int,
                       max_list_tiles: int, ids_ptr: int, q_ptr: int, B: int, nprobe: int, k: int, cand_ptr: int,
                       bound_ptr: int, probes_ptr: int = 0, mask_ptr: int = 0, stream: int = 0) -> None:
        """ivf_search over lists given as extents (hr_ivf_search_ext)."""
        _check(self.lib.hr_ivf_search_ext(self._h, ctypes.c_void_p(centroids_ptr), int(nlist),
                                          ctypes.c_void_p(ext_off_ptr), ctypes.c_void_p(ext_ptr or None),
                                          ctypes.c_void_p(list_ntiles_ptr), int(max_list_tiles),
                                          ctypes.c_void_p(ids_ptr), ctypes.c_void_p(q_ptr), int(B), int(nprobe),
                                          int(k), ctypes.c_void_p(mask_ptr or None), ctypes.c_void_p(cand_ptr),
                                          ctypes.c_void_p(bound_ptr), ctypes.c_void_p(probes_ptr or None),
                                          ctypes.c_void_p(stream or None)))

    def copy_rows_from(self, src: "NativeIndex", src_rows_ptr: int, dst_pos_ptr: int, n: int, n_rows_after: int,
                       stream: int = 0) -> None:
        """Copy the stored bits of n rows of ``src`` (int64 device row numbers) to the int64 device positions of
        this index (hr_index_copy_rows)."""
        _check(self.lib.hr_index_copy_rows(self._h, src._h, ctypes.c_void_p(int(src_rows_ptr) or None),
                                           ctypes.c_void_p(int(dst_pos_ptr) or None), int(n), int(n_rows_after),
                                           ctypes.c_void_p(int(stream) or None)))

    def add_synthetic(self, seed: int, global_row0: int, n: int) -> int:
        first = ctypes.c_int64(0)
        _check(self.lib.hr_index_add_synthetic(self._h, int(seed), int(global_row0), int(n), ctypes.byref(first)))
        return first.value

    def remove(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1))
        _check(self.lib.hr_index_remove(self._h, _ptr(r), len(r)))

    def size(self) -> tuple[int, int]:
        n, live = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib.hr_index_size(self._h, ctypes.byref(n), ctypes.byref(live)))
        return n.value, live.value

    def get_rows(self, rows) -> np.ndarray:
        r = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1))
        out = np.empty((len(r), self.dim), np.float32)
        _check(self.lib.hr_index_get_rows(self._h, _ptr(r), len(r), _ptr(out)))
        return out

    # -- search
    def _queries(self, q) -> np.ndarray:
        """The queries of a host-form search as a contiguous float32 (B, dim) array; one query may come 1-D."""
        q = np.ascontiguousarray(q, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"query dim {q.shape[1]} != index dim {self.dim}")
        return q

    def search(self, q: np.ndarray, k: int, mask: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
        q = self._queries(q)
        B = q.shape[0]
        s = np.empty((B, k), np.float32)
        r = np.empty((B, k), np.int64)
        m = self._mask_words(mask)
        _check(self.lib.hr_index_search(self._h, _ptr(q), B, int(k), _ptr(m), _ptr(s), _ptr(r)))
        return s, r

    def search_masks(self, q: np.ndarray, k: int, masks, mask_of) -> tuple[np.ndarray, np.ndarray]:
        """search() with one row mask PER QUERY in one call (hr_index_search_masks): ``masks`` is a (D, words) uint64
        array of row bitmaps (or a list of D equally long ones), ``mask_of[i]`` the bitmap of query i, -1 = none.
        Query i gets exactly what ``search(q[i], k, masks[mask_of[i]])`` gives.  A multi-device handle raises
        NotImplementedError: group the queries by mask and call search()."""
        q = self._queries(q)
        B = q.shape[0]
        of = np.ascontiguousarray(np.asarray(mask_of, np.int32).reshape(-1))
        if len(of) != B:
            raise ValueError(f"mask_of has {len(of)} entries for {B} queries")
        m = np.ascontiguousarray(masks, np.uint64) if masks is not None and len(masks) else np.zeros((0, 0), np.uint64)
        if m.ndim == 1:
            m = m[None, :]
        D, words = int(m.shape[0]), int(m.shape[1]) if m.ndim == 2 else 0
        if D:
            n_rows = self.size()[0]
            if words * 64 < n_rows:  # the library reads one bit per index row
                raise ValueError(f"row mask has {words} words, the index {n_rows} rows "
                                 f"(needs {(n_rows + 63) // 64})")
        s = np.empty((B, k), np.float32)
        r = np.empty((B, k), np.int64)
        _check(self.lib.hr_index_search_masks(self._h, _ptr(q), B, int(k), _ptr(m) if D else None, D, words, _ptr(of),
                                              _ptr(s), _ptr(r)))
        return s, r

    def search_masks_device(self, q_ptr: int, B: int, k: int, scores_ptr: int, rows_ptr: int, masks_ptr: int, D: int,
                            mask_stride: int, mask_of_ptr: int, stream: int = 0) -> None:
        """search_masks() with every array in device memory (D bitmaps ``mask_stride`` uint64 words apart, B int32
        mask_of entries); ordered after the work queued on ``stream``, which is idle on return."""
        if D:
            n_rows = self.size()[0]
            if int(mask_stride) * 64 < n_rows:
                raise ValueError(f"row mask has {int(mask_stride)} words, the index {n_rows} rows "
                                 f"(needs {(n_rows + 63) // 64})")
        _check(self.lib.hr_index_search_masks_device(self._h, ctypes.c_void_p(q_ptr), int(B), int(k),
                                                     ctypes.c_void_p(masks_ptr or None), int(D), int(mask_stride),
                                                     ctypes.c_void_p(mask_of_ptr), ctypes.c_void_p(scores_ptr),
                                                     ctypes.c_void_p(rows_ptr), ctypes.c_void_p(stream or None)))

    def qmask_launches(self) -> int:
        """FILTER launches that ran with per-query masks (one per chunk of up to 64 queries of search_masks)."""
        out = ctypes.c_int64(0)
        _check(self.lib.hr_index_qmask_launches(self._h, ctypes.byref(out)))
        return int(out.value)

    def set_qmask_timing(self, on: bool) -> None:
        _check(self.lib.hr_index_set_qmask_timing(self._h, int(bool(on))))

    def qmask_last_ms(self) -> dict:
        """HIP-event times of the most recent timed search_masks call's mask prep (set_qmask_timing)."""
        out = (ctypes.c_double * 2)()
        _check(self.lib.hr_index_qmask_last_ms(self._h, out))
        return {"union_tile_list_ms": out[0], "allow_table_ms": out[1]}

    def _mask_words(self, mask):
        if mask is None:
            return None
        m = np.ascontiguousarray(mask, np.uint64).reshape(-1)
        n_rows = self.size()[0]
        if len(m) * 64 < n_rows:  # the library reads one bit per index row
            raise ValueError(f"row mask has {len(m)} words, the index {n_rows} rows (needs {(n_rows + 63) // 64})")
        return m

    # -- collapsed search (hr_collapse.hip): the exact top-k distinct groups, each by its best row
    def set_groups(self, row0: int, groups) -> None:
        """Group ids (int32, -1 = none) of rows [row0, row0 + len(groups)) (hr_index_set_groups)."""
        g = np.ascontiguousarray(np.asarray(groups, np.int32).reshape(-1))
        _check(self.lib.hr_index_set_groups(self._h, int(row0), len(g), _ptr(g)))

    def search_collapsed(self, q: np.ndarray, k: int, mask: np.ndarray | None = None,
                         probe: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """search() with one hit per group: the best row of each of the k best groups, exactly
        (hr_index_search_collapsed).  ``probe``: rows the first stage fetches (0 = the library's default)."""
        q = self._queries(q)
        B = q.shape[0]
        s = np.empty((B, k), np.float32)
        r = np.empty((B, k), np.int64)
        m = self._mask_words(mask)
        _check(self.lib.hr_index_search_collapsed(self._h, _ptr(q), B, int(k), int(probe), _ptr(m), _ptr(s), _ptr(r)))
        return s, r

    def search_collapsed_device(self, q_ptr: int, B: int, k: int, scores_ptr: int, rows_ptr: int, mask_ptr: int = 0,
                                probe: int = 0, stream: int = 0) -> None:
        _check(self.lib.hr_index_search_collapsed_device(self._h, ctypes.c_void_p(q_ptr), int(B), int(k), int(probe),
                                                         ctypes.c_void_p(mask_ptr or None),
                                                         ctypes.c_void_p(scores_ptr), ctypes.c_void_p(rows_ptr),
                                                         ctypes.c_void_p(stream or None)))

    def collapse_stats(self) -> dict:
        """Cumulative collapsed queries answered from the probe / by the all-rows pass."""
        out = (ctypes.c_int64 * 2)()
        _check(self.lib.hr_index_collapse_stats(self._h, out))
        return {"probe": int(out[0]), "all_rows": int(out[1])}

    def set_collapse_timing(self, on: bool) -> None:
        _check(self.lib.hr_index_set_collapse_timing(self._h, int(bool(on))))

    def collapse_last_ms(self) -> dict:
        """HIP-event times of the most recent timed collapsed call (set_collapse_timing)."""
        out = (ctypes.c_double * 3)()
        _check(self.lib.hr_index_collapse_last_ms(self._h, out))
        return {"probe_ms": out[0], "prefix_ms": out[1], "all_rows_ms": out[2]}

    # -- MMR search (hr_mmr.hip): k rows chosen by maximal marginal relevance from the exact top-fetch_k pool
    def search_mmr(self, q: np.ndarray, k: int, lam: float, mask: np.ndarray | None = None,
                   fetch_k: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """search() diversified (hr_index_search_mmr): greedy picks of the largest lam * relevance - (1 - lam) * (max
        similarity to the rows picked so far) from the exact top-``fetch_k`` (0 = min(HR_MAX_K, max(32, 4 k))).  Rows
        in selection order, each with its plain-search score: the scores are not monotone.  lam = 1 is search()."""
        q = self._queries(q)
        B = q.shape[0]
        if int(k) <= 0 or int(k) > HR_MAX_K:  # (before the output arrays are sized by it)
            raise ValueError(f"k must be in [1, {HR_MAX_K}]")
        s = np.empty((B, int(k)), np.float32)
        r = np.empty((B, int(k)), np.int64)
        m = self._mask_words(mask)
        _check(self.lib.hr_index_search_mmr(self._h, _ptr(q), B, int(k), int(fetch_k), float(lam), _ptr(m), _ptr(s),
                                            _ptr(r)))
        return s, r

    def search_mmr_device(self, q_ptr: int, B: int, k: int, lam: float, scores_ptr: int, rows_ptr: int,
                          mask_ptr: int = 0, fetch_k: int = 0, stream: int = 0) -> None:
        _check(self.lib.hr_index_search_mmr_device(self._h, ctypes.c_void_p(q_ptr), int(B), int(k), int(fetch_k),
                                                   float(lam), ctypes.c_void_p(mask_ptr or None),
                                                   ctypes.c_void_p(scores_ptr), ctypes.c_void_p(rows_ptr),
                                                   ctypes.c_void_p(stream or None)))

    def set_mmr_timing(self, on: bool) -> None:
        _check(self.lib.hr_index_set_mmr_timing(self._h, int(bool(on))))

    def mmr_last_ms(self) -> dict:
        """HIP-event times of the most recent timed MMR call (set_mmr_timing)."""
        out = (ctypes.c_double * 2)()
        _check(self.lib.hr_index_mmr_last_ms(self._h, out))
        return {"probe_ms": out[0], "select_ms": out[1]}

    # -- range search (hr_range.hip): every row scoring at least a threshold, with the exact count
    def search_range(self, q: np.ndarray, min_score, max_hits: int = 1024, mask: np.ndarray | None = None):
        """Every live, allowed row whose fp32 score is >= ``min_score`` (a scalar or one value per query), exactly
        (hr_index_search_range): ``(scores, rows, counts)`` -- the first min(count, max_hits) hits of every query in
        search()'s order, -inf / -1 after them, and the exact number of hits, also beyond ``max_hits``.
        ``max_hits = 0`` only counts: ``(None, None, counts)``."""
        q = self._queries(q)
        B = q.shape[0]
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, np.float32).reshape(-1), (B,)))
        max_hits = int(max_hits)
        if max_hits < 0 or max_hits > HR_RANGE_MAX_HITS:  # (before the output arrays are sized by it)
            raise ValueError(f"max_hits must be in [0, {HR_RANGE_MAX_HITS}]")
        s = np.empty((B, max_hits), np.float32) if max_hits else None
        r = np.empty((B, max_hits), np.int64) if max_hits else None
        c = np.zeros(B, np.int64)
        m = self._mask_words(mask)
        _check(self.lib.hr_index_search_range(self._h, _ptr(q), B, _ptr(t), max_hits, _ptr(m), _ptr(s), _ptr(r),
                                              _ptr(c)))
        return s, r, c

    def search_range_device(self, q_ptr: int, B: int, min_score_ptr: int, max_hits: int, scores_ptr: int,
                            rows_ptr: int, counts_ptr: int, mask_ptr: int = 0, stream: int = 0) -> None:
        """search_range() with every array in device memory (B fp32 thresholds, B int64 counts); ordered after the
        work queued on ``stream``, which is idle on return."""
        _check(self.lib.hr_index_search_range_device(self._h, ctypes.c_void_p(q_ptr), int(B),
                                                     ctypes.c_void_p(min_score_ptr), int(max_hits),
                                                     ctypes.c_void_p(mask_ptr or None),
                                                     ctypes.c_void_p(scores_ptr or None),
                                                     ctypes.c_void_p(rows_ptr or None), ctypes.c_void_p(counts_ptr),
                                                     ctypes.c_void_p(stream or None)))

    def range_stats(self) -> dict:
        """Cumulative range queries answered by the window scan / by the all-rows pass, and window-scan launches."""
        out = (ctypes.c_int64 * 3)()
        _check(self.lib.hr_index_range_stats(self._h, out))
        return {"window": int(out[0]), "all_rows": int(out[1]), "scans": int(out[2])}

    def range_wave_tiles(self, cap: int = 1 << 16) -> np.ndarray:
        """Tiles each wave of the most recent window scan of search_range scanned (hr_index_range_wave_tiles)."""
        out = np.zeros(cap, np.uint32)
        n = ctypes.c_int(0)
        _check(self.lib.hr_index_range_wave_tiles(self._h, _ptr(out), int(cap), ctypes.byref(n)))
        return out[: n.value].copy()

    # -- boosted search (hr_boost.hip): the exact top-k of alpha * similarity + sum of beta_c * boost column c
    def set_boost(self, col: int, row0: int, values) -> None:
        """fp32 boost values (finite) of rows [row0, row0 + len(values)) of column ``col`` (hr_index_set_boost)."""
        v = np.ascontiguousarray(np.asarray(values, np.float32).reshape(-1))
        _check(self.lib.hr_index_set_boost(self._h, int(col), int(row0), len(v), _ptr(v)))

    @staticmethod
    def _betas(betas) -> np.ndarray:
        b = np.ascontiguousarray(np.asarray(betas, np.float64).reshape(-1))
        if len(b) > HR_BOOST_MAX_COLS:
            raise ValueError(f"at most {HR_BOOST_MAX_COLS} boost columns")
        return b

    def search_boosted(self, q: np.ndarray, k: int, alpha: float, betas, mask: np.ndarray | None = None,
                       probe: int = 0, window: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The first ``k`` live, allowed rows by ``alpha * score + sum_c betas[c] * column_c`` (fp64, every operation
        rounded once, in column order), then row ascending -- over the whole index, exactly
        (hr_index_search_boosted): ``(blended f64, scores f32, rows i64)``, the scores being search()'s; -inf / -inf /
        -1 past the live, allowed rows.  ``probe`` / ``window``: the pilot's depth and the stage-1 window (0 = the
        library's defaults)."""
        q = self._queries(q)
        B = q.shape[0]
        if int(k) <= 0 or int(k) > HR_MAX_K:  # (before the output arrays are sized by it)
            raise ValueError(f"k must be in [1, {HR_MAX_K}]")
        b = self._betas(betas)
        v = np.empty((B, int(k)), np.float64)
        s = np.empty((B, int(k)), np.float32)
        r = np.empty((B, int(k)), np.int64)
        m = self._mask_words(mask)
        _check(self.lib.hr_index_search_boosted(self._h, _ptr(q), B, int(k), float(alpha), _ptr(b) if len(b) else None,
                                                len(b), int(probe), int(window), _ptr(m), _ptr(v), _ptr(s), _ptr(r)))
        return v, s, r

    def search_boosted_device(self, q_ptr: int, B: int, k: int, alpha: float, betas, blended_ptr: int,
                              scores_ptr: int, rows_ptr: int, mask_ptr: int = 0, probe: int = 0, window: int = 0,
                              stream: int = 0) -> None:
        """search_boosted() with the queries, the mask and the three outputs in device memory (``betas`` stays a host
        sequence); ordered after the work queued on ``stream``, which is idle on return."""
        b = self._betas(betas)
        _check(self.lib.hr_index_search_boosted_device(self._h, ctypes.c_void_p(q_ptr), int(B), int(k), float(alpha),
                                                       _ptr(b) if len(b) else None, len(b), int(probe), int(window),
                                                       ctypes.c_void_p(mask_ptr or None),
                                                       ctypes.c_void_p(blended_ptr), ctypes.c_void_p(scores_ptr),
                                                       ctypes.c_void_p(rows_ptr), ctypes.c_void_p(stream or None)))

    def boost_stats(self) -> dict:
        """Cumulative boosted queries answered by the window (stage 1) / by the all-rows pass (stage 2)."""
        out = (ctypes.c_int64 * 2)()
        _check(self.lib.hr_index_boost_stats(self._h, out))
        return {"window": int(out[0]), "all_rows": int(out[1])}

    # -- search by example (hr_examples.hip): queries built on the device from stored rows
    @staticmethod
    def _example_lists(examples, weights):
        """(rows int64, weights fp32, offsets int64) of a list of row lists; default weights 1 / m_b, computed in
        float64 and cast to fp32."""
        examples = list(examples)
        lens = [len(e) for e in examples]  # (one pass over flat Python lists: this runs before every launch)
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        tot = int(off[-1])
        rows = np.fromiter(itertools.chain.from_iterable(examples), np.int64, count=tot)
        if weights is None:
            w = np.repeat(np.float64(1.0) / np.maximum(np.asarray(lens, np.float64), 1.0), lens).astype(np.float32)
        else:
            weights = list(weights)
            if [len(x) for x in weights] != lens:
                raise ValueError("weights must have the shape of examples")
            w = np.fromiter(itertools.chain.from_iterable(weights), np.float64, count=tot).astype(np.float32)
        return rows, w, off

    def _base_queries(self, q, B):
        if q is None:
            return None
        q = np.ascontiguousarray(q, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape != (B, self.dim):
            raise ValueError(f"base queries must be ({B}, {self.dim}) float32")
        return q

    def build_queries(self, examples, weights=None, q=None) -> np.ndarray:
        """The queries search_examples searches with (hr_index_build_queries): per entry of ``examples`` (a list of
        row lists) ``q[b] + sum of weights[b][e] * stored row examples[b][e]`` accumulated in float64 in list order
        and cast to fp32.  ``weights``: the same shape as ``examples``, default 1 / len(examples[b]); ``q``: optional
        (B, dim) base vectors."""
        rows, w, off = self._example_lists(examples, weights)
        B = len(off) - 1
        q = self._base_queries(q, B)
        out = np.empty((B, self.dim), np.float32)
        _check(self.lib.hr_index_build_queries(self._h, _ptr(rows), _ptr(w), _ptr(off), B, _ptr(q), _ptr(out)))
        return out

    def build_queries_device(self, examples, q_out_ptr: int, weights=None, q_ptr: int = 0, stream: int = 0) -> None:
        """build_queries() with the base vectors and the output in device memory (the lists stay host lists); the
        output can feed any ``*_device`` search.  Ordered after ``stream``, which is idle on return."""
        rows, w, off = self._example_lists(examples, weights)
        _check(self.lib.hr_index_build_queries_device(self._h, _ptr(rows), _ptr(w), _ptr(off), len(off) - 1,
                                                      ctypes.c_void_p(q_ptr or None), ctypes.c_void_p(q_out_ptr),
                                                      ctypes.c_void_p(stream or None)))

    def search_examples(self, examples, k: int, weights=None, q=None, mask: np.ndarray | None = None,
                        keep: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """"More like these rows" (hr_index_search_examples): search() of build_queries(examples, weights, q) with
        every query's own examples -- positive and negative -- removed from its candidates, exactly; ``keep=True``
        leaves them in (then it is search() of the built queries, bit for bit)."""
        rows, w, off = self._example_lists(examples, weights)
        B = len(off) - 1
        q = self._base_queries(q, B)
        if int(k) <= 0:  # (before the output arrays are sized by it)
            raise ValueError("k must be positive")
        s = np.empty((B, int(k)), np.float32)
        r = np.empty((B, int(k)), np.int64)
        m = self._mask_words(mask)
        _check(self.lib.hr_index_search_examples(self._h, _ptr(q), _ptr(rows), _ptr(w), _ptr(off), B, int(k),
                                                 HR_EX_KEEP if keep else 0, _ptr(m), _ptr(s), _ptr(r)))
        return s, r

    def search_examples_device(self, examples, k: int, scores_ptr: int, rows_ptr: int, weights=None, q_ptr: int = 0,
                               mask_ptr: int = 0, keep: bool = False, stream: int = 0) -> None:
        """search_examples() with base vectors, mask and outputs in device memory (the lists stay host lists);
        ordered after ``stream``, which is idle on return."""
        rows, w, off = self._example_lists(examples, weights)
        _check(self.lib.hr_index_search_examples_device(self._h, ctypes.c_void_p(q_ptr or None), _ptr(rows), _ptr(w),
                                                        _ptr(off), len(off) - 1, int(k), HR_EX_KEEP if keep else 0,
                                                        ctypes.c_void_p(mask_ptr or None),
                                                        ctypes.c_void_p(scores_ptr), ctypes.c_void_p(rows_ptr),
                                                        ctypes.c_void_p(stream or None)))

    # -- fused multi-query search (hr_fuse.hip): groups of queries, their exact lists fused on the device
    def fuse_lists(self, rows_ptr: int, scores_ptr: int, P: int, groups, k: int, fused_ptr: int, rows_out_ptr: int,
                   members_ptr: int = 0, mode: str = "rrf", rrf_k: float = 60.0, weights=None, stream: int = 0) -> None:
        """fuse_lists() of the module on this index's device."""
        fuse_lists(self.devices[0], rows_ptr, scores_ptr, P, groups, k, fused_ptr, rows_out_ptr, members_ptr, mode,
                   rrf_k, weights, stream)

    def _fused_args(self, groups, k, mode, weights):
        off, w = _fuse_groups(groups, weights)
        if int(k) <= 0 or int(k) > HR_MAX_K:  # (before the output arrays are sized by it)
            raise ValueError(f"k must be in [1, {HR_MAX_K}]")
        return off, w, _fuse_mode(mode)

    def search_fused(self, q: np.ndarray, groups, k: int, fetch_k: int = 0, mode: str = "rrf", rrf_k: float = 60.0,
                     weights=None, masks=None, mask_of=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Groups of queries answered as one fused list each (hr_index_search_fused).  ``groups``: the member count
        of every group (the queries of ``q`` in order; 1 to 16 members each).  Every member is searched exactly for
        ``fetch_k`` rows (0 = min(HR_MAX_K, max(4 k, 50)) for "rrf", k for "max"), all members in one scan, and the
        lists of a group are fused on the device: ``mode="rrf"`` sums ``weights[i] / (rrf_k + rank)`` in float64 in
        member order (``weights``: one fp32 value per query, default 1), ``mode="max"`` keeps the largest score.
        ``masks`` / ``mask_of`` as search_masks: one row bitmap per member.  Returns ``(fused float64 (G, k), rows
        int64 (G, k), members uint32 (G, k))``, fused score descending then row ascending, -inf / -1 / 0 after the
        distinct rows; bit j of ``members`` says that member j of the group holds the row."""
        q = self._queries(q)
        off, w, md = self._fused_args(groups, k, mode, weights)
        Q, G = int(off[-1]), len(off) - 1
        if q.shape[0] != Q:
            raise ValueError(f"{q.shape[0]} queries for groups of {Q} members")
        m, of, D, words = None, None, 0, 0
        if mask_of is not None:
            of = np.ascontiguousarray(np.asarray(mask_of, np.int32).reshape(-1))
            if len(of) != Q:
                raise ValueError(f"mask_of has {len(of)} entries for {Q} queries")
            m = np.ascontiguousarray(masks, np.uint64) if masks is not None and len(masks) else np.zeros((0, 0), np.uint64)
            if m.ndim == 1:
                m = m[None, :]
            D, words = int(m.shape[0]), int(m.shape[1]) if m.ndim == 2 else 0
            if D:
                n_rows = self.size()[0]
                if words * 64 < n_rows:  # the library reads one bit per index row
                    raise ValueError(f"row mask has {words} words, the index {n_rows} rows "
                                     f"(needs {(n_rows + 63) // 64})")
            elif (of >= 0).any():
                raise ValueError("mask_of names a bitmap and there is none")
        f = np.empty((G, int(k)), np.float64)
        r = np.empty((G, int(k)), np.int64)
        mem = np.empty((G, int(k)), np.uint32)
        _check(self.lib.hr_index_search_fused(self._h, _ptr(q), _ptr(off), _ptr(w), G, int(k), int(fetch_k), md,
                                              float(rrf_k), _ptr(m) if D else None, D, words,
                                              _ptr(of) if D else None, _ptr(f), _ptr(r), _ptr(mem)))
        return f, r, mem

    def search_fused_device(self, q_ptr: int, groups, k: int, fused_ptr: int, rows_ptr: int, members_ptr: int = 0,
                            fetch_k: int = 0, mode: str = "rrf", rrf_k: float = 60.0, weights=None, masks_ptr: int = 0,
                            D: int = 0, mask_stride: int = 0, mask_of_ptr: int = 0, stream: int = 0) -> None:
        """search_fused() with queries, bitmaps, mask_of and outputs in device memory (``groups`` and ``weights`` stay
        host lists; ``members_ptr`` 0: no member bits); ordered after ``stream``, which is idle on return."""
        off, w, md = self._fused_args(groups, k, mode, weights)
        if D:
            n_rows = self.size()[0]
            if int(mask_stride) * 64 < n_rows:
                raise ValueError(f"row mask has {int(mask_stride)} words, the index {n_rows} rows "
                                 f"(needs {(n_rows + 63) // 64})")
        _check(self.lib.hr_index_search_fused_device(self._h, ctypes.c_void_p(q_ptr), _ptr(off), _ptr(w), len(off) - 1,
                                                     int(k), int(fetch_k), md, float(rrf_k),
                                                     ctypes.c_void_p(masks_ptr or None), int(D), int(mask_stride),
                                                     ctypes.c_void_p(mask_of_ptr or None), ctypes.c_void_p(fused_ptr),
                                                     ctypes.c_void_p(rows_ptr), ctypes.c_void_p(members_ptr or None),
                                                     ctypes.c_void_p(stream or None)))

    def search_device(self, q_ptr: int, B: int, k: int, scores_ptr: int, rows_ptr: int, mask_ptr: int = 0,
                      stream: int = 0) -> None:
        _check(self.lib.hr_index_search_device(self._h, ctypes.c_void_p(q_ptr), int(B), int(k),
                                               ctypes.c_void_p(mask_ptr or None), ctypes.c_void_p(scores_ptr),
                                               ctypes.c_void_p(rows_ptr), ctypes.c_void_p(stream or None)))

    def search_submit(self, q_ptr: int, B: int, k: int, scores_ptr: int, rows_ptr: int, stream: int = 0) -> int:
        """Pipelined search_device (no mask): enqueue a batch, return its ticket.  A multi-device handle
        keeps two batches in flight (one host thread per shard); the outputs are final once
        search_finalize(ticket) returns.  A single-device handle finishes the batch here (ticket 0)."""
        t = ctypes.c_int64(0)
        _check(self.lib.hr_index_search_submit(self._h, ctypes.c_void_p(q_ptr), int(B), int(k),
                                               ctypes.c_void_p(scores_ptr), ctypes.c_void_p(rows_ptr),
                                               ctypes.c_void_p(stream or None), ctypes.byref(t)))
        return t.value

    def search_submit_host(self, q: np.ndarray, k: int, notify_fd: int = -1) -> int:
        """Asynchronous search of host queries (single-device handle, no mask): returns a ticket at once;
        when the batch's results reach host memory an 8-byte 1 is written to notify_fd (an eventfd).
        At most two batches in flight, collected in any order (a third raises BusyError).  Raises
        NotImplementedError where hr_index_search must serve (empty index, multi-device handle)."""
        q = np.ascontiguousarray(q, np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be (B, {self.dim}) float32")
        t = ctypes.c_int64(0)
        _check(self.lib.hr_index_search_submit_host(self._h, _ptr(q), q.shape[0], int(k), int(notify_fd),
                                                    ctypes.byref(t)))
        return t.value

    def search_collect(self, ticket: int, B: int, k: int) -> tuple[np.ndarray, np.ndarray]:
        """(scores, rows) of a submitted asynchronous batch (waits if it is not done yet)."""
        s = np.empty((B, k), np.float32)
        r = np.empty((B, k), np.int64)
        _check(self.lib.hr_index_search_collect(self._h, int(ticket), _ptr(s), _ptr(r)))
        return s, r

    def search_poll(self, ticket: int) -> int:
        """State of a submitted asynchronous batch, without waiting: 0 running, 1 ready, 2 ready but its
        collect will run the exact fallback (a corpus pass: collect it off the event loop).  Raises
        BusyError while another call holds the handle."""
        st = ctypes.c_int(0)
        _check(self.lib.hr_index_search_poll(self._h, int(ticket), ctypes.byref(st)))
        return st.value

    def search_finalize(self, ticket: int) -> None:
        """Wait for a submitted batch's guard flags and run its exact fallback (no-op if already final)."""
        _check(self.lib.hr_index_search_finalize(self._h, int(ticket)))

    def host_us(self) -> dict:
        """Host time of the pipelined search: caller us per submit, busiest shard thread us per batch."""
        out = (ctypes.c_double * 3)()
        _check(self.lib.hr_index_host_us(self._h, out))
        return {"submit_us": out[0], "shard_thread_us": out[1], "batches": int(out[2])}

    def search_shard(self, q_ptr: int, B: int, k: int, kc: int, row_offset: int, cand_ptr: int, bound_ptr: int,
                     mask_ptr: int = 0, stream: int = 0, tail_stream: int | None = None,
                     q_ready_event: int = 0) -> None:
        """Per-shard exact top-kc.  With tail_stream (!= stream) the scan runs on `stream` and
        select/rescore on `tail_stream` (pipelined; outputs ready in tail_stream order).
        q_ready_event (raw hipEvent_t, pipelined only): the queries are ready once it completes,
        which lets a large shard prep the queries and run its SAMPLE pass early (see hiprag.h)."""
        if tail_stream is not None:
            _check(self.lib.hr_index_search_shard_async_ev(self._h, ctypes.c_void_p(q_ptr), int(B), int(k), int(kc),
                                                           ctypes.c_void_p(mask_ptr or None), int(row_offset),
                                                           ctypes.c_void_p(cand_ptr), ctypes.c_void_p(bound_ptr),
                                                           ctypes.c_void_p(stream or None),
                                                           ctypes.c_void_p(tail_stream or None),
                                                           ctypes.c_void_p(q_ready_event or None)))
            return
        _check(self.lib.hr_index_search_shard(self._h, ctypes.c_void_p(q_ptr), int(B), int(k), int(kc),
                                              ctypes.c_void_p(mask_ptr or None), int(row_offset),
                                              ctypes.c_void_p(cand_ptr), ctypes.c_void_p(bound_ptr),
                                              ctypes.c_void_p(stream or None)))

    def search_shard_collect(self, q_ptr: int, B: int, kth_ptr: int, cap: int, row_offset: int, cand_ptr: int,
                             bound_ptr: int, mask_ptr: int = 0, stream: int = 0) -> None:
        _check(self.lib.hr_index_search_shard_collect(self._h, ctypes.c_void_p(q_ptr), int(B), ctypes.c_void_p(kth_ptr),
                                                      int(cap), ctypes.c_void_p(mask_ptr or None), int(row_offset),
                                                      ctypes.c_void_p(cand_ptr), ctypes.c_void_p(bound_ptr),
                                                      ctypes.c_void_p(stream or None)))

    def search_shard_exact(self, q_ptr: int, B: int, m: int, row_offset: int, cand_ptr: int, mask_ptr: int = 0,
                           stream: int = 0) -> None:
        """Exact top-m of every query over this shard (the exhaustive pass), B*m sorted records with global rows."""
        _check(self.lib.hr_index_search_shard_exact(self._h, ctypes.c_void_p(q_ptr), int(B), int(m),
                                                    ctypes.c_void_p(mask_ptr or None), int(row_offset),
                                                    ctypes.c_void_p(cand_ptr), ctypes.c_void_p(stream or None)))

    def debug_approx(self, q: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """(approximate MFMA scores B×n, error bound E per query) -- diagnostics."""
        q = np.ascontiguousarray(q, np.float32)
        n, _ = self.size()
        out = np.empty((q.shape[0], n), np.float32)
        e = np.empty(q.shape[0], np.float64)
        _check(self.lib.hr_index_debug_approx(self._h, _ptr(q), q.shape[0], _ptr(out), _ptr(e)))
        return out, e

    def debug_approx8(self, q: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """debug_approx for the shadow-8 scan: (its approximate scores B×n, its error bound E per query)."""
        q = np.ascontiguousarray(q, np.float32)
        n, _ = self.size()
        out = np.empty((q.shape[0], n), np.float32)
        e = np.empty(q.shape[0], np.float64)
        _check(self.lib.hr_index_debug_approx8(self._h, _ptr(q), q.shape[0], _ptr(out), _ptr(e)))
        return out, e

    def set_shadow8(self, mode: int) -> None:
        """Shadow-8 scan of cosine corpora: 0 off, 1 shards beyond 5.1M rows (default), 2 wherever it is built."""
        _check(self.lib.hr_index_set_shadow8(self._h, int(mode)))

    def shadow8_stats(self) -> dict:
        """{"launches": shadow-8 FILTER launches, "kc8": depth the last one planned, "built": bool, "u_x8": float}."""
        out = (ctypes.c_int64 * 3)()
        u = ctypes.c_double(0.0)
        _check(self.lib.hr_index_shadow8_stats(self._h, out, ctypes.byref(u)))
        return {"launches": int(out[0]), "kc8": int(out[1]), "built": bool(out[2]), "u_x8": float(u.value)}

    def last_candidates(self) -> tuple[int, int]:
        t, m = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib.hr_index_last_candidates(self._h, ctypes.byref(t), ctypes.byref(m)))
        return t.value, m.value

    def stats(self) -> dict:
        """Cumulative diagnostics: main scan passes, guard failures (collect fallback), exhaustive passes."""
        out = (ctypes.c_int64 * 3)()
        _check(self.lib.hr_index_stats(self._h, out))
        return {"main_passes": out[0], "guard_failures": out[1], "exhaustive": out[2]}

    def set_q256(self, on: bool) -> None:
        """The 256-query FILTER for 129-256-query batches (default on; off: two 128-query FILTER launches)."""
        _check(self.lib.hr_index_set_q256(self._h, 1 if on else 0))

    def q256_launches(self) -> int:
        """256-query FILTER launches issued so far (hr_index_q256_launches)."""
        out = ctypes.c_int64(0)
        _check(self.lib.hr_index_q256_launches(self._h, ctypes.byref(out)))
        return out.value

    def wide_launches(self) -> int:
        """128-query FILTER launches issued so far (hr_index_wide_launches)."""
        out = ctypes.c_int64(0)
        _check(self.lib.hr_index_wide_launches(self._h, ctypes.byref(out)))
        return out.value

    def wave_tiles(self, cap: int = 1 << 16) -> np.ndarray:
        """Tiles each wave of the most recent k_scan FILTER launch scanned ([group][wave], hr_index_wave_tiles)."""
        out = np.zeros(cap, np.uint32)
        n = ctypes.c_int(0)
        _check(self.lib.hr_index_wave_tiles(self._h, _ptr(out), int(cap), ctypes.byref(n)))
        return out[: n.value].copy()

    def set_persist(self, mode: int) -> None:
        """Persistent FILTER of pipelined shard batches: 0 off, 1 shards of 4.2M-5.1M rows (default), 2 any size."""
        _check(self.lib.hr_index_set_persist(self._h, int(mode)))

    def set_cu_mask(self, cus) -> None:
        """Run this index's internal streams on the CUs listed in `cus` (None / empty: all CUs); see
        hr_index_set_cu_mask and cu_mask_words."""
        words = cu_mask_words(cus) if cus else np.zeros(0, np.uint32)
        _check(self.lib.hr_index_set_cu_mask(self._h, words.ctypes.data if len(words) else None, len(words)))

    def persist_close(self) -> None:
        """No further batch for now: a running persistent FILTER exits once through its batches."""
        _check(self.lib.hr_index_persist_close(self._h))

    def persist_stats(self) -> dict:
        """Persistent FILTER diagnostics: batches served, error word (0 = none), instances that ran."""
        out = (ctypes.c_int64 * 3)()
        _check(self.lib.hr_index_persist_stats(self._h, out))
        return {"batches": out[0], "error": out[1], "runs": out[2]}

    def persist_trace(self, n: int = 64) -> np.ndarray:
        """[epochs, 5] device stamps (us, from the first returned post) of the last n persistent batches: post,
        first / last workgroup start, first / last workgroup arrival."""
        out = np.zeros((max(0, int(n)), 5), np.float64)
        m = ctypes.c_int(0)
        _check(self.lib.hr_index_persist_trace(self._h, int(n), out.ctypes.data, ctypes.byref(m)))
        return out[: m.value].copy()

    def graph_replays(self) -> int:
        """hr_index_search calls answered by a captured HIP graph (hr_index_graph_replays)."""
        n = ctypes.c_int64(0)
        _check(self.lib.hr_index_graph_replays(self._h, ctypes.byref(n)))
        return n.value

    def set_scan_timing(self, every: int) -> None:
        """Record HIP events around every `every`-th main-pass scan (0 = off, the default)."""
        _check(self.lib.hr_index_set_scan_timing(self._h, int(every)))

    def take_scan_times(self, cap: int = 1 << 16) -> tuple[np.ndarray, np.ndarray]:
        """(sample_ms, filter_ms) of every main-pass scan since the previous harvest."""
        a = np.empty(cap, np.float32)
        b = np.empty(cap, np.float32)
        n = ctypes.c_int(0)
        _check(self.lib.hr_index_take_scan_times(self._h, _ptr(a), _ptr(b), int(cap), ctypes.byref(n)))
        return a[: n.value].copy(), b[: n.value].copy()

    def last_scan_ms(self) -> tuple[float, float]:
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        _check(self.lib.hr_index_last_scan_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # -- persistence
    def save(self, path: str) -> None:
        _check(self.lib.hr_index_save(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, path: str, device: int = 0, dim: int | None = None, dtype: str | None = None,
             metric: str | None = None, devices: list[int] | None = None, no_shadows: bool = False
             ) -> "NativeIndex":
        L = load_library()
        h = ctypes.c_void_p()
        devs = [int(d) for d in devices] if devices else [int(device)]
        dev = (ctypes.c_int * len(devs))(*devs)
        _check(L.hr_index_load_ex(os.fsencode(path), len(devs), dev, HR_CREATE_NO_SHADOWS if no_shadows else 0,
                                  ctypes.byref(h)))
        d, dt, m, g = (ctypes.c_int(0) for _ in range(4))
        _check(L.hr_index_info(h, ctypes.byref(d), ctypes.byref(dt), ctypes.byref(m), ctypes.byref(g)))
        # the file's own shape (the dim / dtype / metric arguments are only checked against it)
        dtype_f = {0: "f32", 1: "bf16", 2: "f16"}[dt.value]
        metric_f = {0: "cosine", 1: "ip", 2: "l2"}[m.value]
        if (dim and int(dim) != d.value) or (dtype and DTYPES.get(dtype) != dt.value) or \
                (metric and METRICS.get(metric) != m.value):
            L.hr_index_destroy(h)
            raise ValueError(f"{path}: index is dim={d.value} dtype={dtype_f} metric={metric_f}, "
                             f"not dim={dim} dtype={dtype} metric={metric}")
        return cls(d.value, dtype_f, metric_f, devs[0], devices=devs, _handle=h)


def _csr(lists) -> tuple[np.ndarray, np.ndarray]:
    """uint32 values and int64 offsets of a list of id sequences (or an (ids, offsets) pair, passed through)."""
    if isinstance(lists, tuple) and len(lists) == 2 and isinstance(lists[1], np.ndarray):
        return np.ascontiguousarray(lists[0], np.uint32), np.ascontiguousarray(lists[1], np.int64)
    off = np.zeros(len(lists) + 1, np.int64)
    for i, t in enumerate(lists):
        off[i + 1] = off[i] + len(t)
    vals = np.empty(int(off[-1]), np.uint32)
    for i, t in enumerate(lists):
        vals[off[i]:off[i + 1]] = t
    return vals, off


def lex_pack(token_lists) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host only (hr_lex_pack): the packed rows of raw token-id lists -- (entries `term << 10 | tf` uint32 sorted by
    term within a row, CSR offsets int64, dl uint16)."""
    tok, off = _csr(token_lists)
    n = len(off) - 1
    ent = np.empty(max(len(tok), 1), np.uint32)
    row_off = np.zeros(n + 1, np.int64)
    dl = np.zeros(n, np.uint16)
    _check(load_library().hr_lex_pack(_ptr(tok), _ptr(off), n, _ptr(ent), len(tok), _ptr(row_off), _ptr(dl)))
    return ent[: int(row_off[-1])].copy(), row_off, dl


class NativeLexIndex:
    """The lexical (BM25) forward index on one device (an hr_lex handle); rows are append positions."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.device = int(device)
        h = ctypes.c_void_p()
        _check(self.lib.hr_lex_create(self.device, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.hr_lex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, token_lists) -> int:
        """Append one row per token-id list (ids < 2**22); returns the first new row."""
        tok, off = _csr(token_lists)
        first = ctypes.c_int64(0)
        _check(self.lib.hr_lex_add(self._h, _ptr(tok), _ptr(off), len(off) - 1, ctypes.byref(first)))
        return first.value

    def remove(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1))
        _check(self.lib.hr_lex_remove(self._h, _ptr(r), len(r)))

    def size(self) -> tuple[int, int]:
        n, live = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib.hr_lex_size(self._h, ctypes.byref(n), ctypes.byref(live)))
        return n.value, live.value

    def stats(self) -> tuple[int, int]:
        """(N, sum_dl) over the live rows."""
        n, s = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.lib.hr_lex_stats(self._h, ctypes.byref(n), ctypes.byref(s)))
        return n.value, s.value

    def df(self, terms) -> np.ndarray:
        t = np.ascontiguousarray(np.asarray(terms, np.uint32).reshape(-1))
        out = np.zeros(len(t), np.int32)
        _check(self.lib.hr_lex_df(self._h, _ptr(t), len(t), _ptr(out)))
        return out

    def search(self, query_terms, k: int, mask: np.ndarray | None = None, k1: float = 1.2, b: float = 0.75
               ) -> tuple[np.ndarray, np.ndarray]:
        """(scores float64 (B, k), rows int64 (B, k)) of one term-id list per query; -inf / -1 past the hits."""
        qt, qo = _csr(query_terms)
        B = len(qo) - 1
        s = np.empty((B, k), np.float64)
        r = np.empty((B, k), np.int64)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint64).reshape(-1)
            n_rows = self.size()[0]
            if len(m) * 64 < n_rows:  # the library reads one bit per row
                raise ValueError(f"row mask has {len(m)} words, the index {n_rows} rows (needs {(n_rows + 63) // 64})")
        _check(self.lib.hr_lex_search(self._h, _ptr(qt), _ptr(qo), B, int(k), float(k1), float(b), _ptr(m), _ptr(s),
                                      _ptr(r)))
        return s, r

    def last_ms(self) -> tuple[float, float, int]:
        """Device time of the most recent search: (scan ms, top-k ms, sub-batches) (hr_lex_last_ms)."""
        out = (ctypes.c_double * 3)()
        _check(self.lib.hr_lex_last_ms(self._h, out))
        return out[0], out[1], int(out[2])


def gen_rows_device(seed: int, row0: int, n: int, dim: int, out_ptr: int, stream: int = 0) -> None:
    """Synthetic corpus rows [row0, row0 + n) as fp32 into device memory (the hr_index_add_synthetic generator)."""
    _check(load_library().hr_gen_rows_device(int(seed), int(row0), int(n), int(dim), ctypes.c_void_p(out_ptr),
                                             ctypes.c_void_p(stream or None)))


def ivf_position_mask(ids_ptr: int, n_positions: int, row_mask_ptr: int, n_mask_rows: int, out_ptr: int,
                      stream: int = 0) -> None:
    """uint32-per-tile position mask of a by-id uint64 bitmap, all on the device (hr_ivf_position_mask)."""
    _check(load_library().hr_ivf_position_mask(ctypes.c_void_p(ids_ptr or None), int(n_positions),
                                               ctypes.c_void_p(row_mask_ptr or None), int(n_mask_rows),
                                               ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)))


def _fuse_groups(groups, weights):
    """(offsets int64 (G + 1), weights fp32 (Q) or None) of a list of member counts."""
    counts = np.asarray(list(groups), np.int64).reshape(-1)
    if len(counts) == 0:
        raise ValueError("a fused call needs at least one group")
    if (counts < 1).any() or (counts > HR_FUSE_MAX_MEMBERS).any():
        raise ValueError(f"a group takes 1 to {HR_FUSE_MAX_MEMBERS} members")
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1).astype(np.float32))
        if len(w) != int(off[-1]):
            raise ValueError(f"{len(w)} weights for {int(off[-1])} queries")
    return off, w


def _fuse_mode(mode) -> int:
    if mode not in FUSE_MODES:
        raise ValueError(f"mode must be one of {sorted(FUSE_MODES)} (got {mode!r})")
    return FUSE_MODES[mode]


def fuse_lists(device: int, rows_ptr: int, scores_ptr: int, P: int, groups, k: int, fused_ptr: int, rows_out_ptr: int,
               members_ptr: int = 0, mode: str = "rrf", rrf_k: float = 60.0, weights=None, stream: int = 0) -> None:
    """Ranked lists in device memory fused per group (hr_fuse_lists): ``rows_ptr`` / ``scores_ptr``: Q lists of P
    slots (int64 rows, -1 = padding; fp32 scores), ``groups``: the member count of every group (1 to 16), outputs
    G x k float64 fused scores, int64 rows and (``members_ptr`` != 0) uint32 member bits.  ``mode`` / ``rrf_k`` /
    ``weights`` as NativeIndex.search_fused.  Ordered after ``stream``, which is idle on return."""
    off, w = _fuse_groups(groups, weights)
    _check(load_library().hr_fuse_lists(int(device), ctypes.c_void_p(rows_ptr), ctypes.c_void_p(scores_ptr), int(P),
                                        _ptr(off), _ptr(w), len(off) - 1, int(k), _fuse_mode(mode), float(rrf_k),
                                        ctypes.c_void_p(fused_ptr), ctypes.c_void_p(rows_out_ptr),
                                        ctypes.c_void_p(members_ptr or None), ctypes.c_void_p(stream or None)))


def topk_records(in_ptr: int, B: int, m: int, out_ptr: int, seg_stride: int = 0, seg_off_ptr: int = 0,
                 stream: int = 0) -> None:
    """Exact top-m {score f64, id i64} records per segment, (score desc, id asc) (hr_topk_records)."""
    _check(load_library().hr_topk_records(ctypes.c_void_p(in_ptr), ctypes.c_void_p(seg_off_ptr or None),
                                          int(seg_stride), int(B), int(m), ctypes.c_void_p(out_ptr),
                                          ctypes.c_void_p(stream or None)))


def merge_candidates(device: int, cand_ptr: int, bounds_ptr: int, G: int, B: int, kc: int, k: int, scores_ptr: int,
                     rows_ptr: int, kth_ptr: int, fail_ptr: int, stream: int = 0, cand_rank_stride: int = 0,
                     bound_rank_stride: int = 0) -> None:
    """Merge G ranks' candidates; strides (bytes) default to the dense [G][B][kc] / [G][B] layouts."""
    L = load_library()
    if cand_rank_stride or bound_rank_stride:
        _check(L.hr_merge_candidates_strided(int(device), ctypes.c_void_p(cand_ptr), ctypes.c_void_p(bounds_ptr),
                                             int(cand_rank_stride or B * kc * 16), int(bound_rank_stride or B * 8),
                                             int(G), int(B), int(kc), int(k), ctypes.c_void_p(scores_ptr),
                                             ctypes.c_void_p(rows_ptr), ctypes.c_void_p(kth_ptr),
                                             ctypes.c_void_p(fail_ptr), ctypes.c_void_p(stream or None)))
        return
    _check(L.hr_merge_candidates(int(device), ctypes.c_void_p(cand_ptr), ctypes.c_void_p(bounds_ptr),
                                 int(G), int(B), int(kc), int(k), ctypes.c_void_p(scores_ptr),
                                 ctypes.c_void_p(rows_ptr), ctypes.c_void_p(kth_ptr),
                                 ctypes.c_void_p(fail_ptr), ctypes.c_void_p(stream or None)))


def merge_sorted(device: int, cand_ptr: int, G: int, B: int, m: int, k: int, scores_ptr: int, rows_ptr: int,
                 stream: int = 0, cand_rank_stride: int = 0) -> None:
    """Merge G ranks' sorted exact top-m lists (search_shard_exact records) into the top-k (hr_merge_sorted)."""
    _check(load_library().hr_merge_sorted(int(device), ctypes.c_void_p(cand_ptr), int(cand_rank_stride), int(G),
                                          int(B), int(m), int(k), ctypes.c_void_p(scores_ptr),
                                          ctypes.c_void_p(rows_ptr), ctypes.c_void_p(stream or None)))


def pool_normalize(hidden_ptr: int, dtype: str, mask_ptr: int, B: int, T: int, H: int, n_instr: int, out_ptr: int,
                   stream: int = 0) -> None:
    _check(load_library().hr_pool_normalize(ctypes.c_void_p(hidden_ptr), DTYPES[dtype], ctypes.c_void_p(mask_ptr),
                                            int(B), int(T), int(H), int(n_instr), ctypes.c_void_p(out_ptr),
                                            ctypes.c_void_p(stream or None)))


def pool_normalize_packed(hidden_ptr: int, dtype: str, cu_ptr: int, B: int, H: int, n_instr: int, out_ptr: int,
                          stream: int = 0) -> None:
    """K7 over packed hidden states (rows [cu[b], cu[b+1]) are sequence b; cu: B+1 int32 on the device)."""
    _check(load_library().hr_pool_normalize_packed(ctypes.c_void_p(hidden_ptr), DTYPES[dtype], ctypes.c_void_p(cu_ptr),
                                                   int(B), int(H), int(n_instr), ctypes.c_void_p(out_ptr),
                                                   ctypes.c_void_p(stream or None)))


def hash_words(data: bytes, offsets, first_id: int, span: int, cap: int = -1, cls_id: int = -1, sep_id: int = -1):
    """Host text kernel of the offline tokenizer (hr_hash_words): ASCII texts packed in `data` with int64
    `offsets` (n+1) -> (ids int64 flat, lengths int64 (n,)).  No GPU involved."""
    import numpy as np

    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    cap_ids = len(data) + 2 * n + 1  # every token takes at least one byte
    ids = np.empty(cap_ids, np.int64)
    lengths = np.empty(max(n, 0), np.int64)
    _check(load_library().hr_hash_words(data, offsets.ctypes.data_as(ctypes.c_void_p), int(n), int(first_id),
                                        int(span), int(cap), int(cls_id), int(sep_id),
                                        ids.ctypes.data_as(ctypes.c_void_p), int(cap_ids),
                                        lengths.ctypes.data_as(ctypes.c_void_p)))
    return ids[:int(lengths.sum())], lengths


_ATTN_DT = {"bfloat16": "bf16", "float16": "f16"}


def attn_varlen(qkv, cu, B: int, nH: int, d: int, max_len: int, scale: float, out=None):
    """Short-sequence attention of a packed batch (hr_attn_varlen): qkv (N, 3 nH d) bf16 / f16 device tensor, cu
    (B + 1,) int32 device offsets -> (N, nH d).  Returns None where the kernel does not apply (d != 64, a sequence
    longer than 64 tokens, ...): the caller runs the flash varlen kernel instead."""
    import torch

    dt = _ATTN_DT.get(str(qkv.dtype).replace("torch.", ""))
    if dt is None or d != 64 or max_len > 64 or not qkv.is_contiguous():
        return None
    n = qkv.shape[0]
    out = out if out is not None else torch.empty((n, nH * d), dtype=qkv.dtype, device=qkv.device)
    rc = load_library().hr_attn_varlen(ctypes.c_void_p(qkv.data_ptr()), DTYPES[dt], ctypes.c_void_p(cu.data_ptr()),
                                       int(B), int(nH), int(d), int(max_len), float(scale),
                                       ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream))
    if rc == E_UNSUPPORTED:
        return None
    _check(rc)
    return out


def gelu_erf_(x):
    """In-place exact GELU of a bf16 / f16 device tensor (hr_gelu_erf); returns x, or None if it does not apply."""
    import torch

    dt = _ATTN_DT.get(str(x.dtype).replace("torch.", ""))
    if dt is None or not x.is_contiguous():
        return None
    rc = load_library().hr_gelu_erf(ctypes.c_void_p(x.data_ptr()), DTYPES[dt], x.numel(),
                                    ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc == E_UNSUPPORTED:
        return None
    _check(rc)
    return x


def add_layernorm(x, r, weight, bias, eps: float):
    """K8: LayerNorm(x + r) with affine weight/bias over the last dim, one fused HIP kernel (torch
    tensors on one device, same dtype, contiguous; runs on the current stream)."""
    import torch

    names = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
    if x.dtype not in names or r.dtype != x.dtype or weight.dtype != x.dtype or bias.dtype != x.dtype:
        raise ValueError("add_layernorm: x, r, weight and bias must share one of f32 / bf16 / f16")
    if x.shape != r.shape or weight.shape != (x.shape[-1],) or bias.shape != (x.shape[-1],):
        raise ValueError("add_layernorm: shape mismatch")
    x, r = x.contiguous(), r.contiguous()
    out = torch.empty_like(x)
    H = x.shape[-1]
    if x.numel() == 0:  # no rows (an empty tensor's pointer is null, which the C entry rejects)
        return out
    _check(load_library().hr_add_layernorm(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(r.data_ptr()),
                                           ctypes.c_void_p(weight.data_ptr()), ctypes.c_void_p(bias.data_ptr()),
                                           ctypes.c_void_p(out.data_ptr()), x.numel() // H, H, float(eps),
                                           DTYPES[names[x.dtype]],
                                           ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    return out
