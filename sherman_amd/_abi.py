"""The ctypes mirror of include/sherman_amd.h, the loader of
libsherman_amd.so, and the small conversions every call goes through."""
import ctypes
import os
import sys

# LIB_PATH, HEADER_PATH and the loaded library (_lib) are attributes of the
# package itself, set in __init__.py before this module is imported: tests and
# tools read and patch them there (tests/test_capi.py), so lib() reads them
# there too
_pkg = sys.modules[__package__]

SHM_OK = 0
SHM_EINVAL = -22
SHM_ENOMEM = -12
SHM_EIO = -5
SHM_EAGAIN = -11
SHM_E2BIG = -7
SHM_ENOSPC = -28
SHM_FLAG_SORT_GETS = 0x1
SHM_FLAG_LEAF_DIR = 0x2
SHM_FLAG_AUTO_SORT_GETS = 0x4
SHM_FLAG_TOP_LDS = 0x8
SHM_FLAG_PAGE_CHECK = 0x10

KEY_MAX = (1 << 64) - 1
PAGE_SIZE = 1024
LEAF_CARDINALITY = 54       # include/Tree.h:193-195
INTERNAL_CARDINALITY = 61   # include/Tree.h:189-191

u64 = ctypes.c_uint64
u32 = ctypes.c_uint32
vp = ctypes.c_void_p


class ShmConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("node_id", ctypes.c_uint16),
        ("reserved0", ctypes.c_uint16),
        ("flags", ctypes.c_uint32),
        ("arena_bytes", u64),
        ("max_batch", u64),
        ("num_locks", u32),
        ("sort_bits", u32),
        ("key_lo", u64),
        ("key_bits", u32),
        ("reserved1", u32),
    ]


class ShmStats(ctypes.Structure):
    _fields_ = [
        ("root_ptr", u64),
        ("root_level", u32),
        ("height", u32),
        ("pages_used", u64),
        ("pages_capacity", u64),
        ("arena_bytes", u64),
        ("batches", u64),
        ("splits", u64),
        ("last_error", u32),
        ("reserved", u32),
    ]


class ShmBulkPlan(ctypes.Structure):
    _fields_ = [("pages", u64), ("root_level", u32), ("reserved", u32), ("level_pages", u64 * 8)]


class ShmError(ctypes.Structure):
    _fields_ = [("bits", u32), ("chunk", u32), ("status", ctypes.c_int32), ("resumed", u32)]


class ShmIndexStats(ctypes.Structure):
    _fields_ = [(f, u64) for f in ("gets", "start_internal", "right_moves", "page_hops",
                                   "entry_reads", "hits", "dir_fp_hits")]


class ShmDirStats(ctypes.Structure):
    _fields_ = [("form", u32), ("bits", u32), ("entries", u64), ("bytes", u64), ("builds", u64),
                ("pages_at_build", u64), ("pages_since_build", u64),
                ("last_build_ms", ctypes.c_double), ("total_build_ms", ctypes.c_double),
                ("maintained", u32), ("exact", u32)]


class ShmOrderStats(ctypes.Structure):
    _fields_ = [("units", u64), ("pairs", u64), ("bytes", u64), ("builds", u64),
                ("last_build_ms", ctypes.c_double)]


DIR_FORMS = {0: "none", 1: "fingerprints", 2: "pairs"}


class ShmProfile(ctypes.Structure):
    _fields_ = [
        ("calls", u64),
        ("queries", u64),
        ("order_ms", ctypes.c_double),
        ("walk_ms", ctypes.c_double),
        ("insert_calls", u64),
        ("insert_ops", u64),
        ("insert_ms", ctypes.c_double),
        ("upsert_ms", ctypes.c_double),
        ("range_calls", u64),
        ("range_queries", u64),
        ("range_ms", ctypes.c_double),
        ("insert_unique", u64),
        ("insert_dels", u64),
        ("insert_staged", u64),
        ("walk_kernel_ms", ctypes.c_double),
    ]


ABI_VERSION = 11  # SHM_ABI_VERSION in include/sherman_amd.h

# (name, restype, argtypes) — every symbol declared in include/sherman_amd.h
_SIGNATURES = [
    ("shm_config_init", ctypes.c_int, [ctypes.POINTER(ShmConfig)]),
    ("shm_tree_create", ctypes.c_int, [ctypes.POINTER(ShmConfig), ctypes.POINTER(vp)]),
    ("shm_tree_destroy", ctypes.c_int, [vp]),
    ("shm_strerror", ctypes.c_char_p, [ctypes.c_int]),
    ("shm_abi_version", ctypes.c_int, []),
    ("shm_search_batch", ctypes.c_int, [vp, vp, u64, vp, vp, vp]),
    ("shm_insert_batch", ctypes.c_int, [vp, vp, vp, u64, vp]),
    ("shm_insert_batch_async", ctypes.c_int, [vp, vp, vp, u64, vp]),
    ("shm_insert_order", ctypes.c_int, [vp, vp, vp, u64, vp, ctypes.POINTER(u32)]),
    ("shm_insert_apply", ctypes.c_int, [vp, u32, vp]),
    ("shm_mixed_batch", ctypes.c_int, [vp, vp, u64, vp, vp, vp, vp, u64, vp]),
    ("shm_del_batch", ctypes.c_int, [vp, vp, u64, vp]),
    ("shm_range_query", ctypes.c_int, [vp, vp, vp, u64, vp, vp, vp, vp]),
    ("shm_range_query_batch", ctypes.c_int,
     [vp, vp, vp, u64, vp, vp, vp, u64, ctypes.POINTER(u64), vp]),
    ("shm_range_query_batch_async", ctypes.c_int,
     [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp]),
    ("shm_range_query_slots", ctypes.c_int, [vp, vp, vp, u64, u64, vp, vp, vp, vp]),
    ("shm_scan_batch", ctypes.c_int, [vp, vp, vp, u64, u64, vp, vp, vp, vp, vp]),
    ("shm_rscan_batch", ctypes.c_int, [vp, vp, vp, u64, u64, vp, vp, vp, vp, vp]),
    ("shm_rank_batch", ctypes.c_int, [vp, vp, u64, vp, vp, vp]),
    ("shm_count_batch", ctypes.c_int, [vp, vp, vp, u64, vp, vp, vp]),
    ("shm_select_batch", ctypes.c_int, [vp, vp, u64, vp, vp, vp, vp, vp]),
    ("shm_order_stats", ctypes.c_int, [vp, ctypes.POINTER(ShmOrderStats)]),
    ("shm_stats", ctypes.c_int, [vp, ctypes.POINTER(ShmStats)]),
    ("shm_dump_image", ctypes.c_int, [vp, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
    ("shm_load_image", ctypes.c_int, [vp, vp, u64, u64]),
    ("shm_bulk_plan", ctypes.c_int, [u64, u32, u32, ctypes.POINTER(ShmBulkPlan)]),
    ("shm_bulk_load", ctypes.c_int, [vp, vp, vp, u64, u32, u32, vp]),
    ("shm_export", ctypes.c_int, [vp, u64, u64, vp, vp, u64, ctypes.POINTER(u64), vp]),
    ("shm_compact", ctypes.c_int, [vp, u32, u32, vp]),
    ("shm_check", ctypes.c_int, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
    ("shm_synchronize", ctypes.c_int, [vp]),
    ("shm_read_words", ctypes.c_int, [vp, vp, u64, vp, vp]),
    ("shm_last_error", ctypes.c_int, [vp, ctypes.POINTER(ShmError), ctypes.c_int]),
    ("shm_last_chunk", u32, [vp]),
    ("shm_profile_enable", ctypes.c_int, [vp, ctypes.c_int]),
    ("shm_profile_read", ctypes.c_int, [vp, ctypes.POINTER(ShmProfile), ctypes.c_int]),
    ("shm_index_stats", ctypes.c_int, [vp, ctypes.POINTER(ShmIndexStats), ctypes.c_int]),
    ("shm_dir_stats", ctypes.c_int, [vp, ctypes.POINTER(ShmDirStats)]),
    ("shm_route_bucket", ctypes.c_int, [vp, vp, u64, u32, vp, vp, vp, vp]),
    ("shm_route_bucket_bounds", ctypes.c_int, [vp, vp, u64, u32, vp, vp, vp, vp, vp]),
    ("shm_route_permute", ctypes.c_int, [vp, vp, vp, u64, vp, vp]),
    ("shm_route_unpermute", ctypes.c_int, [vp, vp, vp, u64, vp, vp]),
    ("shm_route_unpermute_found", ctypes.c_int, [vp, vp, vp, u64, vp, vp, vp]),
    ("shm_tree_max_batch", u64, [vp]),
    ("shm_nccl_unique_id", ctypes.c_int, [vp, u64]),
    ("shm_shard_create", ctypes.c_int, [vp, vp, u64, u32, u32, ctypes.POINTER(vp)]),
    ("shm_shard_create_with_comm", ctypes.c_int, [vp, vp, u32, u32, ctypes.POINTER(vp)]),
    ("shm_shard_destroy", ctypes.c_int, [vp]),
    ("shm_shard_search", ctypes.c_int, [vp, vp, u64, vp, vp, vp]),
    ("shm_shard_search_begin", ctypes.c_int, [vp, vp, u64, vp, ctypes.POINTER(u32)]),
    ("shm_shard_search_end", ctypes.c_int, [vp, u32, vp, vp]),
    ("shm_shard_insert", ctypes.c_int, [vp, vp, vp, u64, vp]),
    ("shm_shard_range_query", ctypes.c_int,
     [vp, vp, vp, u64, u64, vp, vp, vp, u64, ctypes.POINTER(u64), vp]),
    ("shm_shard_range_query_async", ctypes.c_int,
     [vp, vp, vp, u64, u64, vp, vp, vp, u64, u64, vp, vp]),
    ("shm_shard_synchronize", ctypes.c_int, [vp]),
    ("shm_shard_range_values", ctypes.c_int, [vp, vp, u64, vp]),
    ("shm_tree_set_key_range", ctypes.c_int, [vp, u64, u32]),
    ("shm_shard_set_splitters", ctypes.c_int, [vp, vp]),
    ("shm_shard_get_splitters", ctypes.c_int, [vp, vp]),
    ("shm_rebalance_plan", ctypes.c_int, [vp, u32, u32, vp, vp, vp]),
    ("shm_shard_rebalance", ctypes.c_int, [vp, u32, u32, ctypes.POINTER(u64), vp]),
    ("shm_lock_bench", ctypes.c_int, [vp, vp, u64, vp]),
    ("shm_gen_keys", ctypes.c_int, [vp, u64, u64, u64, vp, vp]),
    ("shm_hash_keys", ctypes.c_int, [vp, vp, u64, u64, vp, vp]),
]

# library-internal test hooks: an in-process group of P shard handles on one
# GPU whose collectives are device copies (csrc/shard_xport.cpp), the forced
# route (csrc/shard_hooks.cpp), and the tree's own (csrc/tree*.cpp)
_HOOKS = [
    ("shm__local_group_create", ctypes.c_int, [u32, ctypes.POINTER(vp)]),
    ("shm__local_group_destroy", ctypes.c_int, [vp]),
    ("shm__shard_create_local", ctypes.c_int, [vp, vp, u32, ctypes.POINTER(vp)]),
    ("shm__upper_force", ctypes.c_int, [vp, u32]),
    ("shm__hog", ctypes.c_int, [u32, u64, vp]),
    ("shm__mark", ctypes.c_int, [u32, vp]),
    ("shm__early_pages", ctypes.c_int, [vp, ctypes.POINTER(u64)]),
    ("shm__dir_config", ctypes.c_int, [vp, ctypes.c_int, u64]),
    ("shm__shard_force_route", ctypes.c_int, [vp, ctypes.c_int]),
    ("shm__dir_verify", ctypes.c_int, [vp, ctypes.POINTER(u64)]),
    ("shm__dir_dump", ctypes.c_int, [vp, vp, u64, ctypes.POINTER(u64)]),
    ("shm__vt_stats", ctypes.c_int, [vp, ctypes.POINTER(u64)]),
    ("shm__vt_dump", ctypes.c_int, [vp, vp, u64, ctypes.POINTER(u64)]),
    ("shm__get_forms", ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
    ("shm__seq_jump", ctypes.c_int, [vp, ctypes.c_int, u32]),
    ("shm__order_read", ctypes.c_int, [vp, u32, vp, vp, vp, ctypes.POINTER(u64)]),
    ("shm__order_limits", ctypes.c_int, [ctypes.POINTER(u64)]),
    ("shm__insert_batch_padded", ctypes.c_int, [vp, vp, vp, u64, vp]),
    ("shm__side_dump", ctypes.c_int, [vp, vp, vp, u64, ctypes.POINTER(u64)]),
    ("shm__check_image", ctypes.c_int, [vp, u64, u64, ctypes.c_uint16, ctypes.POINTER(u64),
                                        ctypes.POINTER(ctypes.c_int)]),
]

_no_hook = None  # the first hook of _HOOKS the loaded library lacks


def build():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", _pkg._HERE, "-j8"])


def lib():
    """Load libsherman_amd.so (fails loudly if it was not built)."""
    global _no_hook
    if _pkg._lib is None:
        path = _pkg.LIB_PATH
        if not os.path.exists(path):
            raise ImportError(
                f"{path} missing: build it with `make -C sherman_amd` "
                "(there is no CPU fallback)")
        L = ctypes.CDLL(path)
        # an older build under SHM_LIB_PATH (A/B of builds) lacks newer calls and hooks
        older = bool(os.environ.get("SHM_LIB_PATH"))
        no_hook = None
        for name, res, args in _SIGNATURES + _HOOKS:
            f = getattr(L, name, None)
            if f is not None:
                f.restype, f.argtypes = res, args
            elif older:
                continue
            elif name.startswith("shm__"):
                no_hook = no_hook or name  # raised when a hook is used (_hooks)
            else:
                raise ImportError(f"{path} lacks {name}: rebuild with `make -C sherman_amd`")
        if L.shm_abi_version() != ABI_VERSION:
            raise ImportError(f"{path} has ABI {L.shm_abi_version()}, this package "
                              f"expects {ABI_VERSION}: rebuild with `make -C sherman_amd`")
        _pkg._lib, _no_hook = L, no_hook
    return _pkg._lib


def _hooks():
    """The library for a call of one of _HOOKS."""
    L = lib()
    if _no_hook:
        raise AttributeError(f"{_pkg.LIB_PATH} lacks the hook {_no_hook}")
    return L


class ShermanError(RuntimeError):
    def __init__(self, rc, what=""):
        self.rc = rc
        msg = lib().shm_strerror(rc).decode()
        super().__init__(f"{what}: {msg} ({rc})" if what else f"{msg} ({rc})")


def _check(rc, what):
    if rc != SHM_OK:
        raise ShermanError(rc, what)


def header_symbols(path=_pkg.HEADER_PATH):
    """Names of every function declared in include/sherman_amd.h."""
    import re
    txt = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:int|uint32_t|uint64_t|const char \*)\s*(shm_\w+)\s*\(",
                                 txt, re.M)))


def from_i64(x):
    return x & KEY_MAX


def to_i64(x):
    """u64 -> signed int64 bit pattern (torch has no uint64 arithmetic)."""
    x = from_i64(x)
    return x - (1 << 64) if x >= (1 << 63) else x


def _host_u64(words):
    """A ctypes array of u64 from Python ints / numpy u64 (None stays None)."""
    if words is None:
        return None
    w = [from_i64(int(x)) for x in words]
    return (u64 * max(len(w), 1))(*w)


def _as_dict(s):
    """A ctypes struct as {field: value}."""
    return {f: getattr(s, f) for f, _ in s._fields_}


def _ptr(x):
    """Device pointer of a torch tensor / int / None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


def _stream_ptr(stream):
    """hipStream_t for the C-ABI; default = torch's current stream so the
    library is ordered after the torch ops that produced its inputs."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    if isinstance(stream, int):
        return stream or None
    return stream.cuda_stream or None


def _range_bufs(n, cap, dev):
    """A range query's result buffers on `dev`: (counts[n], offsets[n],
    values[cap]), int64."""
    import torch
    return (torch.empty(n, dtype=torch.int64, device=dev),
            torch.empty(n, dtype=torch.int64, device=dev),
            torch.empty(cap, dtype=torch.int64, device=dev))
