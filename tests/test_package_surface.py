"""The package's surface after the split into modules: every name the package,
Tree and CShard had when sherman_amd was one file is still there (tests, tools
and bench.py reach for the private ones too), and the test hooks stay on the
mixin, off the public class.  No GPU.

The three lists are dir() of the one-file package (non-dunder names), recorded
before the split; a name may be added to them, none dropped."""
import sherman_amd as shm
from sherman_amd._tree_hooks import _TreeHooks

PACKAGE = [
    "ABI_VERSION", "CShard", "DIR_FORMS", "HEADER_PATH", "INTERNAL_CARDINALITY", "KEY_MAX",
    "LEAF_CARDINALITY", "LIB_PATH", "LocalGroup", "PAGE_SIZE", "PendingRange", "PendingScan",
    "PendingSlots", "SHM_E2BIG", "SHM_EAGAIN", "SHM_EINVAL", "SHM_EIO", "SHM_ENOMEM",
    "SHM_ENOSPC", "SHM_FLAG_AUTO_SORT_GETS", "SHM_FLAG_LEAF_DIR", "SHM_FLAG_PAGE_CHECK",
    "SHM_FLAG_SORT_GETS", "SHM_FLAG_TOP_LDS", "SHM_OK", "ShermanError", "ShmBulkPlan",
    "ShmConfig", "ShmDirStats", "ShmError", "ShmIndexStats", "ShmOrderStats", "ShmProfile",
    "ShmStats", "Tree", "_HERE", "_HOOKS", "_SIGNATURES", "_StreamDone", "_check", "_hooks",
    "_host_u64", "_lib", "_ptr", "_record_on", "_stream_ptr", "build", "bulk_plan",
    "check_image", "ctypes", "from_i64", "header_symbols", "lib", "order_limits", "os",
    "rebalance_plan", "to_i64", "u32", "u64", "vp",
]

TREE = [
    "_dev", "bulk_load", "check", "close", "compact", "count", "count_batch", "del_",
    "del_batch", "dir_config", "dir_dump", "dir_stats", "dir_verify", "dump_image", "export",
    "floor_batch", "gen_keys", "get_forms", "hash_keys", "index_stats", "insert",
    "insert_apply", "insert_batch", "insert_batch_async", "insert_batch_padded", "insert_order",
    "last_chunk", "last_error", "load_image", "lock_bench", "lower_bound_batch", "mixed_batch",
    "order_read", "order_stats", "profile", "profile_read", "quantile_keys",
    "range_query_batch", "range_query_batch_async", "range_query_slots", "rank_batch",
    "read_i64", "route_bucket", "route_permute", "route_unpermute", "rscan_batch", "scan_batch",
    "search", "search_batch", "select_batch", "seq_jump", "set_key_range", "side_dump", "stats",
    "synchronize", "vt_dump", "vt_stats",
]

CSHARD = [
    "close", "force_route", "insert", "local", "range_query", "range_query_async", "rebalance",
    "search", "search_begin", "search_end", "set_splitters", "splitters", "synchronize",
]


def test_every_name_is_still_there():
    assert len(PACKAGE) == 60 and len(TREE) == 57 and len(CSHARD) == 13
    for what, obj, names in (("sherman_amd", shm, PACKAGE), ("Tree", shm.Tree, TREE),
                             ("CShard", shm.CShard, CSHARD)):
        gone = [n for n in names if not hasattr(obj, n)]
        assert not gone, f"{what} lost {gone}"


def test_hooks_live_on_the_mixin():
    """A Tree method whose docstring starts "Test hook" or "Diagnostics" is
    defined on _TreeHooks, not on Tree itself."""
    hooks = [n for n in dir(shm.Tree)
             if callable(getattr(shm.Tree, n))
             and (getattr(shm.Tree, n).__doc__ or "").startswith(("Test hook", "Diagnostics"))]
    assert len(hooks) >= 10, hooks  # the ten the one-file Tree carried
    for n in hooks:
        assert n in vars(_TreeHooks), f"{n} is a hook: define it in _tree_hooks.py"
        assert n not in vars(shm.Tree), f"{n} is a hook: it does not belong on the public class"
    assert issubclass(shm.Tree, _TreeHooks)
