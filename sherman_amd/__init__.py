"""sherman_amd — MI355X-native Sherman B+tree hot path (batched get / insert).

Python view of the C-ABI in include/sherman_amd.h (libsherman_amd.so, built
in-tree by `make -C sherman_amd`).  The host interface mirrors the reference
`Tree` (include/Tree.h:42-63): `search`, `insert`, `del_`, `range_query`,
plus the batched forms the GPU path is built around.  Batch methods take
torch CUDA (HIP) tensors or raw device pointers; torch is used only as the
device-memory / stream plumbing.

There is no CPU fallback: if the HIP library is missing or no GPU is
visible, constructing a Tree raises.
"""
import ctypes  # noqa: F401  (ctypes and os stay names of the package, as before the split)
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SHM_LIB_PATH: another build of the library (A/B of builds, tools/ab_builds.sh)
LIB_PATH = os.environ.get("SHM_LIB_PATH") or os.path.join(_HERE, "libsherman_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sherman_amd.h")
_lib = None  # the loaded library (_abi.lib)

from ._abi import (ABI_VERSION, DIR_FORMS, INTERNAL_CARDINALITY, KEY_MAX,  # noqa: E402,F401
                   LEAF_CARDINALITY, PAGE_SIZE, SHM_E2BIG, SHM_EAGAIN, SHM_EINVAL, SHM_EIO,
                   SHM_ENOMEM, SHM_ENOSPC, SHM_FLAG_AUTO_SORT_GETS, SHM_FLAG_LEAF_DIR,
                   SHM_FLAG_PAGE_CHECK, SHM_FLAG_SORT_GETS, SHM_FLAG_TOP_LDS, SHM_OK,
                   ShermanError, ShmBulkPlan, ShmConfig, ShmDirStats, ShmError, ShmIndexStats,
                   ShmOrderStats, ShmProfile, ShmStats, _HOOKS, _SIGNATURES, _check, _hooks,
                   _host_u64, _ptr, _stream_ptr, build, from_i64, header_symbols, lib, to_i64,
                   u32, u64, vp)
from ._pending import PendingRange, PendingScan, PendingSlots, _StreamDone  # noqa: E402,F401
from ._tree_hooks import LocalGroup, check_image, order_limits  # noqa: E402,F401
from .cshard import CShard  # noqa: E402,F401
from .tree import Tree, bulk_plan, rebalance_plan  # noqa: E402,F401

_record_on = _StreamDone  # the name call sites used before they constructed _StreamDone
