"""Splitter routing, rebalance and shm_tree_set_key_range at the C-ABI
boundary, without a GPU: the symbols are declared, bound and exported
unmangled, the ABI number is unchanged, the header states the contract, and
rejected arguments return before the handle or the GPU is used."""
import ctypes
import re
import subprocess

import sherman_amd as shm

NEW = (("shm_route_bucket_bounds", 9), ("shm_shard_set_splitters", 2),
       ("shm_shard_get_splitters", 2), ("shm_rebalance_plan", 6), ("shm_shard_rebalance", 5),
       ("shm_tree_set_key_range", 3))


def test_new_symbols_are_declared_bound_and_exported():
    sig = {n: (r, a) for n, r, a in shm._SIGNATURES}
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for name, nargs in NEW:
        assert name in shm.header_symbols()
        assert sig[name][0] is ctypes.c_int and len(sig[name][1]) == nargs
        assert re.search(r"\bT %s$" % name, out, re.M)  # unmangled => extern "C"
    for attr in ("set_splitters", "splitters", "rebalance"):
        assert callable(getattr(shm.CShard, attr))
    assert callable(shm.Tree.set_key_range) and callable(shm.rebalance_plan)
    assert shm.lib().shm_abi_version() == shm.ABI_VERSION == 11  # additions only
    assert re.search(r"#define SHM_ABI_VERSION 11\b", open(shm.HEADER_PATH).read())


def test_the_header_declares_the_documented_signatures():
    txt = re.sub(r"\s+", " ", open(shm.HEADER_PATH).read())
    for decl in (
            "int shm_route_bucket_bounds(shm_tree *t, const uint64_t *keys, uint64_t n, "
            "uint32_t num_shards, const uint64_t *splitters_host, uint64_t *counts_out, "
            "uint64_t *keys_out, uint32_t *perm_out, void *stream);",
            "int shm_shard_set_splitters(shm_shard *s, const uint64_t *splitters_host);",
            "int shm_shard_get_splitters(shm_shard *s, uint64_t *out_host);",
            "int shm_rebalance_plan(const uint64_t *counts, uint32_t P, uint32_t rank, "
            "uint64_t *cut, uint64_t *send_cnt, uint64_t *recv_cnt);",
            "int shm_shard_rebalance(shm_shard *s, uint32_t leaf_fill, uint32_t internal_fill, "
            "uint64_t *n_local_out, void *stream);",
            "int shm_tree_set_key_range(shm_tree *t, uint64_t key_lo, uint32_t key_bits);"):
        assert decl in txt, decl


def comment_of(decl):
    txt = open(shm.HEADER_PATH).read()
    at = txt.index(decl)
    # one line: a phrase may be wrapped in the header
    return re.sub(r"\s*\n\s*\*\s*", " ", txt[txt.rindex("/*", 0, at):at])


def test_the_header_comments_state_the_contract():
    c = comment_of("int shm_route_bucket_bounds(")
    for word in ("HOST", "ascending", "number of splitters <= it", "empty shard", "highest shard",
                 "NULL", "bit for bit", "SHM_EINVAL", "kKeyMax"):
        assert word in c, word
    c = comment_of("int shm_shard_set_splitters(")
    for word in ("NULL", "equal slices", "every rank", "one exchange", "MOVES NO DATA",
                 "owns the consequences", "empty", "SHM_EINVAL", "shm_shard_search_begin"):
        assert word in c, word
    c = comment_of("int shm_rebalance_plan(")
    for word in ("no handle, no GPU", "floor(p N / P)", "at most 1", "send_cnt", "recv_cnt",
                 "P > 16", "SHM_EINVAL"):
        assert word in c, word
    c = comment_of("int shm_shard_rebalance(")
    for word in ("Collective", "exclusive", "synchronising", "shm_compact", "16 B per pair",
                 "cut[j]", "source-rank order", "key_lo", "ceil(log2", "shm_bulk_load",
                 "pages_used", "repeated splitters", "world 1", "in place", "SHM_ENOMEM",
                 "exactly as they were", "n_local_out"):
        assert word in c, word
    c = comment_of("int shm_tree_set_key_range(")
    for word in ("get ordering", "leaf directory", "bucket table", "found exactly",
                 "read as 64", "key_lo = 0", "Exclusive", "synchronising", "shm_bulk_load",
                 "SHM_EINVAL", "shm_insert_order"):
        assert word in c, word


def test_rejected_arguments_return_before_any_use_of_handle_or_gpu():
    """Argument errors on a null handle and on a handle that is no tree (a
    zeroed host buffer, which a call that went on would dereference and
    lock)."""
    L = shm.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)
    n = ctypes.c_uint64(77)
    kmax = (1 << 64) - 1
    desc = (ctypes.c_uint64 * 2)(9, 8)
    top = (ctypes.c_uint64 * 2)(9, kmax)
    good = (ctypes.c_uint64 * 2)(9, 9)
    for h in (None, ctypes.addressof(fake)):
        rb = L.shm_route_bucket_bounds
        assert rb(h, p, 4, 3, desc, p, p, p, None) == shm.SHM_EINVAL    # descending
        assert rb(h, p, 4, 3, top, p, p, p, None) == shm.SHM_EINVAL     # a splitter == kKeyMax
        assert rb(h, p, 4, 0, good, p, p, p, None) == shm.SHM_EINVAL    # no shards
        assert rb(h, p, 4, 65, good, p, p, p, None) == shm.SHM_EINVAL
        assert rb(h, p, 4, 3, good, None, p, p, None) == shm.SHM_EINVAL  # counts_out
        assert rb(h, None, 4, 3, good, p, p, p, None) == shm.SHM_EINVAL  # keys with n > 0
        assert L.shm_tree_set_key_range(h, 0, 65) == shm.SHM_EINVAL
        assert L.shm_tree_set_key_range(h, 5, 1 << 31) == shm.SHM_EINVAL
    assert L.shm_tree_set_key_range(None, 0, 26) == shm.SHM_EINVAL
    assert L.shm_route_bucket_bounds(None, p, 4, 3, good, p, p, p, None) == shm.SHM_EINVAL
    assert L.shm_shard_set_splitters(None, good) == shm.SHM_EINVAL
    assert L.shm_shard_set_splitters(None, None) == shm.SHM_EINVAL
    assert L.shm_shard_get_splitters(None, p) == shm.SHM_EINVAL
    assert L.shm_shard_rebalance(None, 0, 0, ctypes.byref(n), None) == shm.SHM_EINVAL
    assert L.shm_shard_rebalance(ctypes.addressof(fake), 0, 0, None, None) == shm.SHM_EINVAL
    assert n.value == 77
    assert all(x == 0 for x in buf)
    assert all(b == 0 for b in fake.raw)
