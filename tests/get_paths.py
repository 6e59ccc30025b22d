"""Host model of which path answers a batched get (get_sum.hip k_get_sum), in
numpy, sharing no code with the library.

A read phase's get reads its key's bucket of the key-value table first
(valtab.h); a live bucket answers it, found or absent.  Behind a dead bucket,
or without a table, an exact pair-form directory's value-form entry answers
it from its inline copies (layout.h kDirVals).  Every other get reads the
leaves.  The index statistics count all three together (a table answer is a
"dir_fp_hit" that read no entry), so a test that wants to prove one path
must know, per probe, which path the tree's own state sends it down.  That is
what classify() says, from the raw dumps alone (Tree.vt_dump, Tree.dir_dump)
and the formats restated in tests/valtab_model.py and tests/dir_model.py.

Classes, one per key:

  "table"  a table is present and trusted and the tree has no page check;
           the key is neither 0 nor KEY_MAX; lo <= key, its bucket index is
           below the bucket count, and the bucket is not dead.
  "value"  not "table"; the tree has no page check (the value form reads no
           page, so it has no versions to check); the directory is exact and
           in pair form; the key's entry is usable in value form.
  "leaf"   everything else.  A stored key of this class cannot be answered
           without reading at least one leaf entry, whichever walk it takes.

The rules the tests draw from that (assert_rules), none with a measured
constant:

  1. a batch whose probes are all "table" or "value" reads no leaf entry;
  2. any batch reads at least as many leaf entries as it holds stored probes
     of class "leaf".

One exception to rule 1, stated here because the classes above do not see
it: an ABSENT key of class "value" whose top 32 offset bits equal the split
point of its entry's second leaf (ties()) is started at that leaf with a safe
start kept aside, and get_sum.hip answers "absent" from the entry only without
one; such a key walks and may read a false candidate.  Stored keys are never
affected (the inline copy answers them first).  split() keeps such keys out of
the batches held to rule 1.
"""
import os

import numpy as np

import dir_model as dm
import valtab_model as vm

U64 = np.uint64
KEY_MAX = U64(0xFFFFFFFFFFFFFFFF)
TABLE, VALUE, LEAF = "table", "value", "leaf"


def _directory(directory):
    """(dir_model.Directory or None, form) of a Tree.dir_dump() result"""
    ent, info = directory
    ent = np.asarray(ent)
    if ent.size == 0:
        return None, info.get("form", "none")
    return dm.Directory(ent, info["lo"], info["shift"]), info["form"]


def classify(keys, table, directory, flags):
    """The class of each key.

    table:     Tree.vt_dump()'s (buckets, {"lo", "shift", "trusted"}); no
               rows: no table.
    directory: Tree.dir_dump()'s (entries, {"lo", "shift", "form"}).
    flags:     {"exact": the directory is exact (Tree.dir_stats()["exact"]),
                "page_check": the tree was made with page_check=True}.
    Returns an array of "table" / "value" / "leaf"."""
    keys = np.asarray(keys, dtype=U64)
    page_check = bool(flags.get("page_check", False))
    out = np.full(keys.size, LEAF, dtype="<U5")

    buckets, tinfo = table
    buckets = np.asarray(buckets, dtype=U64).reshape(-1, 2 * vm.SLOTS)
    in_table = np.zeros(keys.size, dtype=bool)
    if buckets.shape[0] and tinfo["trusted"] and not page_check:
        n = buckets.shape[0]
        lo, shift = U64(tinfo["lo"]), U64(tinfo["shift"])
        ok = (keys != U64(0)) & (keys != KEY_MAX) & (keys >= lo)
        with np.errstate(over="ignore"):
            b = (keys - lo) >> shift
        ok &= b < U64(n)
        b = np.where(ok, b, U64(0)).astype(np.int64)
        in_table = ok & ~vm.dead(buckets)[b]
    out[in_table] = TABLE

    d, form = _directory(directory)
    if d is not None and form == "pairs" and bool(flags.get("exact", False)) and not page_check:
        p, cov = d.prefix_of(keys)
        out[~in_table & cov & d.val_usable[p]] = VALUE
    return out


def ties(keys, directory):
    """Whether each key's directory lookup is a tie at a split point
    (dir_entry.h dir_start_e): the entry is not in fingerprint form, the
    prefix is wider than 2^32 keys, and the top 32 bits of the key's offset
    in the prefix equal the split point of the leaf after the one it would
    start in.  get_sum.hip keeps a safe start for such a key and then answers
    "absent" from the leaves only."""
    keys = np.asarray(keys, dtype=U64)
    d, _ = _directory(directory)
    out = np.zeros(keys.size, dtype=bool)
    if d is None or d.shift <= 32:
        return out
    p, cov = d.prefix_of(keys)
    a, _ = d.bounds(p)
    with np.errstate(over="ignore"):
        tk = ((keys - a) >> U64(d.shift - 32)).astype(np.int64)
    nl = d.nl[p]
    split = d.ent[p, 4:7].astype(np.int64)  # split points of leaves 1..3
    i = np.zeros(keys.size, dtype=np.int64)
    for j in range(3):
        i += (nl > j + 1) & (split[:, j] < tk)
    nxt = split[np.arange(keys.size), np.minimum(i, 2)]
    return cov & ~d.fp_form[p] & (i + 1 < nl) & (nxt == tk)


def tally(cls):
    """probes per class, as a dict with all three classes"""
    cls = np.asarray(cls)
    return {c: int((cls == c).sum()) for c in (TABLE, VALUE, LEAF)}


def assert_rules(cls, found, st, label=""):
    """Rules 1 and 2 on one batch's index statistics; prints the probes per
    class and the counters.  (A batch with absent ties() keys must not be
    held to rule 1: split() keeps them out.)"""
    cls, found = np.asarray(cls), np.asarray(found).astype(bool)
    n = tally(cls)
    stored_leaf = int((found & (cls == LEAF)).sum())
    print(f"{label}: probes {n} stored-leaf {stored_leaf} gets={st['gets']} hits={st['hits']} "
          f"entry_reads={st['entry_reads']} dir_fp_hits={st['dir_fp_hits']} "
          f"right_moves={st['right_moves']}")
    if n[LEAF] == 0:
        assert st["entry_reads"] == 0, (label, n, st)
    assert st["entry_reads"] >= stored_leaf, (label, n, stored_leaf, st)
    return n


def with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def without_table(fn):
    """fn() with SHM_VALTAB=0: a tree created inside has no bucket table (the
    variable is read when a tree is created, and restored here)"""
    return with_env("SHM_VALTAB", "0", fn)


def dumps(t, page_check=False):
    """(table, directory, flags) of a tree, as classify() takes them"""
    return t.vt_dump(), t.dir_dump(), {"exact": bool(t.dir_stats()["exact"]),
                                       "page_check": page_check}


def split(t, keys, page_check=False):
    """(quiet, classes): quiet marks the probes rule 1 covers -- class
    "table" or "value" and no ties() key -- the others go with the "leaf"
    batch"""
    table, directory, flags = dumps(t, page_check)
    cls = classify(keys, table, directory, flags)
    return (cls != LEAF) & ~((cls == VALUE) & ties(keys, directory)), cls


def assert_equal(keys, ov, of, gv, gf):
    bad = np.nonzero((np.asarray(of) != np.asarray(gf)) | (np.asarray(ov) != np.asarray(gv)))[0]
    if bad.size:
        lines = [f"key={int(keys[i]):#x} oracle=({of[i]},{int(ov[i])}) gpu=({gf[i]},{int(gv[i])})"
                 for i in bad[:8]]
        raise AssertionError(f"{bad.size} mismatches:\n" + "\n".join(lines))


def check_paths(t, orc, keys, table_on, label, upper=None, page_check=False):
    """One batch held to the oracle and to the rules, path by path.

    Always: the whole batch equals the oracle and obeys rules 1 and 2.
    Table off: the model gives no probe to "table", and upper(st, keys,
    found), the caller's own upper bound on the entry reads, is held on the
    whole batch.  Table on: the probes rule 1 covers (split()) go again on
    their own -- no entry read, same answers; the others go again -- rule 2;
    and the probes the model does not give to the table go again for
    upper().  Returns the whole batch's (values, found, stats, classes)."""
    keys = np.ascontiguousarray(keys, dtype=U64)

    def one(k, what):
        gv, gf, st, cls = searched(t, k, page_check)
        assert_equal(k, *orc.search_batch(k), gv, gf)
        assert st["gets"] == int((k != KEY_MAX).sum()), (what, st)
        assert_rules(cls, gf, st, f"{label} [{what}]")
        return gv, gf, st, cls

    whole = one(keys, "whole batch")
    cls = whole[3]
    if not table_on:
        assert not (cls == TABLE).any(), (label, tally(cls))
        if upper is not None:
            upper(whole[2], keys, whole[1])
        return whole
    quiet, cls2 = split(t, keys, page_check)
    assert np.array_equal(cls, cls2)
    if quiet.any():
        _, _, st, _ = one(keys[quiet], "table + value")
        assert st["entry_reads"] == 0, (label, st)
    if (~quiet).any():
        one(keys[~quiet], "leaf")
    rest = cls != TABLE
    if upper is not None and rest.any():
        _, gf, st, _ = one(keys[rest], "not the table's")
        upper(st, keys[rest], gf)
    return whole


def searched(t, keys, page_check=False):
    """One stats-bearing search_batch of `keys`: (values, found flags, the
    index statistics of that batch alone, the model's class per key).  The
    dumps are taken before the search."""
    import torch

    keys = np.ascontiguousarray(keys, dtype=U64)
    cls = classify(keys, *dumps(t, page_check))
    k = torch.from_numpy(keys.view(np.int64)).cuda()
    v = torch.empty_like(k)
    f = torch.empty(k.numel(), dtype=torch.uint8, device="cuda")
    t.profile(False, index_stats=True)
    t.index_stats()  # (reset)
    try:
        t.search_batch(k, v, f)
        t.synchronize()
        st = t.index_stats()
    finally:
        t.profile(False)
    return v.cpu().numpy().view(U64), f.cpu().numpy(), st, cls
