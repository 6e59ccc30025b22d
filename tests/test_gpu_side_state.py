"""The leaf summary lines and occupancy bounds after every leaf writer.

Each arena page carries a 64 B summary line (highest fence, leaf tag, one key
fingerprint per slot) and an occupancy byte that are not part of its bytes.
The summary walk of the get, the page readers' short reads and the page sweeps
of the directory's and the bucket table's builds trust them, and a fault in
them shows only to a get of exactly that key through exactly that path.  Here
the whole side state is dumped (Tree.side_dump) after every writer -- the
empty leaf of create, the in-place upsert, the split writers and the root
that grows in place, the deletes, the bulk load and its line clearing, the
rebuild after a loaded image -- and checked against the dumped pages by a host
model that shares no code with the kernels (tests/state_model.py).

assert_side (test_gpu_tall.py; the tall, arena-full and unreached-page tests
call it too) also runs the structural check and reads the error bits; the
contents are compared with a dict of the ops applied.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bulk_model  # noqa: E402
import dir_model  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, gpu_search, host, lib_ok, U64  # noqa: E402
import state_model as sm  # noqa: E402
import test_gpu_tall as tall  # noqa: E402

ARENA = 64 << 20
MAX_BATCH = 1 << 12
HANDOFF = 0x100  # kErrHandoff

assert_side = tall.assert_side


def tree(**args):
    return shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, **args)


class Model:
    """the contents as the ops applied so far leave them (the last writer of
    a key in a chunk wins; value 0 deletes)"""

    def __init__(self):
        self.d = {}

    def apply(self, keys, vals):
        for k, v in zip(np.asarray(keys, dtype=U64).tolist(), np.asarray(vals, dtype=U64).tolist()):
            if v:
                self.d[k] = v
            else:
                self.d.pop(k, None)

    def pairs(self):
        k = np.array(sorted(self.d), dtype=U64)
        return k, np.array([self.d[x] for x in k.tolist()], dtype=U64)


def put(t, model, keys, vals, mode=None):
    """one chunk on the tree and on the model; mode: a writer mode of
    test_gpu_tall.MODES ("abort" leaves the hand-off bit, read and reset here)"""
    keys, vals = np.asarray(keys, dtype=U64), np.asarray(vals, dtype=U64)
    if mode is not None:
        assert shm._hooks().shm__upper_force(t.h, tall.MODES[mode]) == 0
    t.insert_batch(dev(keys), dev(vals))
    e = t.last_error(reset=True)
    assert not e["bits"] & ~(HANDOFF if mode == "abort" else 0), e
    model.apply(keys, vals)


def check(t, model, what, pages=None):
    """assert_side, and the pages hold the model's pairs; returns the dump"""
    img, root, lines, hw = assert_side(t, what, pages)
    dir_model.Image(img, root).assert_equals(*model.pairs())
    return img, root, lines, hw


def leaves_of(img, root):
    return np.nonzero(sm.reached_leaves(img, root)[1])[0]


def spread(rng, n):
    """n distinct keys over the whole range, none 0 or 2^64 - 1, all even"""
    k = np.unique(rng.integers(1, (1 << 63) - 1, 2 * n, dtype=np.uint64) * U64(2))
    return rng.permutation(k)[:n]


# ---- 1, 2: the empty leaf, and growth key by key ----------------------------------
def test_fresh_handle(lib_ok):
    t = tree()
    img, root, lines, hw = check(t, Model(), "fresh", pages=8)
    assert img.size == 2 * ib.PAGE and root >> 26 == 1
    assert lines[1, sm.SUM_OFF_TAG] == sm.SUM_LEAF
    assert lines[1, :8].tolist() == [0xFF] * 8 and not lines[1, sm.SUM_OFF_FP:].any()
    assert not lines[0].any() and not lines[2:].any()
    t.close()


def test_growth_key_by_key(lib_ok):
    """One key per chunk up to 60: slots fill in order (hw = the count), the
    54th key splits the root leaf, the root page turns internal in place and
    loses its tag, and the new leaves' lines are exact with hw = their count."""
    t, model = tree(), Model()
    keys = spread(np.random.default_rng(2), 60)
    for i, k in enumerate(keys.tolist(), 1):
        put(t, model, [k], [k ^ 0x1111])
        img, root, lines, hw = check(t, model, f"key {i}")
        st = t.stats()
        leaves = leaves_of(img, root)
        tight = sm.hw_tight(img, root, hw.size)
        if i <= 53:
            assert st["root_level"] == 0 and leaves.tolist() == [1] and hw[1] == i, (i, st, hw[:4])
        else:
            assert st["root_level"] == 1 and root >> 26 == 1 and leaves.size == 2, (i, st, leaves)
            assert lines[1, sm.SUM_OFF_TAG] == 0 and 1 not in leaves
            assert np.array_equal(hw[leaves], tight[leaves]), (i, hw[leaves], tight[leaves])
            k_, v_ = sm._slots(img.reshape(-1, ib.PAGE)[leaves])
            assert np.array_equal(hw[leaves], (v_ != 0).sum(axis=1)), (i, hw[leaves])
            assert int((v_ != 0).sum()) == i
        # the lines are the model's, byte for byte
        assert np.array_equal(lines[leaves], sm.side_expected(img, root, hw.size)[leaves]), i
    t.close()


# ---- 3: one chunk into an empty tree, each writer mode -----------------------------------
@pytest.mark.parametrize("mode", list(tall.MODES))
@pytest.mark.parametrize("n", [1, 2, 53, 54, 55, 200, 2500])
def test_one_chunk_into_an_empty_tree(lib_ok, n, mode):
    """No split (1, 2, 53), the two-way split (54, 55), a k-way split of up to
    six pages (200) and a root leaf that grows twice within the chunk (2,500)."""
    t, model = tree(), Model()
    keys = spread(np.random.default_rng([3, n]), n)
    put(t, model, keys, keys ^ U64(0x2222), mode=mode)
    img, root, lines, hw = check(t, model, f"{n} keys, {mode}")
    st = t.stats()
    leaves = leaves_of(img, root)
    assert st["root_level"] == (0 if n <= 53 else 1 if n <= 200 else 2), st
    if n <= 55:
        assert leaves.size == (1 if n <= 53 else 2), leaves
    if n == 200:
        assert 4 <= leaves.size <= 6, leaves
    if n == 2500:
        assert leaves.size > 61, leaves.size  # more than one level-1 page can name
    # a page written whole holds its entries in slots [0, count)
    assert np.array_equal(hw[leaves], sm.hw_tight(img, root, hw.size)[leaves])
    t.close()


# ---- 4: slot reuse ------------------------------------------------------------------
def test_slot_reuse(lib_ok):
    """Four full leaves from a bulk load (slot = rank): deletes at the ends
    and in the middle of a leaf, of a leaf's top slots and of a whole leaf;
    then new keys whose first empty slot lies below, inside and above the
    bound the deletes left; a key deleted and stored again, in two chunks and
    in one."""
    t, model = tree(), Model()
    keys = (np.arange(1, 4 * 53 + 1, dtype=U64) << U64(40))
    vals = keys ^ U64(0x3333)
    t.bulk_load(dev(keys), dev(vals), leaf_fill=53, internal_fill=60)
    model.apply(keys, vals)
    img, root, lines, hw = check(t, model, "loaded")
    leaves = leaves_of(img, root)
    assert leaves.size == 4 and (hw[leaves] == 53).all()
    k0, _ = sm._slots(img.reshape(-1, ib.PAGE)[leaves])
    assert np.array_equal(k0[:, :53].ravel(), keys)  # slot = rank, leaf by leaf
    page = {j: int(leaves[np.nonzero(k0[:, 0] == keys[53 * j])[0][0]]) for j in range(4)}
    leaf = {j: keys[53 * j:53 * j + 53] for j in range(4)}

    def delete(ks, what):
        put(t, model, ks, np.zeros(len(ks), dtype=U64))
        return check(t, model, what)

    _, _, lines, hw = delete(leaf[0][[0, 26, 52]], "slots 0, 26, 52 deleted")
    assert hw[page[0]] in (52, 53, 0xFF) and not lines[page[0], sm.SUM_OFF_FP + 26]
    _, _, lines, hw = delete(leaf[1][43:], "top ten slots deleted")
    assert not lines[page[1], sm.SUM_OFF_FP + 43:sm.SUM_OFF_FP + 53].any()
    _, _, lines, hw = delete(leaf[2], "a whole leaf deleted")
    assert not lines[page[2], sm.SUM_OFF_FP:].any() and lines[page[2], sm.SUM_OFF_TAG] == sm.SUM_LEAF
    print("bounds after the deletes:", [int(hw[page[j]]) for j in range(4)])
    # first empty slot 0, below the bound 52 of leaf 0
    new = leaf[0][[3]] + U64(1)
    put(t, model, new, new ^ U64(0x4444))
    img, _, lines, hw = check(t, model, "a new key below the bound")
    k_, v_ = sm._slots(img.reshape(-1, ib.PAGE)[page[0]:page[0] + 1])
    assert k_[0, 0] == new[0] and v_[0, 0] != 0
    # slots 26 (inside) and 52 (above the bound) of leaf 0, slots 43 and 44 of
    # leaf 1 (at its bound and above), slots 0 and 1 of the emptied leaf 2
    new = np.concatenate([leaf[0][[5, 7]], leaf[1][[1, 2]], leaf[2][[9, 11]]]) + U64(1)
    put(t, model, new, new ^ U64(0x4444))
    img, _, lines, hw = check(t, model, "new keys inside and above the bounds")
    pg = img.reshape(-1, ib.PAGE)
    for j, slots in ((0, [26, 52]), (1, [43, 44]), (2, [0, 1])):
        k_, v_ = sm._slots(pg[page[j]:page[j] + 1])
        assert (v_[0, slots] != 0).all() and np.isin(k_[0, slots], new).all(), (j, slots)
    assert t.stats()["pages_used"] == 5
    # the same key deleted and stored again
    k = leaf[3][[17]]
    delete(k, "a key deleted")
    put(t, model, k, k ^ U64(0x5555))
    check(t, model, "and stored again")
    k2 = leaf[3][[30, 30]]
    put(t, model, k2, np.array([0, int(k2[0]) ^ 0x6666], dtype=U64))
    check(t, model, "deleted and stored in one chunk")
    put(t, model, k2, np.array([int(k2[0]) ^ 0x7777, 0], dtype=U64))
    check(t, model, "stored and deleted in one chunk")
    t.close()


# ---- 5: overwrites change nothing ----------------------------------------------------------
@pytest.mark.parametrize("loaded", [False, True])
def test_overwrites_leave_the_side_state_as_it_is(lib_ok, loaded):
    t, model = tree(), Model()
    keys = spread(np.random.default_rng(5), 2500)
    if loaded:
        keys = np.sort(keys)
        t.bulk_load(dev(keys), dev(keys ^ U64(0x1111)))
        model.apply(keys, keys ^ U64(0x1111))
    else:
        put(t, model, keys, keys ^ U64(0x1111))
    _, _, lines0, hw0 = check(t, model, "before")
    over = keys[::5]
    put(t, model, over, over ^ U64(0x9999))
    _, _, lines, hw = check(t, model, "after")
    assert np.array_equal(lines, lines0) and np.array_equal(hw, hw0)
    t.close()


# ---- 6: a loaded image ----------------------------------------------------------------------
def test_loaded_entry_states(lib_ok):
    """The entry-states image with soil pages behind it: the rebuild gives
    exactly the model's lines (torn entries with their key's fingerprint,
    deleted slots and stale copies 0, the soil untagged) and every bound
    unknown; then one chunk that overwrites a torn key, puts new keys into
    leaves with deleted slots and deletes a key whose entry is at version 15."""
    img, root, info = ib.build_entry_states()
    n_img = img.size // ib.PAGE
    soil, _ = ib.soil_pages(6, ib.soil_keys(info), seed=4, first_page=n_img)
    both = ib.with_soil(img, soil)
    t = tree()
    t.load_image(both, root)
    dump, droot, lines, hw = assert_side(t, "as loaded", pages=n_img + 6 + 4)
    assert np.array_equal(dump[ib.PAGE:], both[ib.PAGE:]) and droot == root
    assert (hw[:n_img + 6] == 0xFF).all()
    assert np.array_equal(lines, sm.side_expected(both, root, lines.shape[0]))
    s = info["slots"]
    fp = lines[s["page"], sm.SUM_OFF_FP + s["slot"]]
    torn, gone = s["kind"] == ib.TORN, (s["kind"] == ib.DELETED) | (s["kind"] == ib.STALE_COPY)
    assert torn.sum() == 25 and np.array_equal(fp[torn], sm.key_fp(s["key"][torn]))
    assert gone.sum() > 50 and not fp[gone].any()
    assert not lines[n_img:].any()
    # the chunk
    model = Model()
    held = s["value"] != 0  # the torn entries hold a value: the tree's writers take them as stored
    model.apply(s["key"][held], s["value"][held])
    tk = s["key"][torn][:1]
    dk = s["key"][s["kind"] == ib.DELETED]
    new = dk[::3] + U64(8)  # absent, inside the fences of a leaf with deleted slots
    vk = info["v15_keys"][:1]
    keys = np.concatenate([tk, new, vk])
    vals = np.concatenate([tk ^ U64(0x7777), new ^ U64(0x8888), np.zeros(1, dtype=U64)])
    used = t.stats()["pages_used"]
    t.insert_batch(dev(keys), dev(vals))
    model.apply(keys, vals)
    assert t.stats()["pages_used"] == used
    dump, droot, lines, hw = assert_side(t, "after the chunk", pages=n_img + 6 + 4)
    # every slot with a value, torn or not, against the model
    pg = dump.reshape(-1, ib.PAGE)
    at = leaves_of(dump, droot)
    k_, v_ = sm._slots(pg[at])
    o = np.argsort(k_[v_ != 0])
    mk, mv = model.pairs()
    assert np.array_equal(k_[v_ != 0][o], mk) and np.array_equal(v_[v_ != 0][o], mv)
    # the upsert wrote these pages' bounds (a delete alone leaves a bound as it is)
    touched = np.unique(s["page"][np.isin(s["key"], np.concatenate([tk, dk[::3]]))])
    assert (hw[touched] != 0xFF).all(), hw[touched]
    gv, gf = gpu_search(t, keys)
    assert np.array_equal(gf != 0, vals != 0) and np.array_equal(gv[vals != 0], vals[vals != 0])
    t.close()


# ---- 7: bulk loads ----------------------------------------------------------------------------
def shape_pairs(n, lf, inf):
    k = bulk_model.shape_keys(n, bulk_model.shape_kind(n, lf, inf))
    return k, bulk_model.shape_vals(k)


@pytest.mark.parametrize("n,lf,inf", [s for s in bulk_model.SHAPES if s[0] < 6000])
def test_bulk_load_shapes(lib_ok, n, lf, inf):
    t, model = tree(), Model()
    k, v = shape_pairs(n, lf, inf)
    t.bulk_load(dev(k), dev(v), leaf_fill=lf, internal_fill=inf)
    model.apply(k, v)
    img, root, lines, hw = check(t, model, f"bulk load {n, lf, inf}")
    pl = bulk_model.plan(n, lf, inf)
    assert img.size // ib.PAGE == pl["pages"] + 1
    reached, leaf = sm.reached_leaves(img, root)
    assert leaf.sum() == pl["level_pages"][0]
    assert np.array_equal(hw[leaf], sm.hw_tight(img, root, hw.size)[leaf])
    assert (hw[reached & ~leaf] == 0xFF).all()
    assert np.array_equal(lines[leaf], sm.side_expected(img, root, hw.size)[leaf])
    t.close()


def test_a_smaller_load_clears_the_lines_behind_it(lib_ok):
    """5,000 keys, then 54 over them; that tree grown by a chunk, then 100
    keys over it.  The dump is asked up to the largest tree's end: every line
    in [next_page, that end) is zero.  Then 5,000 keys again, every third
    deleted, and compact()."""
    t, model = tree(), Model()
    k, v = shape_pairs(5000, 0, 0)
    t.bulk_load(dev(k), dev(v))
    old_end = t.stats()["pages_used"] + 1
    assert (assert_side(t, "5,000 keys")[2][1:old_end, sm.SUM_OFF_TAG] == sm.SUM_LEAF).sum() >= 139
    k, v = shape_pairs(54, 53, 60)
    t.bulk_load(dev(k), dev(v), leaf_fill=53, internal_fill=60)
    model.apply(k, v)
    img, root, lines, hw = check(t, model, "54 keys over 5,000", pages=old_end)
    assert img.size // ib.PAGE == 4 and not lines[4:].any() and lines.shape[0] == old_end > 140
    # a tree grown by chunks, shrunk by a load
    k = spread(np.random.default_rng(7), 2500)
    put(t, model, k, k ^ U64(0x1111))
    grown = t.stats()["pages_used"] + 1
    check(t, model, "grown by a chunk", pages=old_end)
    t.bulk_load(dev(np.sort(k[:100])), dev(np.sort(k[:100]) ^ U64(0x2222)))
    model = Model()
    model.apply(k[:100], k[:100] ^ U64(0x2222))
    img, root, lines, hw = check(t, model, "100 keys over the grown tree", pages=old_end)
    assert img.size // ib.PAGE < grown and not lines[img.size // ib.PAGE:].any()
    # compact
    k, v = shape_pairs(5000, 0, 0)
    t.bulk_load(dev(k), dev(v))
    model = Model()
    model.apply(k, v)
    put(t, model, k[::3], np.zeros(k[::3].size, dtype=U64))
    check(t, model, "every third key deleted", pages=old_end)
    t.compact()
    img, root, lines, hw = check(t, model, "compacted", pages=old_end)
    assert img.size // ib.PAGE < old_end and not lines[img.size // ib.PAGE:].any()
    t.close()


# ---- 8: the queued forms ----------------------------------------------------------------------
def mixed_chunks(rng, model_keys, n_chunks, size):
    """chunks of new spread keys, a clustered run that splits a leaf, and
    overwrites and deletes of keys stored so far"""
    out, have = [], list(model_keys)
    for c in range(n_chunks):
        new = spread(rng, size)
        base = int(rng.integers(1 << 40, 1 << 62)) * 2
        run = np.arange(base, base + 80, 2, dtype=U64)  # 40 neighbours
        k = [new, run]
        v = [new ^ U64(0x1111), run ^ U64(0x2222)]
        if have:
            old = np.array(have, dtype=U64)
            pick = rng.permutation(old.size)[:size // 2]
            over, dele = old[pick[::2]], old[pick[1::2]]
            k += [over, dele]
            v += [over ^ U64(0xA000 + c), np.zeros(dele.size, dtype=U64)]
            have = list(set(have) - set(dele.tolist()))
        have += new.tolist() + run.tolist()
        k, v = np.concatenate(k), np.concatenate(v)
        o = rng.permutation(k.size)
        out.append((k[o], v[o]))
    return out


def test_ordered_chunks_on_two_streams(lib_ok):
    """Eight chunks through insert_order on one stream and insert_apply on
    another, a search between the chunks, every chunk keeping the directory."""
    t, model = tree(), Model()
    t.dir_config(maint="always")
    rng = np.random.default_rng(8)
    chunks = mixed_chunks(rng, [], 8, 600)
    tensors = [(dev(k), dev(v)) for k, v in chunks]
    probe = dev(np.concatenate([k[:256] for k, _ in chunks]))
    s_ord, s_app = torch.cuda.Stream(), torch.cuda.Stream()
    s_ord.wait_stream(torch.cuda.current_stream())
    s_app.wait_stream(torch.cuda.current_stream())
    outs = []
    tickets = [t.insert_order(*tensors[0], stream=s_ord)]
    for i in range(len(tensors)):
        if i + 1 < len(tensors):
            tickets.append(t.insert_order(*tensors[i + 1], stream=s_ord))
        t.insert_apply(tickets[i], stream=s_app)
        v = torch.empty_like(probe)
        f = torch.empty(probe.numel(), dtype=torch.uint8, device="cuda")
        t.search_batch(probe, v, f, stream=s_app)
        outs.append((v, f))
    t.synchronize()
    torch.cuda.synchronize()
    for k, v in chunks:
        model.apply(k, v)
    check(t, model, "eight ordered chunks")
    mk, mv = model.pairs()
    for a in range(0, mk.size, MAX_BATCH):
        gv, gf = gpu_search(t, mk[a:a + MAX_BATCH])
        assert gf.all() and np.array_equal(gv, mv[a:a + MAX_BATCH])
    t.close()


def test_async_chunks_and_a_mixed_batch(lib_ok):
    t, model = tree(), Model()
    t.dir_config(maint="always")
    rng = np.random.default_rng(9)
    chunks = mixed_chunks(rng, [], 5, 600)
    tensors = [(dev(k), dev(v)) for k, v in chunks]
    for kd, vd in tensors[:4]:
        t.insert_batch_async(kd, vd)
    t.synchronize()
    for k, v in chunks[:4]:
        model.apply(k, v)
    check(t, model, "four queued chunks")
    mk, mv = model.pairs()
    gk = dev(mk[:2000])
    gv = torch.empty_like(gk)
    gf = torch.empty(gk.numel(), dtype=torch.uint8, device="cuda")
    t.mixed_batch(gk, gv, gf, *tensors[4])
    t.synchronize()
    # the gets saw the tree before the batch's inserts
    assert gf.cpu().numpy().all() and np.array_equal(host(gv), mv[:2000])
    model.apply(*chunks[4])
    check(t, model, "a mixed batch")
    t.close()


# ---- 9: seeded rounds ---------------------------------------------------------------------------
@pytest.mark.parametrize("leaf_dir", [True, False])
def test_seeded_rounds(lib_ok, leaf_dir):
    """Twelve rounds of about 700 ops each (some 2^13 in all): new spread keys, a
    clustered run of 40 that splits its leaf, overwrites and deletes of stored
    keys; a read phase between the rounds, so that a tree with a directory
    keeps it through every chunk."""
    t, model = tree(leaf_dir=leaf_dir), Model()
    rng = np.random.default_rng([9, int(leaf_dir)])
    total = 0
    for r in range(12):
        k, v = mixed_chunks(rng, model.d.keys(), 1, 450)[0]
        total += k.size
        put(t, model, k, v)
        check(t, model, f"round {r}")
        mk, mv = model.pairs()
        for _ in range(3):
            gv, gf = gpu_search(t, mk[:1024])
        assert gf.all() and np.array_equal(gv, mv[:1024]), r
    assert 7000 <= total <= 9500, total
    t.close()
