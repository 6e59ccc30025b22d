"""The reader rule for a leaf entry -- value != 0 and (f ^ r) & 0xF == 0 --
on the GPU, over an image whose leaves hold every kind of slot
(tests/image_builder.build_entry_states): valid entries, deleted slots with
stale key bytes (some a stale copy of a key that is live in another slot of
the same leaf), torn entries (value != 0, f != r) and valid entries at
version 15.

Ten kernels restate that rule.  A tree written by this library or by the
oracle never holds an entry that fails its second half at rest, so no other
test would notice the version compare missing from any of them.

Read-only except the last step, and no write touches a leaf that holds a
torn entry: what the writers do with one is out of scope.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, gpu_search, host, lib_ok, SENT, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402
from scan_model import ScanModel  # noqa: E402

KEY_MAX = (1 << 64) - 1
ARENA = 64 << 20
MAX_BATCH = 1 << 14


@pytest.fixture(scope="module")
def states():
    img, root, info = ib.build_entry_states()
    img.setflags(write=False)
    return img, root, info


def load(states, **tree_args):
    """The image in a Tree and in an oracle, after the oracle's structural
    check and both CPU readers agreed on its contents."""
    img, root, info = states
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=1 << 20)
    rc, shape = orc.check()
    assert rc == 0, rc
    assert shape["keys"] == info["n_valid"] + info["n_torn"] and shape["height"] == 3
    ok, ov = orc.dump()
    dir_model.Image(img, root).assert_equals(ok, ov)
    assert np.array_equal(np.sort(ok), info["keys"])
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, **tree_args)
    t.load_image(img, root)
    return t, orc, info


def probes(info):
    every = np.concatenate([info["keys"], info["torn"], info["deleted"], info["stale_copy"]])
    p = np.concatenate([every, every + U64(1), every - U64(1), info["leaf_lo"],
                        info["leaf_lo"] - U64(1), np.array([0, KEY_MAX - 1], dtype=U64)])
    return np.unique(p[p != U64(KEY_MAX)])


def check_gets(t, orc, info, what):
    probe = probes(info)
    ov, of = orc.search_batch(probe)
    # the oracle against what the builder stored
    at = np.minimum(np.searchsorted(info["keys"], probe), info["keys"].size - 1)
    stored = info["keys"][at] == probe
    assert np.array_equal(of.astype(bool), stored)
    assert np.array_equal(ov, np.where(stored, info["vals"][at], U64(0)))
    for order in (np.arange(probe.size), np.random.default_rng(5).permutation(probe.size)):
        gv, gf = gpu_search(t, probe[order])
        bad = np.nonzero((gf != of[order]) | (gv != ov[order]))[0]
        assert bad.size == 0, (what, [(hex(int(probe[order][i])), int(gf[i]), hex(int(gv[i])))
                                      for i in bad[:8]])
    for name in ("torn", "deleted"):
        gv, gf = gpu_search(t, info[name])
        assert not gf.any() and not gv.any(), (what, name)
    gv, gf = gpu_search(t, info["stale_copy"])
    assert gf.all() and np.array_equal(gv, info["stale_copy"] ^ U64(ib.VALUE_XOR)), what
    assert t.last_error()["bits"] == 0, (what, t.last_error())


def check_scans(t, orc, info, what):
    model = ScanModel(info["keys"], info["vals"])
    probe = probes(info)
    # range scans: the whole key space, every leaf's fences, around every
    # torn, deleted and copied key
    odd = np.concatenate([info["torn"], info["deleted"], info["stale_copy"]])
    lo = np.concatenate([np.array([0], dtype=U64), info["leaf_lo"], odd - U64(1), odd])
    hi = np.concatenate([np.array([KEY_MAX - 1], dtype=U64),
                         np.append(info["leaf_lo"][1:], U64(KEY_MAX - 1)), odd + U64(1), odd])
    counts, vals = t.range_query_batch(dev(lo), dev(hi))
    counts, vals = counts.cpu().numpy(), host(vals)
    a = np.searchsorted(model.keys, lo, side="left")
    b = np.searchsorted(model.keys, hi, side="right")
    assert np.array_equal(counts, b - a), (what, np.nonzero(counts != b - a)[0][:8])
    off = 0
    for i in range(lo.size):  # the oracle walks the same pages: the same order
        ref, n = orc.range_query(int(lo[i]), int(hi[i]), cap=1 << 12)
        assert n == counts[i] and np.array_equal(vals[off:off + n], ref), (what, i)
        off += n
    for limit in (1, 7, 54, 200):
        n = probe.size
        keys = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
        vals = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
        c, k, v = t.scan_batch(dev(probe), limit, keys=keys, vals=vals).result()
        mc, mk, mv, w = model.scan(probe, limit)
        assert np.array_equal(c.cpu().numpy(), mc), (what, limit)
        assert np.array_equal(host(k)[w], mk[w]) and np.array_equal(host(v)[w], mv[w]), (what, limit)
        assert (host(k)[~w] == U64(SENT)).all()
    found, k, v = t.lower_bound_batch(dev(probe))
    at = np.searchsorted(model.keys, probe, side="left")
    has = at < model.keys.size
    at = np.minimum(at, model.keys.size - 1)
    assert np.array_equal(found.cpu().numpy(), has), what
    assert np.array_equal(host(k)[has], model.keys[at][has]), what
    assert np.array_equal(host(v)[has], model.vals[at][has]), what
    assert t.last_error()["bits"] == 0, (what, t.last_error())


def test_gets_without_a_directory(lib_ok, states):
    for sort_gets in (False, True):
        t, orc, info = load(states, leaf_dir=False, sort_gets=sort_gets)
        check_gets(t, orc, info, f"no directory, sort_gets {sort_gets}")
        check_scans(t, orc, info, "no directory")
        orc.close()
        t.close()


def test_gets_with_the_top_of_the_tree_in_lds(lib_ok, states):
    t, orc, info = load(states, leaf_dir=False, sort_gets=True, top_lds=True)
    check_gets(t, orc, info, "top_lds")
    orc.close()
    t.close()


def test_directory_forms_and_the_table(lib_ok, states):
    """The fingerprint directory of the first search, then a read phase: the
    pair form, the value form and the bucket table all leave torn and deleted
    keys absent and count a key with a stale copy once."""
    t, orc, info = load(states)
    # three searches: the fourth in a row starts a read phase
    probe = probes(info)
    ov, of = orc.search_batch(probe)
    gv, gf = gpu_search(t, probe)
    bad = np.nonzero((gf != of) | (gv != ov))[0]
    assert bad.size == 0, [(hex(int(probe[i])), int(gf[i]), hex(int(gv[i]))) for i in bad[:8]]
    for name in ("torn", "deleted"):
        gv, gf = gpu_search(t, info[name])
        assert not gf.any() and not gv.any(), name
        assert t.dir_stats()["form"] == "fingerprints", t.dir_stats()
    dv = t.dir_verify()
    assert dv["checked"] > 0, dv
    assert dv["bad_lists"] == dv["bad_pairs"] == dv["bad_fps"] == dv["bad_vals"] == 0, dv
    check_scans(t, orc, info, "first directory")
    for _ in range(6):
        gpu_search(t, info["keys"])
    assert t.dir_stats()["form"] == "pairs", t.dir_stats()
    assert t.vt_stats()["trusted"], t.vt_stats()
    check_gets(t, orc, info, "read phase")
    check_scans(t, orc, info, "read phase")
    dv = t.dir_verify()
    assert dv["checked"] > 0 and dv["vals_checked"] > 0, dv
    assert dv["bad_lists"] == dv["bad_pairs"] == dv["bad_fps"] == dv["bad_vals"] == 0, dv
    # the numpy reference of the directory, over the raw dumps
    bad, checked = dir_model.check_tree(t, info["keys"], info["vals"])
    assert not bad, bad[:4]
    assert checked["pair"] > 0 and checked["value"] > 0, checked
    # the table holds valid pairs only
    table, _ = t.vt_dump()
    table = table[table[:, 0] != U64(KEY_MAX)]  # a dead bucket answers nothing
    tk, tv = table[:, 0::2].ravel(), table[:, 1::2].ravel()
    held = tk[tv != 0]
    assert held.size > 0 and np.isin(held, info["keys"]).all()
    # the structural check counts value != 0: the torn entries too
    assert t.check() == {"leaves": info["leaves"], "internal": info["internal"],
                         "keys": info["n_valid"] + info["n_torn"]}
    orc.close()
    t.close()


def test_overwrites_at_version_15_wrap_to_0(lib_ok, states):
    """Every valid key of the leaves at version 15 overwritten: the entry
    bytes equal the oracle's after the same batch (f = r = 0), and nothing
    else in the image moved.  No leaf with a torn entry is written."""
    t, orc, info = load(states)
    s = info["slots"]
    k = info["v15_keys"]
    assert not np.isin(s["page"][np.isin(s["key"], k)], info["torn_pages"]).any()
    v = k ^ U64(0x7777)
    gpu_search(t, k)  # a directory for the chunk to keep
    t.insert_batch(dev(k), dev(v))
    orc.apply_batch(k, v)
    assert t.last_error()["bits"] == 0, t.last_error()
    img, root = t.dump_image()
    ref = orc.image()
    assert root == orc.root_ptr and img.size == ref.size
    diff = np.nonzero(img[ib.PAGE:] != ref[ib.PAGE:])[0]
    assert diff.size == 0, f"{diff.size} bytes differ, first at {ib.PAGE + int(diff[0])}"
    pg = img.reshape(-1, ib.PAGE)
    sel = s["kind"] == ib.VALID15
    for p, sl, key in zip(s["page"][sel], s["slot"][sel], s["key"][sel]):
        e = pg[p, ib.OFF_RECORDS + 18 * sl:][:18]
        assert e[0] & 0xF == 0 and e[17] & 0xF == 0, (p, sl, e[0], e[17])
        assert e[9:17].view("<u8")[0] == key ^ U64(0x7777)
    gv, gf = gpu_search(t, k)
    assert gf.all() and np.array_equal(gv, v)
    gv, gf = gpu_search(t, info["torn"])
    assert not gf.any()
    orc.close()
    t.close()
