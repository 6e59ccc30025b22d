"""What the GPU tests share: u64 arrays to and from the device, the device
key generator, a batched get with its outputs prefilled, and the comparison
of its results with the oracle's."""
import numpy as np
import pytest
import torch

import sherman_amd as shm

U64 = np.uint64
SENT = 0x5A5A5A5A5A5A5A5A  # prefill of the value buffers: a get that writes nothing shows


def dev(a):
    """u64 values as an int64 tensor on the GPU (a writable copy)."""
    return torch.from_numpy(np.array(a, dtype=U64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(U64)


@pytest.fixture(scope="module")
def lib_ok():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    shm.lib()
    return True


def gen_keys(t, first, n, keyspace=0):
    """key(i) = CityHash64(i) + 1 for i = first .. first + n - 1 (the
    device generator; test_device_cityhash_matches_oracle pins it)."""
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    t.gen_keys(first, n, k, keyspace=keyspace)
    torch.cuda.synchronize()
    return host(k).copy()


def _prefilled(k, prefill):
    if not prefill:
        return torch.empty_like(k), torch.empty(k.numel(), dtype=torch.uint8, device=k.device)
    return (torch.full_like(k, SENT),
            torch.full((k.numel(),), 7, dtype=torch.uint8, device=k.device))


def gpu_search(t, keys, prefill=True):
    """(vals, found) of one search_batch; the outputs start as SENT and 7."""
    k = dev(keys)
    v, f = _prefilled(k, prefill)
    t.search_batch(k, v, f)
    t.synchronize()
    return host(v), f.cpu().numpy()


def gpu_search_stats(t, keys, prefill=True):
    """gpu_search plus the walk's index statistics of that batch."""
    k = dev(keys)
    v, f = _prefilled(k, prefill)
    t.profile(False, index_stats=True)
    t.search_batch(k, v, f)
    t.synchronize()
    st = t.index_stats()
    t.profile(False)
    return host(v), f.cpu().numpy(), st


def assert_same(probe, ov, of, gv, gf, what=None):
    bad = np.nonzero((of != gf) | (ov != gv))[0]
    if bad.size:
        lines = [f"key={int(probe[i]):#x} oracle=({of[i]},{int(ov[i])}) gpu=({gf[i]},{int(gv[i])})"
                 for i in bad[:8]]
        raise AssertionError((f"{what}: " if what else "") + f"{bad.size} gets differ:\n"
                             + "\n".join(lines))
