"""gripnet_amd._cache.VersionedCache without a GPU or the shared library: CPU tensors as keys."""
import gc
import threading
import weakref

import torch

from gripnet_amd import _cache, _hip
from gripnet_amd._cache import MISS, VersionedCache


class Value:
    """A value a weak reference can watch."""


def test_hit_on_the_same_unmodified_object_only():
    cache = VersionedCache(4)
    t = torch.arange(6)
    v = Value()
    assert cache.get(t, 3) is MISS
    assert cache.put(t, v, 3) is v
    assert cache.get(t, 3) is v
    assert cache.get(t, 4) is MISS                             # different extra
    assert cache.get(t) is MISS
    assert cache.get(t.clone(), 3) is MISS                     # equal, but another tensor
    assert cache.get(t.view(-1), 3) is MISS                    # the same storage, another object
    assert cache.get(t, 3) is v
    t[0] = 7                                                   # an in-place write moves _version
    assert cache.get(t, 3) is MISS
    w = Value()
    cache.put(t, w, 3)                                         # ... and the new value takes the old one's place
    assert cache.get(t, 3) is w
    assert len(cache._entries) == 1


def test_extras_of_one_object_are_entries_of_their_own():
    cache = VersionedCache(4)
    t = torch.zeros(2)
    cache.put(t, "cpu", torch.device("cpu"))
    cache.put(t, "blocks", ((0, 2), (2, 5)), 9)
    assert cache.get(t, torch.device("cpu")) == "cpu"
    assert cache.get(t, ((0, 2), (2, 5)), 9) == "blocks"
    assert cache.get(t, ((0, 2), (2, 5)), 8) is MISS


def test_a_cached_none_is_a_hit():
    cache = VersionedCache(4)
    t = torch.zeros(3)
    assert cache.get(t) is MISS
    assert cache.put(t, None) is None
    assert cache.get(t) is None
    cache.put(t, 5)                                            # (node_gather_plan: the plan arrives at a later sighting)
    assert cache.get(t) == 5
    cache.clear()
    assert cache.get(t) is MISS


def test_depth_drops_the_least_recently_used():
    cache = VersionedCache(3)
    a, b, c, d = (torch.zeros(1) for _ in range(4))
    for i, t in enumerate((a, b, c)):
        cache.put(t, i)
    assert cache.get(a) == 0                                   # a hit moves to the front: b is the oldest now
    cache.put(d, 3)
    assert cache.get(b) is MISS
    assert (cache.get(a), cache.get(c), cache.get(d)) == (0, 2, 3)
    assert len(cache._entries) == 3


def test_a_key_that_is_gone_takes_its_value_with_it():
    """What the module-global lists of the tensors themselves did not do: a caller that drops its tensor frees what was
    derived from it (on the GPU: the derived device arrays), without four other tensors having to push it out."""
    cache = VersionedCache(4)
    t, other = torch.zeros(3), torch.zeros(3)
    v = Value()
    seen = weakref.ref(v)
    cache.put(t, v)
    cache.put(other, 1)
    del v
    gc.collect()
    assert seen() is not None                                  # the cache holds the value ...
    del t
    gc.collect()
    assert cache.get(other) == 1                               # (any access sweeps)
    assert seen() is None                                      # ... while its key lives
    assert len(cache._entries) == 1


def test_objects_without_a_version_are_never_stored():
    cache = VersionedCache(4)
    ranges = [[0, 2], [2, 5]]
    assert cache.put(ranges, "plan") == "plan"
    assert cache.get(ranges) is MISS

    class Plain:                                               # weakly referable, but nothing says when it was written
        pass
    p = Plain()
    cache.put(p, "plan")
    assert cache.get(p) is MISS
    assert cache._entries == []


def test_eight_threads():
    cache = VersionedCache(4)
    keys = [torch.zeros(1) for _ in range(12)]
    errors = []

    def work(seed):
        try:
            for i in range(2000):
                k = (seed * 7 + i * 5) % len(keys)
                got = cache.get(keys[k], k % 2)
                assert got is MISS or got == k
                if got is MISS or i % 3 == 0:
                    cache.put(keys[k], k, k % 2)
                if i % 500 == 499:
                    keys[k].add_(1)                            # a version moves under the others' feet
        except BaseException as err:                           # noqa: BLE001 (reported by the main thread)
            errors.append(err)

    threads = [threading.Thread(target=work, args=(s,)) for s in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []
    assert len(cache._entries) <= 4
    assert sum(cache.get(t, k % 2) is not MISS for k, t in enumerate(keys)) <= 4


def test_the_cache_module_stands_alone():
    assert not any(name in vars(_cache) for name in ("_hip", "torch"))


def test_an_int16_edge_type_is_not_its_own_cache_entry():
    """`et.to(torch.int16)` of an int16 tensor is the tensor itself: stored, the value would keep its key alive for ever."""
    et16 = torch.tensor([0, 0, 1], dtype=torch.int16)
    assert _hip.relation_ids16(et16) is et16
    seen = weakref.ref(et16)
    del et16
    gc.collect()
    assert seen() is None
    et = torch.tensor([0, 0, 1])
    r16 = _hip.relation_ids16(et)
    assert r16.dtype == torch.int16 and _hip.relation_ids16(et) is r16
    seen = weakref.ref(r16)
    del et, r16
    gc.collect()
    _hip.relation_ids16(torch.tensor([2]))
    assert seen() is None
