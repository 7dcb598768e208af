"""The bookkeeping of toist_amd/devcache.py without a device: CPU tensors as entries, the capturing predicate replaced, and a weakref to an entry
to tell whether anything still holds it."""
import weakref

import pytest
import torch

from toist_amd import devcache
from toist_amd.devcache import DeviceCache


@pytest.fixture
def capturing(monkeypatch):
    """A switch for the predicate: capturing.on = True / False.  The process-lifetime Keep is replaced by a fresh one for the test."""
    class Switch:
        on = False
    monkeypatch.setattr(devcache, "_capturing", lambda: Switch.on)
    monkeypatch.setattr(devcache, "FOREVER", devcache.Keep())
    return Switch


def entry(cache, key, refs, **kw):
    """cache.get of a fresh tensor whose weakref lands in refs[key] -> how many times make() ran."""
    made = []

    def make():
        t = torch.zeros(4)
        refs[key] = weakref.ref(t)
        made.append(1)
        return t
    cache.get(key, make, **kw)
    return len(made)


def test_entries_evicted_outside_a_capture_die(capturing):
    cache, refs = DeviceCache(limit=2), {}
    assert [entry(cache, key, refs) for key in "abc"] == [1, 1, 1]
    assert refs["a"]() is None and refs["b"]() is None and refs["c"]() is not None and len(cache) == 1      # over the limit: every older entry goes
    assert entry(cache, "c", refs) == 0 and entry(cache, "a", refs) == 1
    assert len(cache) == 2 and refs["c"]() is not None


def test_a_hit_under_capture_outlives_its_eviction_by_exactly_the_keep(capturing):
    cache, refs = DeviceCache(limit=1), {}
    entry(cache, "a", refs)
    with devcache.keeping() as kept:
        capturing.on = True
        assert entry(cache, "a", refs) == 0         # the hit
        capturing.on = False
    entry(cache, "b", refs)                         # evicts a
    assert len(cache) == 1 and refs["a"]() is not None
    assert [type(x) for x in kept] == [tuple] and next(iter(kept))[0] is refs["a"]()
    del kept
    assert refs["a"]() is None


def test_a_miss_under_capture_belongs_to_that_graph_alone(capturing):
    cache, refs = DeviceCache(), {}
    with devcache.keeping() as kept:
        capturing.on = True
        assert entry(cache, "a", refs) == 1
        capturing.on = False
    captured = refs["a"]()
    assert len(cache) == 0 and list(kept) == [captured]
    assert entry(cache, "a", refs) == 1 and refs["a"]() is not captured       # not served to an eager caller: make() runs again
    assert entry(cache, "a", refs) == 0


def test_keep_goes_to_the_innermost_open_keep_or_to_the_process(capturing):
    cache, refs = DeviceCache(), {}
    t = torch.zeros(1)
    assert devcache.keep(t) is t and len(devcache.FOREVER) == 0              # not capturing: nothing happens
    capturing.on = True
    assert devcache.keep(t) is t and devcache.keep(t) is t
    assert list(devcache.FOREVER) == [t]                                       # nobody's capture: alive with the process, once
    entry(cache, "a", refs)
    assert len(devcache.FOREVER) == 2 and refs["a"]() is not None
    with devcache.keeping() as outer:
        with devcache.keeping() as inner:
            devcache.keep(t)
        assert list(inner) == [t] and len(outer) == 0
        devcache.keep(refs["a"]())
        assert list(outer) == [refs["a"]()] and len(inner) == 1
    assert len(devcache.FOREVER) == 2


def test_lru_moves_a_hit_to_the_end_and_pins_live_with_their_entry(capturing):
    class Ref:
        pass
    cache, refs, pins = DeviceCache(limit=2, lru=True), {}, {}
    for key in "ab":
        pin = Ref()
        pins[key] = weakref.ref(pin)
        entry(cache, key, refs, pin=(pin,))
        del pin
    assert entry(cache, "a", refs) == 0             # a is the most recently used now
    entry(cache, "c", refs)
    assert refs["b"]() is None and pins["b"]() is None
    assert refs["a"]() is not None and pins["a"]() is not None and len(cache) == 2
    entry(cache, "d", refs)
    assert refs["a"]() is None and pins["a"]() is None and refs["c"]() is not None
