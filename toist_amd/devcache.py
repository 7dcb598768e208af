"""Who keeps a device tensor alive for as long as a captured graph reads it: the graph's owner.  A kernel node of a hipGraph holds raw addresses,
so a tensor that a capture pass touched must outlive the graph -- whatever a process-wide cache or a scratch buffer that regrows does in the
meantime.  The launchers say keep(tensor) where they hand such a tensor out; whoever captures opens keeping() around the capture and stores the
Keep beside the graph.  The rule is written down in DESIGN.md, section 4, "What a captured graph keeps alive".  No device code here: the
predicate is a module attribute, so that tests run the bookkeeping without a device."""
import contextlib
from collections import OrderedDict

import torch

from . import staging


def _capturing():
    """staging._capturing, asked only once a GPU runtime exists: before that nothing captures, and the query itself raises without a device."""
    return torch.cuda.is_initialized() and staging._capturing()


class Keep:
    """Holds objects alive, each once (by identity)."""

    def __init__(self):
        self._held = {}

    def add(self, obj):
        self._held[id(obj)] = obj

    def __iter__(self):
        return iter(self._held.values())

    def __len__(self):
        return len(self._held)


_OPEN = []              # the Keeps of the open keeping() blocks, innermost last
FOREVER = Keep()        # what captures that nobody opened a keeping() for have read: alive as long as the process


@contextlib.contextmanager
def keeping():
    """with keeping() as kept: <capture> -- `kept` receives everything keep() is told about inside the block; store it beside the graph."""
    kept = Keep()
    _OPEN.append(kept)
    try:
        yield kept
    finally:
        _OPEN.remove(kept)


def _hold(obj):
    (_OPEN[-1] if _OPEN else FOREVER).add(obj)
    return obj


def keep(obj):
    """-> obj.  While the current stream is capturing, obj joins the innermost open Keep (FOREVER when none is open); otherwise nothing happens."""
    return _hold(obj) if _capturing() else obj


class DeviceCache:
    """key -> what make() built (device tensors, or a tuple that holds some), process-wide.  limit: at most that many entries -- going over drops
    every older entry (lru=False) or the least recently used one (lru=True).  Dropping releases the cache's own reference and nothing else: a
    graph that read the entry while it was captured holds it through its Keep."""

    def __init__(self, limit=None, lru=False):
        self.limit, self.lru, self._entries = limit, lru, OrderedDict()

    def __len__(self):
        return len(self._entries)

    def get(self, key, make, pin=None):
        """The entry of `key`, built by make() on a miss.  pin: objects that live exactly as long as the entry (those whose id() stands in the key).
        While capturing, a hit is kept for the graph; a miss runs make() inside the capture, as part of the graph, and belongs to that graph
        alone -- its contents exist only once the graph has been replayed, so it is not served to anybody else."""
        capturing = _capturing()
        ent = self._entries.get(key)
        if ent is not None:
            if self.lru:
                self._entries.move_to_end(key)
            return _hold(ent)[0] if capturing else ent[0]
        val = make()
        if capturing:
            return _hold(val)
        self._entries[key] = (val, pin)
        if self.limit is not None and len(self._entries) > self.limit:
            if self.lru:
                while len(self._entries) > self.limit:
                    self._entries.popitem(last=False)
            else:
                self._entries.clear()
                self._entries[key] = (val, pin)
        return val
