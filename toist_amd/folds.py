"""The deferred-reduction queue: fp32 partial sums wait in a per-stream arena (or a buffer of the caller's) until one batched
toist_splitk_reduce_batch launch folds them into their outputs.  The contract is written down in DESIGN.md, section 4."""
import ctypes

import torch

from . import _lib
from .devcache import keep as _keep


def _raw_stream():
    """hipStream_t of torch's current stream as an int.  torch.cuda.current_stream() builds a Stream object through three
    Python layers (~9 us): at ~1500 launches per step that alone was 13 ms of host time; the C accessor takes ~0.3 us."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _launch(descs):
    arr = (_lib.ReduceDesc * len(descs))(*descs)
    _lib.check(_lib.lib().toist_splitk_reduce_batch(ctypes.cast(arr, ctypes.c_void_p), len(descs), ctypes.c_void_p(_raw_stream())),
               "toist_splitk_reduce_batch")


class _Lane:
    """One (device, stream): the arena and its fill mark (elements), the queued (ReduceDesc, keep-alive tensors), the addresses of their outputs."""
    __slots__ = ("buf", "used", "items", "busy")

    def __init__(self):
        self.buf, self.used, self.items, self.busy = None, 0, [], set()


class FoldQueue:
    """launch(list of ReduceDesc), stream_key() and keep(arena) can be replaced so that tests run the bookkeeping without a device."""

    def __init__(self, launch=_launch, stream_key=_raw_stream, keep=_keep):
        self._launch, self._stream_key, self._keep, self._lanes = launch, stream_key, keep, {}

    def _lane(self, device):
        key = (device, self._stream_key())
        if key not in self._lanes:
            self._lanes[key] = _Lane()
        return self._lanes[key]

    def acquire(self, elems, device, outs):
        """`elems` floats of arena space for partials whose folds go into the tensors `outs`.  The only way to arena space: it flushes FIRST when
        one of `outs` has a queued fold (two folds of one output must not share a launch), so no space is handed out while a queued descriptor
        points into it."""
        lane = self._lane(device)
        if not lane.busy.isdisjoint(o.data_ptr() for o in outs):
            self.flush()
        elems = (elems + 63) // 64 * 64
        if lane.buf is None or lane.used + elems > lane.buf.numel():
            self.flush()                        # queued descriptors point into the old arena
            size = max(elems, 1 << 26 if lane.buf is None else 2 * lane.buf.numel())
            lane.buf = torch.empty(size, dtype=torch.float32, device=device)       # a graph that wrote the old arena keeps it
        lane.used += elems
        return self._keep(lane.buf)[lane.used - elems:lane.used]

    def queue(self, ws, out, splits, M, N, ldc, rscale=None, alpha=1.0, accumulate=True, keep=(), now=False, when_busy="raise"):
        """Queue out[M, N] (row stride ldc) = alpha * rscale[row] * the sum of `splits` slices [M, N] at address `ws`, in slice order (+ out when
        accumulate).  now: fold this one descriptor at once on the current stream, beside the queue.  when_busy, for callers whose `ws` is not
        from acquire() and `out` has a queued fold: "flush" the queue first, or fold this one "now"."""
        rd = _lib.ReduceDesc(ws, out.data_ptr(), None if rscale is None else rscale.data_ptr(), splits, M, N, ldc, alpha, 1 if accumulate else 0)
        lane = self._lane(out.device)
        if not now and rd.out in lane.busy:
            if when_busy not in ("flush", "now"):
                raise RuntimeError("a fold into this output is already queued")
            if when_busy == "flush":
                self.flush()
            now = when_busy == "now"
        if now:
            self._launch([rd])
        else:
            lane.items.append((rd, (out, rscale) + tuple(keep)))
            lane.busy.add(rd.out)

    def flush(self):
        """Fold everything queued on the current stream, in queue order, and reset its arenas: space acquired before is invalid from here on."""
        if not self._lanes:         # nothing was ever queued (true without a device): the stream is not asked for
            return
        stream = self._stream_key()
        for key, lane in self._lanes.items():
            if key[1] == stream:
                items, lane.items, lane.used = lane.items, [], 0
                lane.busy.clear()
                if items:
                    self._launch([rd for rd, _ in items])      # `items` keeps the tensors alive until the launch is issued


FOLDS = FoldQueue()
