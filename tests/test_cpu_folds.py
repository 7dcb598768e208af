"""The bookkeeping of the deferred-reduction queue (toist_amd/folds.py) without a device: a recording launcher, a constant stream key and
CPU tensors, of which the queue only uses the addresses."""
import itertools
import weakref
from types import SimpleNamespace

import pytest
import torch

from toist_amd.folds import FoldQueue

CPU = torch.device("cpu")
SPLITS, M, N = 3, 4, 16     # 192 floats per fold: a multiple of the arena's 64-element granule, so a take is exactly the descriptor's range


def make_queue():
    batches = []
    return FoldQueue(launch=batches.append, stream_key=lambda: 7), batches


def out_tensor():
    return torch.zeros(M * N)


def span(rd):
    return (rd.ws, rd.ws + 4 * rd.splits * rd.M * rd.N)


def overlapping(spans):
    return [(a, b) for a, b in itertools.combinations(spans, 2) if a[0] < b[1] and b[0] < a[1]]


def test_second_fold_into_a_busy_output_sends_the_first_batch_ahead():
    q, batches = make_queue()
    a, b = out_tensor(), out_tensor()
    for out in (a, b):
        q.queue(q.acquire(SPLITS * M * N, CPU, (out,)).data_ptr(), out, SPLITS, M, N, N)
    assert batches == []
    ws = q.acquire(SPLITS * M * N, CPU, (a,))       # a is busy: the batch goes out before the space is handed over
    assert [[rd.out for rd in batch] for batch in batches] == [[a.data_ptr(), b.data_ptr()]]
    q.queue(ws.data_ptr(), a, SPLITS, M, N, N)
    own = torch.zeros(SPLITS * M * N)               # a caller with partials of its own: the flushing variant
    q.queue(own.data_ptr(), a, SPLITS, M, N, N, when_busy="flush")
    assert [[rd.out for rd in batch] for batch in batches] == [[a.data_ptr(), b.data_ptr()], [a.data_ptr()]]
    q.flush()
    assert [rd.out for batch in batches for rd in batch] == [a.data_ptr(), b.data_ptr(), a.data_ptr(), a.data_ptr()]      # call order
    assert batches[2][0].ws == own.data_ptr()
    q.flush()
    assert len(batches) == 3        # nothing queued: no launch


class TakeFlushQueue:
    """The order in which kernels.wgrad3x3_small went about it before the queue became one module: take arena space (and launch the kernel into it),
    THEN flush if the output has a queued fold -- which resets the fill mark under the space just taken -- then queue."""

    def __init__(self, launch):
        self.launch, self.used, self.items = launch, 0, []

    def take_and_queue(self, out, taken):
        ws = 4096 + 4 * self.used
        self.used += SPLITS * M * N
        taken(ws)
        if any(rd.out == out for rd in self.items):
            self.launch(self.items)
            self.items, self.used = [], 0
        self.items.append(SimpleNamespace(ws=ws, out=out, splits=SPLITS, M=M, N=N))

    def flush(self):
        self.launch(self.items)


def overlaps_of_sequence(make):
    """Run A, A, B, C then a flush on make(launch) -> (step, flush).  Returns the overlaps seen at any launch among the spans whose partials were
    written and not yet folded (the batch itself, and whatever else was acquired ahead of that launch), and the batch sizes."""
    live, found, sizes = [], [], []

    def launch(batch):
        found.extend(overlapping(live))
        for rd in batch:
            live.remove(span(rd))
        sizes.append(len(batch))

    step, flush = make(launch)
    a, b, c = 1 << 20, 2 << 20, 3 << 20
    for out in (a, a, b, c):
        step(out, lambda ws: live.append((ws, ws + 4 * SPLITS * M * N)))
    flush()
    assert not live and sum(sizes) == 4
    return found, sizes


def test_space_acquired_after_a_flush_never_overlaps_a_queued_descriptor():
    def the_queue(launch):
        q, outs = FoldQueue(launch=launch, stream_key=lambda: 7), {}

        def step(out, taken):
            t = outs.setdefault(out, out_tensor())
            ws = q.acquire(SPLITS * M * N, CPU, (t,))
            taken(ws.data_ptr())
            q.queue(ws.data_ptr(), t, SPLITS, M, N, N)
        return step, q.flush

    assert overlaps_of_sequence(the_queue) == ([], [1, 3])

    # the check can fail: the take -> flush -> queue order hands C the space of A's second, still queued, fold
    def the_model(launch):
        model = TakeFlushQueue(launch)
        return model.take_and_queue, model.flush

    found, sizes = overlaps_of_sequence(the_model)
    assert len(found) == 1 and sizes == [1, 3]


def test_arena_growth_flushes_first_and_keeps_the_old_buffer_until_the_launch():
    alive = []
    batches = []
    q = FoldQueue(launch=lambda descs: (batches.append(descs), alive.append(old() is not None)), stream_key=lambda: 7)
    a, b = out_tensor(), out_tensor()
    ws = q.acquire(1 << 26, CPU, (a,))              # the whole first arena (the memory is never touched)
    old, first = weakref.ref(ws._base), ws.data_ptr()
    assert ws._base.numel() == 1 << 26
    q.queue(first, a, 1 << 10, 1 << 8, 1 << 8, 1 << 8)
    del ws
    ws = q.acquire(1, CPU, (b,))
    assert [[rd.ws for rd in batch] for batch in batches] == [[first]] and alive == [True]
    assert old() is None and ws._base.numel() == 2 << 26 and ws.numel() == 64
    own = torch.zeros(M * N)
    q.queue(own.data_ptr(), a, 1, M, N, N)          # strict: no output is busy after the flush
    q.queue(ws.data_ptr(), b, 1, 1, 64, 64)
    q.flush()
    assert [rd.out for rd in batches[1]] == [a.data_ptr(), b.data_ptr()]


@pytest.mark.parametrize("capturing", [True, False])
def test_an_arena_handed_out_under_capture_outlives_the_regrow_through_the_keep_seam(capturing):
    kept = []
    q = FoldQueue(launch=lambda descs: None, stream_key=lambda: 7, keep=lambda buf: (kept.append(buf) if capturing else None, buf)[1])
    old = weakref.ref(q.acquire(1 << 26, CPU, (out_tensor(),))._base)       # the whole first arena, handed out and let go
    assert q.acquire(1, CPU, (out_tensor(),))._base.numel() == 2 << 26      # the regrow drops the queue's reference to the first
    assert (old() is not None) == capturing and all(buf.numel() == (1 << 26) << i for i, buf in enumerate(kept))
    del kept[:]
    assert old() is None


def test_the_default_keep_seam_is_devcache_keep(monkeypatch):
    from toist_amd import devcache
    monkeypatch.setattr(devcache, "_capturing", lambda: True)
    with devcache.keeping() as kept:
        ws = FoldQueue(launch=lambda descs: None, stream_key=lambda: 7).acquire(64, CPU, (out_tensor(),))
    assert [buf.data_ptr() for buf in kept] == [ws._base.data_ptr()]


@pytest.mark.parametrize("kwargs", [dict(now=True), dict(when_busy="now")])
def test_fold_at_once_launches_one_descriptor_beside_the_queue(kwargs):
    q, batches = make_queue()
    a, b = out_tensor(), out_tensor()
    first = q.acquire(SPLITS * M * N, CPU, (a,))
    q.queue(first.data_ptr(), a, SPLITS, M, N, N)
    own = torch.zeros(SPLITS * M * N)
    target = a if "when_busy" in kwargs else b
    q.queue(own.data_ptr(), target, SPLITS, 1, M * N, M * N, alpha=0.5, accumulate=False, **kwargs)
    assert len(batches) == 1 and len(batches[0]) == 1
    rd = batches[0][0]
    assert (rd.ws, rd.out, rd.rscale, rd.splits, rd.M, rd.N, rd.ldc, rd.alpha, rd.accumulate) == (own.data_ptr(), target.data_ptr(), None, SPLITS, 1, M * N, M * N, 0.5, 0)
    assert q.acquire(64, CPU, (b,)).data_ptr() == first.data_ptr() + 4 * SPLITS * M * N       # the fill mark did not move, nothing was flushed
    assert len(batches) == 1
    q.flush()
    assert [rd.ws for rd in batches[1]] == [first.data_ptr()]


def test_strict_queue_refuses_a_busy_output():
    q, batches = make_queue()
    a = out_tensor()
    own = torch.zeros(2 * SPLITS * M * N)
    q.queue(own.data_ptr(), a, SPLITS, M, N, N)
    with pytest.raises(RuntimeError, match="already queued"):
        q.queue(own.data_ptr() + 4 * SPLITS * M * N, a, SPLITS, M, N, N)
    q.flush()
    assert [len(batch) for batch in batches] == [1]


def test_flush_without_anything_queued_needs_no_device():
    FoldQueue().flush()         # the default stream key would need a device: it is not asked
