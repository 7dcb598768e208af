"""A captured graph keeps alive every cached table and scratch buffer it reads (toist_amd/devcache.py): what a process-wide cache evicts, or a
scratch buffer that regrows lets go of, stays allocated for as long as the graph's Keep does.  No test here replays a graph whose tables it has
not just verified, so a wrong implementation fails an assertion instead of reading freed memory."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu


def _tensors(obj, seen=None, depth=0):
    """Every tensor reachable from obj through tuples, lists, dicts and plain attributes."""
    seen = set() if seen is None else seen
    if id(obj) in seen or depth > 6:
        return
    seen.add(id(obj))
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v, seen, depth + 1)
    elif isinstance(obj, (tuple, list)) or type(obj).__name__ == "Keep":
        for v in obj:
            yield from _tensors(v, seen, depth + 1)
    elif hasattr(obj, "__dict__") and not isinstance(obj, (torch.nn.Module, type, torch.cuda.CUDAGraph, torch.cuda.Stream)):
        yield from _tensors(vars(obj), seen, depth + 1)


def _extent(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def test_a_group_table_hit_under_capture_survives_its_eviction(dev, monkeypatch):
    from toist_amd import devcache, kernels
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf = torch.zeros(64, dtype=torch.bfloat16, device=dev)
        rows = [[buf.data_ptr() + 32 * i, buf.data_ptr() + 32 * i + 16, 16 * i, i, 0] for i in range(3)]
        want = torch.tensor([r + [0] for r in rows], dtype=torch.int64)
        table = kernels.group_table(rows, dev)                                    # outside any capture: filled and cached
        x = torch.zeros(4, device=dev)
        graph = torch.cuda.CUDAGraph()
        with devcache.keeping() as kept, torch.cuda.graph(graph, stream=side):
            hit = kernels.group_table(rows, dev)
            x.add_(1)
        assert hit is table and any(t is table for t in _tensors(kept))
        monkeypatch.setattr(kernels._GROUP_TABLES, "limit", 1)
        other = kernels.group_table([[buf.data_ptr(), buf.data_ptr() + 64, 0, 0, 0]], dev)                 # evicts the first table
        assert len(kernels._GROUP_TABLES) == 1 and kernels.group_table([[buf.data_ptr(), buf.data_ptr() + 64, 0, 0, 0]], dev) is other
        ptr, alive = table.data_ptr(), weakref.ref(table)
        del table, hit
        assert alive() is not None                                                # the Keep alone holds it now
        fresh = [torch.empty(3, 6, dtype=torch.int64, device=dev) for _ in range(64)]
        assert all(f.data_ptr() != ptr for f in fresh)
        assert alive().data_ptr() == ptr and torch.equal(alive().cpu(), want)
        graph.replay()
        assert x.tolist() == [1.0] * 4
        del kept
        gc.collect()
        assert alive() is None
    torch.cuda.current_stream().wait_stream(side)


def test_a_workspace_handed_out_under_capture_survives_the_regrow(dev):
    from toist_amd import devcache, kernels
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ws = kernels._workspace(1, dev)                                           # this stream's scratch exists before the capture
        x = torch.zeros(4, device=dev)
        graph = torch.cuda.CUDAGraph()
        with devcache.keeping() as kept, torch.cuda.graph(graph, stream=side):
            inside = kernels._workspace(1, dev)
            x.add_(1)
        assert inside is ws and [t is ws for t in kept] == [True]
        ptr, n, alive = ws.data_ptr(), ws.numel(), weakref.ref(ws)
        grown = kernels._workspace(n + 1, dev)                                    # the regrow drops the launchers' reference to the first
        assert grown.numel() > n and grown.data_ptr() != ptr and kernels._workspace(1, dev) is grown
        del ws, inside
        assert alive() is not None
        fresh = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(16)]
        assert all(f.data_ptr() != ptr for f in fresh) and alive().data_ptr() == ptr
        del kept
        gc.collect()
        assert alive() is None
    torch.cuda.current_stream().wait_stream(side)


def test_a_bucket_replays_bit_equal_after_every_cache_it_hit_was_evicted(dev, monkeypatch):
    """One CapturedTrainStep, two buckets (the model and batches of test_gpu_captured_step.py::test_captured_step_lru_evicts_the_oldest_bucket).
    Bucket A is captured and replayed; with the limit of every bounded DeviceCache at ONE entry, bucket B's eager pass then evicts everything A's
    capture hit.
    A's Keep still holds all of it, untouched and aliased by nothing of B's, and only then A is replayed from the state of its first replay: the
    same loss, bit for bit.  A third bucket pushes A out of the LRU, and its Keep goes with its graph.
    The learning rate is 0 (as in test_caption_length_is_not_padded_by_default), so the masters and the bf16 compute copies that the graphs read
    stay put through all three steps: the moments, the optimizer's state words and the seed word are what the snapshot restores."""
    import toist_amd
    from toist_amd import devcache, engine, harness, kernels
    from toist_amd.optim import FusedClipAdamWEMA
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=1, num_queries=10, dropout=0.0)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    old_reuse = engine.REUSE_GRAD_BUFFERS
    try:
        params = [p for p in model.parameters() if p.requires_grad]
        opt = FusedClipAdamWEMA([{"params": params, "lr": 0.0}], weight_decay=0.0, max_norm=0.1)
        cap = harness.CapturedTrainStep(model, criterion, opt, weight_dict, batch=1, max_targets_per_image=4, pad_hw=64, pad_tokens=8, max_graphs=2)

        def step(h, w):
            samples, tok, targets, pmap = harness.synthetic_batch(1, h, w, tokens=8, seed=h + w, max_targets=3)
            return cap.step(samples.to(dev), tok.to(dev), targets, pmap)

        state = params + opt.exp_avg + opt.exp_avg_sq + [opt.state, kernels.SEED_DEV]
        step(64, 64)                                                              # A: eagerly, then captured
        torch.cuda.synchronize()
        snapshot = [t.detach().clone() for t in state]
        recorded = step(64, 64).detach().clone()                                  # A: its first replay
        torch.cuda.synchronize()
        assert cap.captures == 1 and cap.replays == 1 and bool(torch.isfinite(recorded))
        a = cap._buckets[(64, 64, 8)]
        kept_a = list(_tensors(a["kept"]))
        small = [t for t in kept_a if t.numel() < 1 << 16]                        # the tables (the scratch buffers and the table arena are shared and rewritten)
        before = [(t.data_ptr(), _extent(t)) for t in kept_a], [t.clone() for t in small]
        tables_a = [t for t in small if t.dtype == torch.int64 and t.dim() == 2 and t.shape[1] == 6]
        assert tables_a, "A's capture hit no group table: the test does not see what it is about"

        print(f"A keeps {len(kept_a)} tensors: {len(tables_a)} group tables, {sum(t._base is None for t in tables_a)} of them cache hits")

        caches = [c for c in gc.get_objects() if type(c) is devcache.DeviceCache]
        bounded = [c for c in caches if c.limit is not None]                      # (a cache without a limit never lets go of anything)
        assert kernels._GROUP_TABLES in bounded and len(bounded) >= 6 and len(caches) >= 12
        for c in bounded:
            monkeypatch.setattr(c, "limit", 1)
        step(64, 128)                                                             # B: its eager pass evicts what A's graph hit
        torch.cuda.synchronize()
        assert cap.captures == 2 and len(kernels._GROUP_TABLES) == 1
        cached_now = {id(t) for c in caches for t in _tensors(list(c._entries.values()))}
        assert not any(id(t) in cached_now for t in tables_a)

        b = cap._buckets[(64, 128, 8)]
        own_a = {_extent(t) for t in kept_a}
        of_b = [t for t in list(_tensors(b["kept"])) + list(_tensors({k_: v for k_, v in b.items() if k_ not in ("graph", "kept")})) if t.is_cuda]
        assert [(t.data_ptr(), _extent(t)) for t in kept_a] == before[0]
        for t in of_b:                                # an allocation of B's is one A keeps too (the scratch, the arena, a cache of one key), or overlaps none of A's
            lo, hi = _extent(t)
            assert (lo, hi) in own_a or all(hi <= a_lo or a_hi <= lo for a_lo, a_hi in own_a), (t.shape, t.dtype)
        assert all(torch.equal(t, was) for t, was in zip(small, before[1]))

        with torch.no_grad():                                                     # only now: back to the state of A's first replay, and replay A
            for t, was in zip(state, snapshot):
                t.copy_(was)
        again = step(64, 64).detach().clone()
        torch.cuda.synchronize()
        assert cap.captures == 2 and cap.replays == 2
        assert torch.equal(again, recorded), (float(again), float(recorded))

        gone = weakref.ref(a["kept"])
        del a, b, kept_a, small, before, tables_a, of_b, own_a
        step(64, 128)
        step(128, 64)                                                             # a third bucket: A is the least recently used
        torch.cuda.synchronize()
        assert (64, 64, 8) not in cap._buckets and len(cap._buckets) == 2
        gc.collect()
        assert gone() is None
    finally:
        engine.REUSE_GRAD_BUFFERS = old_reuse
