"""The core shared by the three captured steps (toist_amd/captured.py): bucket keys, the static inputs of a bucket and the upload into them, the LRU
of buckets and the rule that voids captured graphs -- all host logic, checked on CPU tensors."""
from types import SimpleNamespace

import torch


class _Stub(torch.nn.Module):
    """what CapturedEvalStep's constructor looks at: the query table (Q) and a parameter's device"""

    def __init__(self, queries=20):
        super().__init__()
        self.query_embed = torch.nn.Embedding(queries, 8)


def _core(**state):
    """The shared core alone: entries without any tensors, at most two of them."""
    from toist_amd import captured

    class Core(captured._CapturedStep):
        max_graphs = 2

        def _static_inputs(self, key):
            return dict(captured._NO_GRAPH)

    core = Core()
    core._init_capture_state(**state)
    return core


def test_bucket_of_is_the_same_for_training_and_evaluation():
    from toist_amd import captured, harness
    assert harness.CapturedTrainStep is captured.CapturedTrainStep and harness.CapturedEvalStep is captured.CapturedEvalStep
    assert harness.CapturedDistillStep is captured.CapturedDistillStep
    for pad_hw, pad_tokens, hw, tokens, want in ((64, 8, (120, 150), 10, (128, 192, 16)), (64, 1, (120, 150), 10, (128, 192, 10)),
                                                 (32, 4, (128, 129), 16, (128, 160, 16)), (1, 1, (37, 41), 5, (37, 41, 5))):
        samples, tok, _, _ = harness.synthetic_batch(2, *hw, tokens=tokens, seed=1)
        train = captured.CapturedTrainStep.bucket_of(SimpleNamespace(pad_hw=pad_hw, pad_tokens=pad_tokens), samples, tok)   # (its constructor needs a GPU)
        evalu = captured.CapturedEvalStep(_Stub(), batch=2, masks=False, pad_hw=pad_hw, pad_tokens=pad_tokens).bucket_of(samples, tok)
        assert train == evalu == want


def test_static_inputs_shapes_dtypes_and_fill_values():
    from toist_amd import captured
    for fill in (True, False):
        ent = captured.static_inputs(2, 64, 128, 8, 7, "cpu", mask_fill=fill)
        img, msk, ids, att = ent["samples"].tensors, ent["samples"].mask, ent["tok"]["input_ids"], ent["tok"]["attention_mask"]
        assert (img.shape, img.dtype) == ((2, 3, 64, 128), torch.float32) and not img.any()
        assert (msk.shape, msk.dtype) == ((2, 64, 128), torch.bool) and bool(msk.all()) == fill and bool(msk.any()) == fill
        assert (ids.shape, ids.dtype) == ((2, 8), torch.int64) and bool((ids == 7).all())
        assert (att.shape, att.dtype) == ((2, 8), torch.int64) and not att.any()
    assert bool(captured.static_inputs(1, 8, 8, 4, 1, "cpu")["samples"].mask.all())           # the bucketed steps start with everything masked as padding


def test_upload_reblanks_the_pad_region_after_a_larger_batch():
    from toist_amd import captured, harness
    ent = captured.static_inputs(2, 64, 64, 8, 1, "cpu")
    big, big_tok, _, _ = harness.synthetic_batch(2, 64, 64, tokens=8, seed=2)
    small, small_tok, _, _ = harness.synthetic_batch(2, 40, 50, tokens=6, seed=3)
    img, msk, ids, att = ent["samples"].tensors, ent["samples"].mask, ent["tok"]["input_ids"], ent["tok"]["attention_mask"]
    captured.upload(ent, big, big_tok)
    assert torch.equal(img, big.tensors) and not msk.any() and torch.equal(ids, big_tok["input_ids"]) and bool(att.all())
    captured.upload(ent, small, small_tok)
    assert torch.equal(img[:, :, :40, :50], small.tensors) and not msk[:, :40, :50].any()
    assert not img[:, :, 40:, :].any() and not img[:, :, :, 50:].any()                          # nothing of the larger batch is left
    assert bool(msk[:, 40:, :].all()) and bool(msk[:, :, 50:].all())
    assert torch.equal(ids[:, :6], small_tok["input_ids"]) and bool((ids[:, 6:] == 1).all())
    assert bool(att[:, :6].all()) and not att[:, 6:].any()
    assert ent["samples"].tensors is img and ent["tok"]["input_ids"] is ids                     # the addresses a captured graph reads stay


def test_lru_evicts_the_least_recently_used_bucket():
    core = _core()
    a, b, c = (64, 64, 8), (128, 64, 8), (64, 128, 8)
    ent_a = core._entry(a)
    core._entry(b)
    assert core._entry(a) is ent_a and list(core._buckets) == [b, a]          # a use moves the bucket to the recent end
    core._entry(c)                                                            # over max_graphs = 2: b is the least recently used
    assert list(core._buckets) == [a, c] and core._buckets[a] is ent_a
    core._entry(b)
    assert list(core._buckets) == [c, b]
    assert core._entry(a) is not ent_a and list(core._buckets) == [b, a]      # an evicted bucket starts again from fresh static inputs


def test_graphs_are_voided_once_per_flip_of_xdec_failed():
    from toist_amd import kernels
    core = _core()
    keys = [(64, 64, 8), (128, 64, 8)]

    def arm():
        for key in keys:
            core._buckets[key].update(graph=object(), loss=object(), xdec=True)

    old = kernels.XDEC_FAILED
    try:
        kernels.XDEC_FAILED = False
        for key in keys:
            core._entry(key)
        arm()
        core._entry(keys[0])
        assert all(e["graph"] is not None for e in core._buckets.values())                # no failure: the graphs stay
        kernels.XDEC_FAILED = True
        core._entry(keys[0])
        assert all(e["graph"] is None and e["loss"] is None and not e["xdec"] for e in core._buckets.values())
        arm()                                                                              # captured again, on the per-op launches
        core._entry(keys[1])
        core._void_graphs()
        assert all(e["graph"] is not None for e in core._buckets.values())                # the same flip does not void them a second time
        core._void_graphs(force=True)                                                      # (CapturedEvalStep: its own replay reported the failure)
        assert all(e["graph"] is None for e in core._buckets.values())
        # an object built after the flip (CapturedTrainStep passes the flag of its construction time) has nothing captured before it
        late = _core(xdec_seen=kernels.XDEC_FAILED)
        late._entry(keys[0]).update(graph=object())
        late._entry(keys[0])
        assert late._buckets[keys[0]]["graph"] is not None
    finally:
        kernels.XDEC_FAILED = old
