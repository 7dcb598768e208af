"""CapturedSweepStep: the task sweep replayed from hipGraphs against the eager sweep on the same padded inputs (bit for bit), changing pair tables
under one graph, padded pairs, the device guard of the tables behind a capture, and the LRU of buckets.
(The file sorts behind every other GPU test file on purpose: DESIGN 8 item 6.  No training step is built here.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(dev, **over):
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cuda", **{**dict(enc_layers=1, dec_layers=2, num_queries=20), **over}))[0]
    return model.to(dev).eval()


def _padded(dev, key, samples, tok):
    from toist_amd.misc import NestedTensor
    from toist_amd.transformer import TokenizedText
    Hp, Wp, Lp = key
    B, _, H, W = samples.tensors.shape
    img, msk = torch.zeros(B, 3, Hp, Wp), torch.ones(B, Hp, Wp, dtype=torch.bool)
    img[:, :, :H, :W] = samples.tensors.cpu()
    msk[:, :H, :W] = samples.mask.cpu()
    T, L = tok["input_ids"].shape
    ids, att = torch.full((T, Lp), 1, dtype=torch.int64), torch.zeros(T, Lp, dtype=torch.int64)
    ids[:, :L] = tok["input_ids"].cpu()
    att[:, :L] = tok["attention_mask"].cpu()
    return NestedTensor(img.to(dev), msk.to(dev)), TokenizedText({"input_ids": ids.to(dev), "attention_mask": att.to(dev)})


def _eager(model, dev, key, samples, tok, orig, pairs, capacity):
    """The eager sweep on the SAME padded inputs and the SAME padded tables, through the eagerly launched toist_postprocess."""
    from toist_amd.postprocessors import PostProcess
    from toist_amd.sweep import pair_tables
    s2, t2 = _padded(dev, key, samples, tok)
    pi, pc, live = pair_tables(samples.tensors.shape[0], tok["input_ids"].shape[0], pairs, capacity=capacity)
    with torch.no_grad():
        state, text = model.sweep_stages(s2, t2)
        out = model.decode(model.sweep_pairs(state, text, pi, pc))
        res = PostProcess().forward_static(out, torch.tensor([orig[i] for i in pi.tolist()], dtype=torch.int64, device=dev))
    return res[:live], pi, pc, live


def _snapshot(results):
    return [{k_: v.clone() for k_, v in r.items()} for r in results]


def _same(got, want, note):
    assert len(got) == len(want), note
    for p, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) == {"scores", "labels", "boxes"}, note
        for k_ in g:
            assert g[k_].dtype == w[k_].dtype and torch.equal(g[k_], w[k_]), (note, p, k_)


def _inputs(n_images, n_captions, h, w, tokens, seed):
    from toist_amd import harness
    samples, _, _, _ = harness.synthetic_batch(n_images, h, w, tokens=tokens, seed=seed, max_targets=0)
    _, tok, _, _ = harness.synthetic_batch(n_captions, 32, 32, tokens=tokens, seed=seed + 100, max_targets=0)
    return samples, tok


def test_replay_equals_eager_with_changing_pair_tables(dev):
    """Three batches through ONE graph (bucket 128 x 192 x 16): two image sizes, three different pair tables (the full product, a short list with a
    repeat, another short list).  Each equals the eager sweep on the same padded inputs bit for bit; rows behind `live` are never handed out."""
    from toist_amd import harness, sweep
    model = _model(dev)
    step = harness.CapturedSweepStep(model, batch=2, captions=3, pad_hw=64)
    assert step.pairs == 6
    stream = [((128, 160), None, [(131, 170), (64, 99)]), ((120, 150), [(1, 2), (0, 0), (1, 2), (0, 1)], [(300, 200), (120, 150)]),
              ((128, 160), [(0, 2), (1, 1)], [(128, 160), (256, 320)])]
    for n, ((h, w), pairs, orig) in enumerate(stream):
        samples, tok = _inputs(2, 3, h, w, 16, 20 + n)
        results, pi, pc, live = step.step(samples.to(dev), tok.to(dev), orig, pairs=pairs)
        got = _snapshot(results)
        assert step.bucket_of(samples, tok) == (128, 192, 16)
        want, wi, wc, wlive = _eager(model, dev, (128, 192, 16), samples, tok, orig, pairs, 6)
        assert live == wlive == (6 if pairs is None else len(pairs)) and len(got) == live                  # padded pairs never appear
        assert pi.numel() == 6 and torch.equal(pi, wi) and torch.equal(pc, wc)
        _same(got, want, n)
        keyed = sweep.keyed_results(results, [10, 11], ["a", "b", "c"], pi, pc, live)
        assert sorted(keyed) == sorted({(10 + i, "abc"[t]) for i, t in (pairs or [(i, t) for i in range(2) for t in range(3)])})
    assert step.captures == 1 and step.replays == 2
    # the loop on top of it: the same keys and values as the eager loop
    tasks = [("a", "x"), ("b", "y"), ("c", "z")]
    samples, tok = _inputs(2, 3, 128, 160, 16, 31)
    batch = {"samples": samples.to(dev), "image_ids": [10, 11], "orig_sizes": [(131, 170), (64, 99)]}
    from toist_amd.postprocessors import PostProcess
    cap = {k_: _snapshot([v])[0] for k_, v in harness.evaluate_sweep(model, PostProcess(), [batch], tasks, dev, captured=step, tokenized=tok.to(dev)).items()}
    assert step.replays == 3 and len(cap) == 6
    with pytest.raises(ValueError, match="cluster criterion"):
        harness.evaluate_sweep(model, PostProcess(), [batch], [t + ("task_1_train.json",) for t in tasks], dev, cluster_criterion=torch.nn.Module(), captured=step)


def test_a_table_corrupted_behind_the_capture_raises_through_the_status_word(dev):
    """The graph's assemble launch reads the tables at replay time.  An entry rewritten on the device after the capture (here: image 2 of 2) is never
    used as an index: the next step raises ValueError from the status word, and the step after it -- tables uploaded afresh -- is right again."""
    from toist_amd import harness, kernels
    model = _model(dev)
    step = harness.CapturedSweepStep(model, batch=2, captions=2, pairs=5, pad_hw=64)
    samples, tok = _inputs(2, 2, 64, 64, 8, 3)
    orig = [(70, 80), (90, 100)]
    pairs = [(0, 1), (1, 0), (1, 1)]
    first = _snapshot(step.step(samples.to(dev), tok.to(dev), orig, pairs=pairs)[0])                        # eager + capture
    again = _snapshot(step.step(samples.to(dev), tok.to(dev), orig, pairs=pairs)[0])                        # replay
    _same(again, first, "replay")
    ent = step._buckets[(64, 64, 8)]
    assert ent["graph"] is not None and ent["pair_image"].tolist() == [0, 1, 1, 0, 0]
    ent["pair_image"][1] = 2
    with pytest.raises(ValueError, match="pair 1"):
        step.step(samples.to(dev), tok.to(dev), orig, pairs=pairs)
    assert int(kernels.sweep_status(dev).item()) == 0                                                        # read and cleared
    after = _snapshot(step.step(samples.to(dev), tok.to(dev), orig, pairs=pairs)[0])
    assert ent["pair_image"].tolist() == [0, 1, 1, 0, 0]
    _same(after, first, "after the refusal")
    assert step.captures == 1 and step.replays == 3
    with pytest.raises(ValueError):
        step.step(samples.to(dev), tok.to(dev), orig, pairs=pairs + [(0, 0)] * 3)                           # 6 pairs, capacity 5
    with pytest.raises(ValueError):
        step.step(samples.to(dev), tok.to(dev), orig, pairs=[(2, 0)])                                       # refused on the host: nothing launched
    with pytest.raises(ValueError):
        step.step(samples.to(dev), tok.to(dev), orig[:1])
    assert step.replays == 3


def test_lru_evicts_the_oldest_bucket_and_recaptures(dev):
    from toist_amd import harness
    model = _model(dev, dec_layers=1, num_queries=10)
    step = harness.CapturedSweepStep(model, batch=1, captions=2, pad_hw=64, pad_tokens=8, max_graphs=2)
    for n, (h, w) in enumerate(((64, 64), (64, 128), (128, 64), (64, 64), (64, 64))):
        samples, tok = _inputs(1, 2, h, w, 8, h + w + n)
        orig = [(h + 9, w + 3)]
        got = _snapshot(step.step(samples.to(dev), tok.to(dev), orig)[0])
        want, _, _, _ = _eager(model, dev, step.bucket_of(samples, tok), samples, tok, orig, None, 2)
        _same(got, want, n)
    # the third bucket evicted (64, 64, 8); its next use captured again (4 captures), the step after that replayed
    assert len(step._buckets) == 2 and (64, 64, 8) in step._buckets and (128, 64, 8) in step._buckets
    assert step.captures == 4 and step.replays == 1


def test_what_the_captured_sweep_refuses(dev):
    import toist_amd
    from toist_amd import harness
    model = _model(dev, dec_layers=1, num_queries=10)
    with pytest.raises(ValueError, match="cluster criterion"):
        harness.CapturedSweepStep(model, torch.nn.Module(), batch=1, captions=2)
    with pytest.raises(ValueError):
        harness.CapturedSweepStep(model, batch=0, captions=2)
    segm = toist_amd.build_model(harness.default_args(device="cpu", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=4))[0]
    with pytest.raises(NotImplementedError, match="DETRsegm sweeps"):
        harness.CapturedSweepStep(segm, batch=1, captions=2, device=dev)
    step = harness.CapturedSweepStep(model, batch=1, captions=2)
    samples, tok = _inputs(1, 3, 64, 64, 8, 1)
    with pytest.raises(ValueError, match="captions"):
        step.step(samples.to(dev), tok.to(dev), [(64, 64)])                                                 # 3 captions, built for 2
    assert step.captures == 0
