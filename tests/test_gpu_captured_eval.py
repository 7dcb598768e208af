"""Captured evaluation on the device: the two post-processing kernels (csrc/postproc.hip: toist_postprocess; csrc/evalmask.hip:
toist_mask_resize_pack_batch) against the real reference's fixtures, and harness.CapturedEvalStep -- the evaluation body replayed from one
hipGraph per padded input shape -- against the same launches issued eagerly on the same padded inputs."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cast", ["f32", "bf16"])
def test_postprocess_kernel_vs_reference_fixture(dev, cast):
    """toist_postprocess against the REAL reference's PostProcess outputs (tests/golden/postprocess.npz) with the tolerances of
    test_gpu_coco.py::test_postprocess_values_vs_reference_fixture; with bf16-cast logits against torch's PostProcess on the same cast values."""
    from toist_amd.postprocessors import PostProcess
    d = np.load(os.path.join(GOLDEN, "postprocess.npz"))
    logits, boxes = torch.from_numpy(d["logits"]).to(dev), torch.from_numpy(d["boxes"]).to(dev)
    sizes = torch.from_numpy(d["sizes"]).to(dev)
    if cast == "bf16":
        logits = logits.to(torch.bfloat16)
        want = PostProcess()({"pred_logits": logits, "pred_boxes": boxes}, sizes)
        want_scores = [r["scores"].cpu().numpy() for r in want]
        want_boxes = [r["boxes"].cpu().numpy() for r in want]
    else:
        want_scores, want_boxes = d["scores"], d["out_boxes"]
    res = PostProcess().forward_static({"pred_logits": logits, "pred_boxes": boxes}, sizes.to(torch.int64))
    assert len(res) == logits.shape[0]
    for i, r in enumerate(res):
        assert r["scores"].is_cuda and r["scores"].dtype == torch.float32 and r["boxes"].dtype == torch.float32 and r["labels"].dtype == torch.int64
        assert tuple(r["scores"].shape) == (logits.shape[1],) and tuple(r["boxes"].shape) == (logits.shape[1], 4)
        s_err = float(np.abs(r["scores"].cpu().numpy() - want_scores[i]).max())
        b_err = float(np.abs(r["boxes"].cpu().numpy() - want_boxes[i]).max())
        print(f"postprocess[{cast}] image {i}: max |score error| {s_err:.3e}, max |box error| {b_err:.3e}")
        assert np.allclose(r["scores"].cpu().numpy(), want_scores[i], rtol=1e-5, atol=1e-6)
        assert np.array_equal(r["labels"].cpu().numpy(), d["labels"][i])
        assert np.allclose(r["boxes"].cpu().numpy(), want_boxes[i], rtol=1e-5, atol=1e-3)
        assert "scores_refexp" not in r


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_postprocess_kernel_refexp_scores_vs_torch(dev, dtype):
    """The fixture holds no pred_isfinal: scores_refexp (and a C that is not a multiple of the wave) against today's torch PostProcess.forward."""
    from toist_amd.postprocessors import PostProcess
    g = torch.Generator().manual_seed(5)
    B, Q, C = 3, 37, 101
    out = {"pred_logits": (torch.randn(B, Q, C, generator=g) * 3).to(dev).to(dtype), "pred_boxes": torch.rand(B, Q, 4, generator=g).to(dev).to(dtype),
           "pred_isfinal": torch.randn(B, Q, 1, generator=g).to(dev).to(dtype)}
    sizes = torch.tensor([[480, 640], [600, 333], [75, 1333]], device=dev)
    want = PostProcess()(out, sizes)
    got = PostProcess().forward_static(out, sizes)
    for w, r in zip(want, got):
        assert set(r) == set(w) == {"scores", "labels", "boxes", "scores_refexp"}
        for name, atol in (("scores", 1e-6), ("scores_refexp", 1e-6), ("boxes", 1e-3)):
            assert r[name].dtype == w[name].dtype and r[name].shape == w[name].shape
            assert torch.allclose(r[name], w[name], rtol=1e-5, atol=atol), (name, float((r[name] - w[name]).abs().max()))
        assert torch.equal(r["labels"], w["labels"])


def test_batched_mask_kernel_vs_reference_fixture_and_per_image_launches(dev):
    """toist_mask_resize_pack_batch on the `equal` AND the `ragged` case of tests/golden/postprocess_segm.npz in ONE launch (four images, one common
    first-resize size).  Every image's planes are bit-identical to the per-image toist_mask_resize_pack launch with the same parameters (the body is
    shared); against the real reference's masks at most 1e-4 of the pixels + 1 are flipped per image (the existing per-image bound); the words past an
    image's extent are untouched and the bits past h_i are zero."""
    from toist_amd import kernels as k
    d = np.load(os.path.join(GOLDEN, "postprocess_segm.npz"))
    pred = torch.from_numpy(d["pred_masks"]).to(dev)                         # [2, Q, 1, h0, w0]
    Bf, Q = pred.shape[:2]
    cases = ("equal", "ragged")
    mx = {c: d[c + "_max"] for c in cases}
    max_h, max_w = int(max(m[:, 0].max() for m in mx.values())), int(max(m[:, 1].max() for m in mx.values()))
    for c in cases:          # one common first-resize size serves both cases: it is each case's own batch maximum
        assert (int(mx[c][:, 0].max()), int(mx[c][:, 1].max())) == (max_h, max_w)
    src = torch.cat([pred, pred]).squeeze(2).contiguous()                    # images 0, 1 = equal; 2, 3 = ragged
    rows, want = [], []
    for c in cases:
        for i in range(Bf):
            rows.append([int(mx[c][i, 0]), int(mx[c][i, 1]), int(d[c + "_orig"][i, 0]), int(d[c + "_orig"][i, 1])])
            want.append(d[f"{c}_bits{i}"])
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    cap_hw = (130, 170)                                                      # >= the largest original (120, 161), not a multiple of 64
    cap = Q * cap_hw[1] * k.mask_words(cap_hw[0]) + 7                        # an odd slack: the image stride is the ARGUMENT, not derived from cap_hw
    SENT = -0x0123456789ABCDF
    out = torch.full((len(rows) * cap + 5,), SENT, dtype=torch.int64, device=dev)
    k.mask_resize_pack_batch(src, (max_h, max_w), table, cap_hw, cap, out)
    torch.cuda.synchronize()
    for i, (ch, cw, h, w) in enumerate(rows):
        words = Q * w * k.mask_words(h)
        got = out[i * cap:i * cap + words].view(Q, w, k.mask_words(h))
        single = k.mask_resize_pack(src[i], (max_h, max_w), (ch, cw), (h, w))
        assert torch.equal(got, single), (i, int((got != single).sum()))
        assert bool((out[i * cap + words:(i + 1) * cap] == SENT).all()), i                    # past the image's extent: untouched
        if h % 64:
            assert int((got[:, :, -1] >> (h % 64)).abs().max()) == 0, i                        # bits beyond h_i in the last word: zero
        m = k.mask_unpack(got, h, w).cpu().numpy()
        ref = np.unpackbits(want[i])[:m.size].reshape(Q, h, w).astype(bool)
        flipped = int((m != ref).sum())
        print(f"batched mask kernel, image {i} ({h} x {w}): {flipped} of {ref.size} pixels differ from the reference")
        assert flipped <= 1e-4 * ref.size + 1, (i, flipped, ref.size)
    assert bool((out[len(rows) * cap:] == SENT).all())
    # a row that does not fit the capacity writes nothing (the host check of the callers raises before the launch)
    out.fill_(SENT)
    bad = table.clone()
    bad[2, 2] = cap_hw[0] + 1
    k.mask_resize_pack_batch(src, (max_h, max_w), bad, cap_hw, cap, out)
    assert bool((out[2 * cap:3 * cap] == SENT).all()) and not bool((out[3 * cap:4 * cap] == SENT).all())
    # the wrapper: same planes as views, packed format
    from toist_amd.postprocessors import PostProcessSegm
    res = PostProcessSegm(packed=True).forward_static([{} for _ in rows], {"pred_masks": torch.cat([pred, pred])}, table, [(r[2], r[3]) for r in rows],
                                                      (max_h, max_w), cap_hw)
    for i, (ch, cw, h, w) in enumerate(rows):
        assert res[i]["mask_size"] == (h, w) and torch.equal(res[i]["mask_bits"], k.mask_resize_pack(src[i], (max_h, max_w), (ch, cw), (h, w)))
    with pytest.raises(ValueError, match="capacity"):
        PostProcessSegm(packed=True).forward_static([{} for _ in rows], {"pred_masks": torch.cat([pred, pred])}, table, [(r[2], r[3]) for r in rows],
                                                    (max_h, max_w), (100, 170))


# ---- the captured step -------------------------------------------------------------------------------------------------------------------
def _stream_of_batches():
    """(height, width, tokens) as tests/test_gpu_captured_step.py::_batches plus two: three buckets at pad_hw = 64, pad_tokens = 8.  Each image of a batch
    has its own un-padded size and its own original size (one larger, one smaller than the padded batch)."""
    from toist_amd import harness
    spec = [(128, 160, 12), (192, 128, 16), (120, 150, 10), (128, 190, 9), (180, 100, 14), (100, 130, 16), (150, 128, 11), (110, 120, 15)]
    out = []
    for i, (h, w, t) in enumerate(spec):
        samples, tok, _, _ = harness.synthetic_batch(2, h, w, tokens=t, seed=70 + i, max_targets=0)
        sizes = [(h, w), (h - 16 - i, w - 24)]
        orig = [(h + 23 + 5 * i, w + 31), (61 + 7 * i, 93 - i)]
        out.append((samples, tok, orig, sizes))
    return out


def _padded(dev, key, samples, tok):
    from toist_amd.misc import NestedTensor
    from toist_amd.transformer import TokenizedText
    Hp, Wp, Lp = key
    B, _, H, W = samples.tensors.shape
    img, msk = torch.zeros(B, 3, Hp, Wp), torch.ones(B, Hp, Wp, dtype=torch.bool)
    img[:, :, :H, :W] = samples.tensors.cpu()
    msk[:, :H, :W] = samples.mask.cpu()
    ids, att = torch.full((B, Lp), 1, dtype=torch.int64), torch.zeros(B, Lp, dtype=torch.int64)
    L = tok["input_ids"].shape[1]
    ids[:, :L] = tok["input_ids"].cpu()
    att[:, :L] = tok["attention_mask"].cpu()
    return NestedTensor(img.to(dev), msk.to(dev)), TokenizedText({"input_ids": ids.to(dev), "attention_mask": att.to(dev)})


def _eager(model, dev, key, samples, tok, orig, sizes, masks):
    """The eager forward on the padded inputs + the eager post-processors with the bucket's size as the first resize target:
    (outputs, PostProcess.forward_static results, per-image toist_mask_resize_pack planes)."""
    from toist_amd import kernels as k
    from toist_amd.postprocessors import PostProcess
    s2, t2 = _padded(dev, key, samples, tok)
    with torch.no_grad():
        mc = model(s2, t2, encode_and_save=True)
        out = model(s2, t2, encode_and_save=False, memory_cache=mc)
        res = PostProcess().forward_static(out, torch.tensor(orig, dtype=torch.int64, device=dev))
        planes = None
        if masks:
            logits = out["pred_masks"].squeeze(2).float()
            planes = [k.mask_resize_pack(logits[i], (key[0], key[1]), sizes[i], orig[i]) for i in range(len(orig))]
    return out, res, planes


def _assert_same_results(got, want_res, want_planes, tag):
    for i, r in enumerate(got):
        assert torch.equal(r["scores"], want_res[i]["scores"]), (tag, i, float((r["scores"] - want_res[i]["scores"]).abs().max()))
        assert torch.equal(r["boxes"], want_res[i]["boxes"]), (tag, i)
        assert torch.equal(r["labels"], want_res[i]["labels"])
        if want_planes is not None:
            assert r["mask_bits"].shape == want_planes[i].shape and torch.equal(r["mask_bits"], want_planes[i]), (tag, i)


def _snapshot(results):
    return [{k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in r.items()} for r in results]


def test_replay_equals_eager_on_a_mixed_stream(dev):
    """Eight batches over three buckets (mixed image sizes, caption lengths, per-image crops and original sizes) through CapturedEvalStep with a mask
    head.  Per batch, against the eager forward on the SAME padded inputs: scores / boxes bit-identical to the eagerly launched toist_postprocess,
    mask_bits bit-identical to the per-image toist_mask_resize_pack launches with the bucket's (Hp, Wp) as first resize target -- and all of it inside
    the fixture tolerances of today's torch PostProcess.forward on those outputs (rtol 1e-5; atol 1e-6 scores, 1e-3 boxes).  The eval forward holds no
    atomics (tests/test_gpu_determinism.py), so equality is exact."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=2, num_queries=20)
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    step = harness.CapturedEvalStep(model, batch=2, max_orig_hw=(256, 256), pad_hw=64, pad_tokens=8, max_graphs=4)
    assert step.masks
    stream = _stream_of_batches()
    stream = stream + stream[:3]                       # 11 steps: every bucket captured once, then replayed (also on a batch it has already seen)
    keys, seen = [], []
    for n, (samples, tok, orig, sizes) in enumerate(stream):
        key = step.bucket_of(samples, tok)
        keys.append(key)
        got = _snapshot(step.step(samples.to(dev), tok.to(dev), orig, sizes))
        out, want_res, want_planes = _eager(model, dev, key, samples, tok, orig, sizes, True)
        assert set(got[0]) == {"scores", "labels", "boxes", "mask_bits", "mask_size"}
        _assert_same_results(got, want_res, want_planes, (n, key))
        torch_res = PostProcess()(out, torch.tensor(orig, device=dev))
        for i, r in enumerate(got):
            assert r["mask_size"] == tuple(orig[i]) and r["mask_bits"].dtype == torch.int64 and r["scores"].dtype == torch.float32
            assert torch.allclose(r["scores"], torch_res[i]["scores"], rtol=1e-5, atol=1e-6)
            assert torch.allclose(r["boxes"], torch_res[i]["boxes"], rtol=1e-5, atol=1e-3)
        seen.append(torch.cat([r["scores"] for r in got]).cpu())
    buckets = set(keys)
    assert len(buckets) >= 2 and step.captures == len(buckets) and step.replays == len(stream) - len(buckets), (keys, step.captures, step.replays)
    # different batches really went through the graphs: no two of the eight distinct batches share their scores
    for a in range(8):
        for b in range(a + 1, 8):
            assert not torch.equal(seen[a], seen[b]), (a, b)
    # dense_masks: the reference's result format from the same planes
    dense = harness.CapturedEvalStep(model, batch=2, max_orig_hw=(256, 256), pad_hw=64, pad_tokens=8, dense_masks=True)
    samples, tok, orig, sizes = stream[0]
    res = dense.step(samples.to(dev), tok.to(dev), orig, sizes)
    from toist_amd import kernels as k
    for i, r in enumerate(res):
        assert "mask_bits" not in r and r["masks"].dtype == torch.bool and not r["masks"].is_cuda and tuple(r["masks"].shape) == (20, 1, *orig[i])
    _, _, planes = _eager(model, dev, keys[0], samples, tok, orig, sizes, True)
    assert torch.equal(res[1]["masks"][:, 0], k.mask_unpack(planes[1], *orig[1]).cpu())
    with pytest.raises(ValueError, match="max_orig_hw"):
        step.step(samples.to(dev), tok.to(dev), [(257, 100), orig[1]], sizes)


def test_evaluation_loop_end_to_end_through_the_captured_step(dev):
    """tests/test_gpu_coco.py::test_evaluation_loop_end_to_end rebuilt around the captured step: harness.evaluate(criterion=None, captured=step) and the
    eager harness.evaluate(criterion=None) give identical COCO summaries for boxes and masks.  The image sizes are multiples of pad_hw, so both paths
    see the same tensors."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess, PostProcessSegm
    torch.manual_seed(0)
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=20)
    model, _, _, weight_dict = toist_amd.build_model(args)
    model.to(dev)
    batches = []
    for b in range(3):
        samples, tok, targets, pmap = harness.synthetic_batch(2, 128, 192, tokens=12, seed=20 + b, device=dev, max_targets=4, with_masks=True)
        for i, t in enumerate(targets):
            t["image_id"] = torch.tensor([100 + 2 * b + i], device=dev)
            t["orig_size"], t["size"] = torch.tensor([128, 192], device=dev), torch.tensor([128, 192], device=dev)
        batches.append({"samples": samples, "tokenized": tok, "targets": targets, "positive_map": pmap})
    gt = harness.synthetic_ground_truth([b["targets"] for b in batches])
    post = {"bbox": PostProcess(), "segm": PostProcessSegm(packed=True)}
    ev = toist_amd.TDODCocoEvaluator(gt, ["bbox", "segm"], device=dev)
    eager = harness.evaluate(model, None, None, post, weight_dict, batches, [ev], dev, args)
    step = harness.CapturedEvalStep(model, batch=2, max_orig_hw=(128, 192), pad_hw=64)
    ev2 = toist_amd.TDODCocoEvaluator(gt, ["bbox", "segm"], device=dev)
    captured = harness.evaluate(model, None, None, post, weight_dict, batches, [ev2], dev, args, captured=step)
    assert sorted(ev2.img_ids) == [100, 101, 102, 103, 104, 105]
    assert step.captures == 1 and step.replays == 2
    for name in ("coco_eval_bbox", "coco_eval_masks"):
        assert len(captured[name]) == 12 and captured[name] == eager[name], (name, captured[name], eager[name])
    assert "loss" not in captured


def test_lru_evicts_the_oldest_bucket_and_recaptures(dev):
    import toist_amd
    from toist_amd import harness
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=1, num_queries=10)
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    step = harness.CapturedEvalStep(model, batch=1, pad_hw=64, pad_tokens=8, max_graphs=2)
    assert not step.masks
    for n, (h, w) in enumerate(((64, 64), (64, 128), (128, 64), (64, 64), (64, 64))):
        samples, tok, _, _ = harness.synthetic_batch(1, h, w, tokens=8, seed=h + w + n, max_targets=0)
        orig, sizes = [(h + 9, w + 3)], [(h, w)]
        got = _snapshot(step.step(samples.to(dev), tok.to(dev), orig, sizes))
        _, want, _ = _eager(model, dev, step.bucket_of(samples, tok), samples, tok, orig, sizes, False)
        _assert_same_results(got, want, None, n)
    # the third bucket evicted (64, 64, 8); its next use captured again (4 captures), the step after that replayed
    assert len(step._buckets) == 2 and (64, 64, 8) in step._buckets and (128, 64, 8) in step._buckets
    assert step.captures == 4 and step.replays == 1


def test_prototype_choice_inside_the_graph(dev):
    """cluster=True: the captured prototype choice (ClusterCriterion.infer_choice_static on the pack_eval tables) against ClusterCriterion.infer_choice on
    the same batch from the same memory state: the same rows in img_memory_mod and the same cluster_centers, to the tolerance
    tests/test_gpu_distill.py uses for the static against the list path (rtol 1e-3, atol 1e-4); the banks are filled as there."""
    import toist_amd
    from toist_amd import harness
    args = harness.default_args(device="cuda", distillation=True, cluster=True, cluster_memory_size=32, num_queries=20, enc_layers=1, dec_layers=2)
    torch.manual_seed(0)
    model, _, cc, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    cc.to(dev)
    step = harness.CapturedEvalStep(model, cc, batch=2, pad_hw=64)
    samples0, tok0, _, _ = harness.synthetic_batch(2, 128, 192, tokens=16, seed=1, max_targets=0)
    with pytest.raises(RuntimeError, match="memory bank full"):          # _static_ok's error while a bank is still filling
        step.step(samples0.to(dev), tok0.to(dev), [(128, 192)] * 2, [(128, 192)] * 2, dataset_names=["task_1_train.json"] * 2, captions=["use something"] * 2)
    cc.full_label.fill_(1)
    cc.update_count.fill_(100)
    cc.sync_host_state()
    cc_ref = copy.deepcopy(cc)
    cc_ref.sync_host_state()
    plans = [(3, 7), (2, 2), (1, 9), (11, 4), (5, 5)]
    for n, tasks in enumerate(plans):
        batch = harness.synthetic_distill_batch(2, 128, 192, tokens=16, seed=40 + n, device=dev)
        samples, tok, captions = batch["samples"][1], batch["tokenized"][1], batch["captions"][1]
        names = [f"task_{t}_train.json" for t in tasks]
        centers_before = cc.cluster_centers.clone()
        got = _snapshot(step.step(samples, tok, [(128, 192)] * 2, [(128, 192)] * 2, dataset_names=names, captions=captions))
        mod = step._buckets[(128, 192, 16)]["img_memory_mod"].clone()
        with torch.no_grad():
            mc = model(samples, tok, encode_and_save=True)
            mc = cc_ref.infer_choice(mc, names, captions)
            out = model(samples, tok, encode_and_save=False, memory_cache=mc)
        L = tok["input_ids"].shape[1]
        changed = (mod[-L:] != mc["img_memory"][-L:]).any(-1)
        assert bool(changed.any()) and torch.equal(changed, (mc["img_memory_mod"][-L:] != mc["img_memory"][-L:]).any(-1)), n      # the same rows were replaced
        assert torch.allclose(mod, mc["img_memory_mod"], rtol=1e-3, atol=1e-4), (n, float((mod - mc["img_memory_mod"]).abs().max()))
        assert torch.allclose(cc.cluster_centers, cc_ref.cluster_centers, rtol=1e-3, atol=1e-4), (n, float((cc.cluster_centers - cc_ref.cluster_centers).abs().max()))
        if n == 0:
            assert not torch.equal(cc.cluster_centers, centers_before)             # k-means moved the centres of the batch's tasks, in place
        assert all(bool(torch.isfinite(r["scores"]).all()) for r in got) and bool(torch.isfinite(out["pred_logits"]).all())
        cc_ref.cluster_centers.copy_(cc.cluster_centers)
    assert step.captures == 1 and step.replays == len(plans) - 1


def test_decoder_fallback_recaptures_on_the_per_op_path(dev):
    """The XCD-resident decoder launch inside a captured evaluation graph reports groups that were not co-resident (the project's clean-fallback test
    switch kernels.XDEC_TEST_ABSENT, armed for the captured launch only: the bounded spins expire, the launch marks its status word and ends): the step
    notices where it hands the results out, drops the graphs, runs the SAME batch again on the per-op launches and captures again.  The results equal
    the per-op eager results; later batches replay the new graph."""
    import toist_amd
    from toist_amd import harness
    from toist_amd import kernels as k
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=2, num_queries=20)
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    if not k.xdec_supported(2, 20, 4 * 6 + 12, 2):
        pytest.skip("device without 8 XCDs x 32 CUs")
    real = k.xdec_fwd

    def armed(*a, **kw):          # the eager launch is healthy; the launch recorded into the graph leaves one workgroup per XCD out
        k.XDEC_TEST_ABSENT = 1 if torch.cuda.is_current_stream_capturing() else 0
        try:
            return real(*a, **kw)
        finally:
            k.XDEC_TEST_ABSENT = 0

    batches = []
    for n in range(3):
        samples, tok, _, _ = harness.synthetic_batch(2, 128, 192, tokens=12, seed=90 + n, max_targets=0)
        batches.append((samples, tok, [(150 + n, 200), (99, 77 + n)], [(128, 192), (120, 180)]))
    try:
        k.xdec_fwd = armed
        step = harness.CapturedEvalStep(model, batch=2, pad_hw=64)
        key = step.bucket_of(*batches[0][:2])
        step.step(batches[0][0].to(dev), batches[0][1].to(dev), *batches[0][2:])
        assert step.captures == 1 and step._buckets[key]["xdec"] and not k.XDEC_FAILED
        got1 = _snapshot(step.step(batches[1][0].to(dev), batches[1][1].to(dev), *batches[1][2:]))
        assert k.XDEC_FAILED and step.captures == 2 and step.replays == 1 and not step._buckets[key]["xdec"]
        got2 = _snapshot(step.step(batches[2][0].to(dev), batches[2][1].to(dev), *batches[2][2:]))
        assert step.captures == 2 and step.replays == 2
        k.xdec_fwd = real
        for got, (samples, tok, orig, sizes) in ((got1, batches[1]), (got2, batches[2])):
            assert all(bool(torch.isfinite(r["scores"]).all()) for r in got)
            _, want, _ = _eager(model, dev, key, samples, tok, orig, sizes, False)          # (XDEC_FAILED: the eager decoder is the per-op one)
            _assert_same_results(got, want, None, "fallback")
    finally:
        k.xdec_fwd = real
        k.XDEC_TEST_ABSENT = 0
        torch.cuda.synchronize()
        k.xdec_check(raise_on_failure=False)
        k.XDEC_FAILED = False
