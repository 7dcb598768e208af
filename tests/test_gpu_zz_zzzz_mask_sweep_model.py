"""The task sweep with the mask head on a tiny DETRsegm (one encoder layer, one decoder layer, four queries): encode_mask_sweep / decode_mask_sweep
against the per-pair path they replace (identity for the pairing (i, i); equal maps whatever the pass size; no further from the existing forward on
the expanded batch than that forward is from the fp32 oracle), CapturedMaskSweepStep against the eager sweep on the same padded inputs, and
harness.evaluate_sweep scored by SweepEvaluator(iou_types=("bbox", "segm")) against per-task evaluators fed by update().
(The file builds captured steps, so it sorts behind every older GPU test file: DESIGN 8 item 6.)"""
import numpy as np
import pytest
import torch

import rounding_bounds as rb

pytestmark = pytest.mark.gpu
FILE = "mask_sweep_model_parity.json"
PAIRS = [(1, 0), (0, 2), (1, 0), (0, 1), (1, 2)]                # a repeat, non-monotone, every image and every caption


def rel_err(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).norm() / (b.detach().float().cpu().norm() + 1e-12))


@pytest.fixture(scope="module")
def setup(dev):
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=4)
    model = toist_amd.build_model(args)[0]
    assert type(model).__name__ == "DETRsegm"
    for n, b in model.named_buffers():
        if n.endswith("bn3.weight"):
            b.mul_(0.3)                                       # 33 residual blocks keep the activations in range (tests/test_gpu_model.py)
    sd = {k_: v.detach().clone().float() for k_, v in model.state_dict().items()}
    return model.to(dev).eval(), sd


def _inputs(n_images, n_captions, h, w, tokens, seed):
    from toist_amd import harness
    samples, _, _, _ = harness.synthetic_batch(n_images, h, w, tokens=tokens, seed=seed, max_targets=0)
    _, tok, _, _ = harness.synthetic_batch(n_captions, 32, 32, tokens=tokens, seed=seed + 100, max_targets=0)
    return samples, tok


def _expanded(samples, tok, pairs):
    """the per-pair path's batch: row p = (image pairs[p][0], caption pairs[p][1])"""
    from toist_amd.misc import NestedTensor
    from toist_amd.transformer import TokenizedText
    pi = torch.tensor([p[0] for p in pairs], device=samples.tensors.device)
    pc = torch.tensor([p[1] for p in pairs], device=tok["input_ids"].device)
    return (NestedTensor(samples.tensors[pi].contiguous(), samples.mask[pi].contiguous()),
            TokenizedText({"input_ids": tok["input_ids"][pc].contiguous(), "attention_mask": tok["attention_mask"][pc].contiguous()}))


def _forward(model, samples, tok):
    mc = model(samples, tok, encode_and_save=True)
    return model(samples, tok, encode_and_save=False, memory_cache=mc)


def _sweep(model, samples, tok, pairs, pairs_per_pass=8):
    from toist_amd import kernels
    out = model.decode_mask_sweep(model.encode_mask_sweep(samples, tok, pairs), pairs_per_pass)
    assert kernels.sweep_check(raise_on_failure=False) == 0
    kernels.xdec_check()
    return out


# ------------------------------------------------------------------------------------------------------------------ identity
@torch.no_grad()
def test_the_pairing_i_i_is_the_ordinary_forward(dev, setup):
    """64 x 64: every map is one strip per stage, so no atomic order is free -- and the per-image terms run at the shapes of the ordinary forward"""
    model, _ = setup
    samples, tok = _inputs(2, 2, 64, 64, 8, 21)
    samples, tok = samples.to(dev), tok.to(dev)
    want = _forward(model, samples, tok)
    got = _sweep(model, samples, tok, [(0, 0), (1, 1)])
    assert got["pred_masks"].shape == want["pred_masks"].shape == (2, 4, 16, 16) and got["pred_masks"].dtype == torch.float32
    for name in ("pred_masks", "pred_logits", "pred_boxes"):
        assert torch.equal(got[name], want[name]), name
    assert float(got["pred_masks"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ pass invariance
@torch.no_grad()
def test_the_pass_size_does_not_change_a_map(dev, setup):
    model, _ = setup
    samples, tok = _inputs(2, 3, 64, 64, 8, 22)
    samples, tok = samples.to(dev), tok.to(dev)
    outs = {n: _sweep(model, samples, tok, PAIRS, n)["pred_masks"] for n in (1, 2, 5)}
    assert outs[5].shape == (5, 4, 16, 16)
    assert torch.equal(outs[1], outs[5]) and torch.equal(outs[2], outs[5])
    assert torch.equal(outs[2][0], outs[2][2])                # the pair listed twice, in different passes
    assert not torch.equal(outs[2][0], outs[2][1])
    with pytest.raises(ValueError):
        model.decode_mask_sweep(model.encode_mask_sweep(samples, tok, PAIRS), 0)


# ------------------------------------------------------------------------------------------------------------------ the existing path and the oracle
@pytest.mark.parametrize("hw", [(64, 64), (128, 160), (104, 136)], ids=lambda v: "x".join(map(str, v)))
@torch.no_grad()
def test_against_the_existing_forward_and_the_oracle(dev, setup, hw):
    """E = the existing forward on the expanded batch against the fp32 oracle, S = the sweep against it: S < 6e-2 (the bound of
    test_gpu_model.py::test_segmentation_model_end_to_end) and the sweep is no further from the existing forward than that is from fp32.
    (104, 136): levels that are not doublings of each other -- the per-op path through resize_add_pairs."""
    from oracle import model_ref
    model, sd = setup
    samples, tok = _inputs(2, 3, hw[0], hw[1], 8, 23)
    pi, pc = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    # the oracle: the ResNet once per image, everything else on the expanded batch
    dsd = {k_[5:]: v for k_, v in sd.items() if k_.startswith("detr.")}
    feats = [f[pi] for f in model_ref.resnet_body(samples.tensors, dsd, "backbone.0.body.")]
    rmc = model_ref.mdetr_encode(dsd, samples.tensors[pi], samples.mask[pi], tok["input_ids"][pc], tok["attention_mask"][pc], features=feats[-1])
    rout = model_ref.mdetr_decode(dsd, rmc)
    src_proj = torch.nn.functional.conv2d(feats[-1], dsd["input_proj.weight"], dsd["input_proj.bias"])
    fmask = model_ref.downsample_mask(samples.mask[pi], feats[-1].shape[-2:])
    ref = model_ref.segm_decode(sd, rmc, rout, feats, src_proj, fmask, prefix="detr.")
    samples, tok = samples.to(dev), tok.to(dev)
    old = _forward(model, *_expanded(samples, tok, PAIRS))["pred_masks"]
    new = _sweep(model, samples, tok, PAIRS, 2)["pred_masks"]
    up = lambda v, s_: (v + s_ - 1) // s_
    assert new.shape == old.shape == (5, 4, up(hw[0], 4), up(hw[1], 4))
    E, S, D = rel_err(old, ref), rel_err(new, ref), rel_err(new, old)
    print(f"mask sweep {hw}: existing vs oracle {E:.3e}, sweep vs oracle {S:.3e}, sweep vs existing {D:.3e}")
    rb.record("mask_sweep.pred_masks", f"{hw[0]}x{hw[1]}", S / 6e-2, file=FILE,
              extra={"existing_vs_oracle": E, "sweep_vs_oracle": S, "sweep_vs_existing": D, "bound": 6e-2})
    assert S < 6e-2, (hw, S)
    assert D <= E, (hw, D, E)


# ------------------------------------------------------------------------------------------------------------------ captured
ORIG, CROP = [(90, 80), (96, 96)], [(64, 60), (50, 64)]


@torch.no_grad()
def _eager_step(model, samples, tok, pairs, capacity, pairs_per_pass):
    """the eager sweep + kernels.postprocess + per-pair mask_resize_pack on the table padded with (0, 0) to the capacity"""
    from toist_amd import kernels as k
    padded = list(pairs) + [(0, 0)] * (capacity - len(pairs))
    out = _sweep(model, samples, tok, padded, pairs_per_pass)
    sizes = torch.tensor([ORIG[i] for i, _ in padded], dtype=torch.int64, device=samples.tensors.device)
    post = k.postprocess(out["pred_logits"], out["pred_boxes"], sizes)
    bits = [k.mask_resize_pack(out["pred_masks"][p], tuple(samples.tensors.shape[-2:]), CROP[i], ORIG[i]) for p, (i, _) in enumerate(padded)]
    return post, bits


def test_captured_step_equals_the_eager_sweep(dev, setup):
    from toist_amd import harness
    model, _ = setup
    step = harness.CapturedMaskSweepStep(model, batch=2, captions=3, pairs=6, max_orig_hw=(96, 96), pad_hw=64, pairs_per_pass=4)
    _, tok = _inputs(2, 3, 64, 64, 8, 30)
    tok = tok.to(dev)
    full, short = None, [(1, 2), (0, 0), (1, 0), (0, 1)]       # every caption on every image; four pairs + two padding rows
    for n, pairs in enumerate((full, short, full, short, short)):
        samples, _ = _inputs(2, 3, 64, 64, 8, 31 + n)
        samples = samples.to(dev)
        results, pi, pc, live = step.step(samples, tok, ORIG, CROP, pairs=pairs)
        listed = [(i, t) for i in range(2) for t in range(3)] if pairs is None else pairs
        assert live == len(listed) == len(results) and pi.numel() == pc.numel() == 6               # rows from `live` on are never handed out
        assert list(zip(pi.tolist(), pc.tolist()))[:live] == listed and pi.tolist()[live:] == [0] * (6 - live)
        got = [{k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in r.items()} for r in results]
        post, bits = _eager_step(model, samples, tok, listed, 6, 4)
        for p, r in enumerate(got):
            i = listed[p][0]
            assert set(r) == {"scores", "labels", "boxes", "mask_bits", "mask_size"}
            assert r["mask_size"] == ORIG[i] and tuple(r["mask_bits"].shape) == (4, ORIG[i][1], (ORIG[i][0] + 63) // 64) and r["mask_bits"].dtype == torch.int64
            assert torch.equal(r["scores"], post["scores"][p]) and torch.equal(r["boxes"], post["boxes"][p]), (n, p)
            assert torch.equal(r["mask_bits"], bits[p]), (n, p)
        assert (step.captures, step.replays) == (1, n)                                              # one capture per bucket, replays otherwise
        assert any(bool(r["mask_bits"].any()) for r in got) and not all(bool((r["mask_bits"] == -1).all()) for r in got)
    # step_rows: the same rows, the planes as a RowMasks over the bucket
    out, masks, pi, pc, live = step.step_rows(samples, tok, ORIG, CROP, pairs=short)
    assert live == 4 and tuple(out["scores"].shape) == (6, 4) and masks.capacity_words == step.capacity_words and masks.hw_host[:4] == [ORIG[i] for i, _ in short]
    assert torch.equal(out["scores"][:4], torch.stack([r["scores"] for r in got]))
    assert torch.equal(masks.hw_dev.cpu(), torch.tensor([ORIG[i] for i in pi.tolist()]))
    # refused before any launch
    before = (step.captures, step.replays)
    with pytest.raises(ValueError, match="capacity"):
        step.step(samples, tok, ORIG, CROP, pairs=[(0, 0)] * 7)
    with pytest.raises(ValueError, match="max_orig_hw"):
        step.step(samples, tok, [(97, 80), (96, 96)], CROP)
    with pytest.raises(ValueError, match="does not fit"):
        step.step(samples, tok, ORIG, [(65, 60), (50, 64)])
    with pytest.raises(ValueError):
        step.step(samples, tok, ORIG, CROP, pairs=[(2, 0)])
    assert (step.captures, step.replays) == before


# ------------------------------------------------------------------------------------------------------------------ the loop and the scoring
def _ground_truth_from(keyed, names, image_ids, sizes):
    """Per task a ground truth cut from the model's own detections: the two best boxes of every (image, task) with the masks the model predicted for
    them (a rectangle where it predicted none), the second one shifted; task 0 does not know the last image, task 1 has no annotation on the first."""
    from toist_amd import kernels as k
    data = {}
    for t, name in enumerate(names):
        known = image_ids[:-1] if t == 0 else image_ids
        anns = []
        for img in known:
            if t == 1 and img == image_ids[0]:
                continue
            r = keyed[(img, name)]
            h, w = r["mask_size"]
            dense = k.mask_unpack(r["mask_bits"], h, w).cpu().numpy()
            top = torch.sort(r["scores"].double(), descending=True, stable=True).indices[:2].tolist()
            for j, q in enumerate(top):
                x0, y0, x1, y1 = (float(v) for v in r["boxes"][q])
                bw, bh = max(x1 - x0, 1.0), max(y1 - y0, 1.0)
                m = dense[q].copy()
                if not m.any():
                    m[h // 4:h // 2, w // 4:w // 2] = True
                if j:
                    m = np.roll(m, 3, axis=1)
                anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "iscrowd": 0, "bbox": [x0 + 3.0 * j, y0, bw, bh], "area": bw * bh,
                             "segmentation": m})
        data[name] = {"images": [{"id": i, "height": sizes[i][0], "width": sizes[i][1]} for i in known], "annotations": anns}
    return data


def _control(per_batch_keyed, data, names, dev):
    from toist_amd import coco_eval as C
    evs = {n: C.TDODCocoEvaluator(data[n], ["bbox", "segm"], device=dev) for n in names}
    for keyed in per_batch_keyed:
        for n in names:
            evs[n].update({img: {k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in r.items()} for (img, name), r in keyed.items() if name == n})
    stats = {}
    for n, ev in evs.items():
        ev.synchronize_between_processes()
        ev.accumulate()
        ev.summarize(verbose=False)
        stats[n] = {t: ev.coco_eval[t].stats for t in ("bbox", "segm")}
    return evs, stats


def _same_records(got, want, note):
    assert sorted(got, key=str) == sorted(want, key=str), note
    for img in want:
        g, w = got[img], want[img]
        assert list(g) == list(w) and g["image_id"] == w["image_id"], (note, img)
        for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
            assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape and g[key].tobytes() == w[key].tobytes(), (note, img, key)


def _same_as_control(sw, got, evs, stats, names, note):
    assert set(got) == {"tasks", "mAP50", "mAP", "segm"} and set(got["segm"]) == {"tasks", "mAP50", "mAP"}
    for n in names:
        assert sw.evaluators[n].img_ids == evs[n].img_ids, (note, n)
        for t, numbers in (("bbox", got), ("segm", got["segm"])):
            _same_records(sw.evaluators[n].coco_eval[t].records, evs[n].coco_eval[t].records, (note, n, t))
            assert np.array_equal(numbers["tasks"][n], stats[n][t]) and len(numbers["tasks"][n]) == 12, (note, n, t)
    for t, numbers in (("bbox", got), ("segm", got["segm"])):
        assert numbers["mAP50"] == float(np.mean([stats[n][t][1] for n in names])) and numbers["mAP"] == float(np.mean([stats[n][t][0] for n in names])), (note, t)


def _clone_keyed(keyed):
    return {key: {k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in r.items()} for key, r in keyed.items()}


def test_scored_mask_sweep_equals_per_task_update_captured_and_eager(dev, setup):
    from toist_amd import coco_eval as C, harness, sweep
    from toist_amd.postprocessors import PostProcess
    model, _ = setup
    names, tasks = ["a", "b", "c"], [("a", "x"), ("b", "y"), ("c", "z")]
    _, tok = _inputs(2, 3, 64, 64, 8, 40)
    tok = tok.to(dev)
    batches, sizes = [], {}
    for n, ids in enumerate(([10, 11], [12, 13])):
        samples, _ = _inputs(2, 3, 64, 64, 8, 41 + n)
        batches.append({"samples": samples.to(dev), "image_ids": ids, "orig_sizes": ORIG, "sizes": CROP})
        sizes.update(zip(ids, ORIG))
    image_ids = [10, 11, 12, 13]
    # captured
    step = harness.CapturedMaskSweepStep(model, batch=2, captions=3, max_orig_hw=(96, 96), pad_hw=64, pairs_per_pass=4)
    per_batch = []
    for b in batches:
        results, pi, pc, live = step.step(b["samples"], tok, b["orig_sizes"], b["sizes"])
        per_batch.append(_clone_keyed(sweep.keyed_results(results, b["image_ids"], names, pi, pc, live)))
    data = _ground_truth_from({**per_batch[0], **per_batch[1]}, names, image_ids, sizes)
    evs, stats = _control(per_batch, data, names, dev)
    sw = C.SweepEvaluator(data, dev, iou_types=("bbox", "segm"))
    replays = step.replays
    got = harness.evaluate_sweep(model, PostProcess(), batches, tasks, dev, captured=step, tokenized=tok, evaluator=sw)
    assert step.replays == replays + 2 and step.captures == 1
    _same_as_control(sw, got, evs, stats, names, "captured")
    assert max(stats[n]["bbox"][1] for n in names) > 0.0 and max(stats[n]["segm"][1] for n in names) > 0.0          # not a comparison of empty tables
    # without an evaluator: the keyed results carry the planes
    keyed = harness.evaluate_sweep(model, PostProcess(), batches[:1], tasks, dev, captured=step, tokenized=tok)
    assert sorted(keyed) == sorted((i, n) for i in (10, 11) for n in names)
    assert all(set(r) == {"scores", "labels", "boxes", "mask_bits", "mask_size"} for r in keyed.values())
    assert torch.equal(keyed[(11, "b")]["mask_bits"], per_batch[0][(11, "b")]["mask_bits"])
    # eager, two pair stages per batch, the mask program in passes of two pairs
    eager = [_clone_keyed(harness.evaluate_sweep(model, PostProcess(), [b], tasks, dev, max_pairs=4, tokenized=tok, pairs_per_pass=2)) for b in batches]
    assert all(set(r) == {"scores", "labels", "boxes", "mask_bits", "mask_size"} for keyed in eager for r in keyed.values())
    evs, stats = _control(eager, data, names, dev)
    sw = C.SweepEvaluator(data, dev, iou_types=("bbox", "segm"))
    got = harness.evaluate_sweep(model, PostProcess(), batches, tasks, dev, max_pairs=4, tokenized=tok, evaluator=sw, pairs_per_pass=2)
    _same_as_control(sw, got, evs, stats, names, "eager")
    # a detection sweep's evaluator is unchanged: boxes only, no "segm" entry
    assert C.SweepEvaluator(data, dev).iou_types == ("bbox",)
    with pytest.raises(ValueError, match="masks"):
        sw.update_rows({"scores": torch.zeros(1, 4, device=dev), "boxes": torch.zeros(1, 4, 4, device=dev)}, [10], names, [0], [0])
