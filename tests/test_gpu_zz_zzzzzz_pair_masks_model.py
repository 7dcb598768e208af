"""Shared-image training with the mask head on a tiny DETRsegm (one encoder layer, one decoder layer, four queries, dropout 0):
DETRsegm.encode_mask_pairs / decode_mask_pairs against forward() -- the identity pairing against forward() itself, shared pairs against forward() on
the expanded batch (losses and gradients by the bounds of tests/test_gpu_zz_pair_train.py, pred_masks by the rule of
tests/test_gpu_zz_zzzz_mask_sweep_model.py) on the fused tail (64 x 64) and the per-op path (104 x 136), with the matched-only and the dense backward;
and the frozen-detector recipe.  The figures go to pair_masks_model_parity.json (committed as profiles/pair_masks_model_parity.json).
(The file sorts behind every older GPU test file on purpose: DESIGN 8 item 6.)"""
import pytest
import torch

import rounding_bounds as rb

pytestmark = pytest.mark.gpu
FILE = "pair_masks_model_parity.json"

GRAD_COS_MIN = 0.985                                       # tests/test_gpu_zz_pair_train.py (tests/test_gpu_model.py)
GRAD_RATIO = (0.95, 1.06)
LAYER1 = "detr.backbone.0.body.layer1.2.conv3.weight"      # frozen by default; trained here so that C2 (read by adapter3 alone) wants a gradient
CHECKS = ["mask_head.lay1.weight", "mask_head.adapter1.weight", "mask_head.adapter2.weight", "mask_head.adapter3.weight", "mask_head.lay4.weight",
          "mask_head.out_lay.weight", "bbox_attention.k_linear.weight", "detr.input_proj.weight", LAYER1, "detr.backbone.0.body.layer4.2.conv3.weight"]
# image 0 by three pairs, caption 1 by two, not sorted by image
SPEC_A = dict(images=2, captions=3, pairs=[(0, 0), (0, 1), (1, 1), (0, 2), (1, 0)], hw=(64, 64), seed=31, empty=None)
# three images of which image 1 has no pair; a repeated pair; pair 2 has no target.  (104, 136): levels that are no doublings -- the per-op path
SPEC_B = dict(images=3, captions=2, pairs=[(2, 0), (0, 1), (2, 1), (0, 0), (2, 1)], hw=(104, 136), seed=32, empty=2)


def rel_err(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).norm() / (b.detach().float().cpu().norm() + 1e-12))


def _build(dev, **over):
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=4, dropout=0.0, **over)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    assert type(model).__name__ == "DETRsegm" and "masks" in criterion.losses
    for n, b in model.named_buffers():
        if n.endswith("bn3.weight"):
            b.mul_(0.3)                                       # 33 residual blocks keep the activations in range (tests/test_gpu_model.py)
    sd = {k_: v.detach().clone().float() for k_, v in model.state_dict().items()}
    model.to(dev).train()
    model.detr.transformer.text_encoder.config.hidden_dropout_prob = 0.0
    model.detr.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    criterion.train()
    return model, criterion, weight_dict, sd


@pytest.fixture(scope="module")
def setup(dev):
    model, criterion, weight_dict, sd = _build(dev)
    for n, p in model.named_parameters():                  # the last block of layer1 trains (a block trains as a whole): its output is C2
        if n.startswith(LAYER1.rsplit(".", 2)[0] + ".conv"):
            p.requires_grad_(True)
    assert dict(model.named_parameters())[LAYER1].requires_grad
    return model, criterion, weight_dict, sd


def _batch(spec, dev):
    """harness.synthetic_pair_batch(with_masks=True) on the device; spec["empty"]: that pair loses its targets"""
    from toist_amd import harness
    samples, tok, pi, pc, targets, pmap = harness.synthetic_pair_batch(spec["images"], spec["captions"], spec["pairs"], height=spec["hw"][0],
                                                                       width=spec["hw"][1], tokens=8, seed=spec["seed"], max_targets=spec.get("max_targets", 3),
                                                                       with_masks=True)
    assert all(tuple(t["masks"].shape) == (len(t["boxes"]),) + spec["hw"] for t in targets)
    if spec["empty"] is not None:
        t = targets[spec["empty"]]
        assert len(t["boxes"]) > 0
        targets[spec["empty"]] = {**{k_: v[:0] for k_, v in t.items() if torch.is_tensor(v)}, "token_spans": []}
        pmap = torch.cat([t["positive_map"] for t in targets])
    assert sum(len(t["boxes"]) for t in targets) >= spec.get("targets", 3) and pmap.shape[0] == sum(len(t["boxes"]) for t in targets)
    to = lambda t: {k_: (v.to(dev) if torch.is_tensor(v) else v) for k_, v in t.items()}
    return samples.to(dev), tok.to(dev), pi, pc, [to(t) for t in targets], pmap.to(dev)


def _step(model, criterion, weight_dict, batch, shared):
    """one forward + backward: (a) shared = encode_mask_pairs / decode_mask_pairs, (b) forward() on harness.expand_pairs -> outputs, losses, gradients"""
    from toist_amd import harness, kernels
    from toist_amd.mdetr import weighted_total
    model.zero_grad(set_to_none=True)
    if shared:
        losses, out = harness.mask_pair_train_losses(model, criterion, batch)
    else:
        samples, tok, targets, pmap = harness.expand_pairs(*batch)
        mc = model(samples, tok, encode_and_save=True)
        out = model(samples, tok, encode_and_save=False, memory_cache=mc)
        losses = criterion(mc, out, targets, pmap, None)
    total = weighted_total(losses, weight_dict)
    total.backward()
    torch.cuda.synchronize()
    assert kernels.sweep_check(raise_on_failure=False) == 0
    kernels.xdec_check()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    keep = {k_: out[k_].detach().clone() for k_ in ("pred_masks", "pred_logits", "pred_boxes")}
    return keep, {k_: float(v.detach()) for k_, v in losses.items()}, float(total.detach()), grads


# ------------------------------------------------------------------------------------------------------------------ identity
def test_identity_pairs_are_the_ordinary_forward_and_backward(dev, setup):
    """One pair per image and caption, p = (p, p), at 64 x 64: every launch of the forward sees the shapes and the bits of forward()'s.  The backward's
    GroupNorm parameter gradients and the mask loss's gradient are summed with float atomics, so forward() does not repeat itself bit for bit in
    every parameter: a gradient must equal forward()'s bit for bit where three runs of forward() are bit-equal among themselves, and
    differ from the nearest of the three by at most 4 x the largest difference among them elsewhere (the margin covers sampling that noise three times).
    The batch has ONE target per image: gn_bwd_stats_kernel adds every map's share of a GroupNorm weight's gradient with one float atomic per map, in
    any order -- two terms commute, more do not.  (Measured with two targets per image: 8 of 370 gradients differed among three runs of forward(),
    each by one ulp, 4.7e-10 .. 9.3e-10 -- gn1 / gn3 / gn4 / gn5.weight, gn5.bias, lay5.weight / bias, lay1.weight -- and gn2.weight, equal in those
    three runs, differed by the same 4.7e-10 in the fourth: the rule then fails on forward()'s own noise, sampled a fourth time.)
    KNOWN TO FAIL ON CORRECT CODE, measured: of eight separate runs of this test six passed (worst difference / (4 x spread) 0.125 .. 0.5 over
    gn1 / gn4 / gn5.weight) and two failed, both on out_lay.bias = sum of the logit gradient in fp32: equal in the three runs of forward(), it
    differed from them by 3.7e-9 and 7.5e-9 (one and two ulps) in the pair run.  Its noise is forward()'s own -- mask_loss_fwd adds the per-pair
    sums of 16 workgroups with float atomics, the dice gradient reads them -- and the pair run launches the same kernels on the same bits; every
    other tensor carries that gradient in bf16, which rounds it away.  The rule is the issue's and stays as stated."""
    model, criterion, weight_dict, _ = setup
    batch = _batch(dict(images=2, captions=2, pairs=[(0, 0), (1, 1)], hw=(64, 64), seed=34, empty=None, max_targets=1, targets=2), dev)
    assert [len(t["boxes"]) for t in batch[4]] == [1, 1]
    runs = [_step(model, criterion, weight_dict, batch, False) for _ in range(3)]
    out, losses, total, grads = _step(model, criterion, weight_dict, batch, True)
    out0, losses0, total0, g0 = runs[0]
    assert out["pred_masks"].shape == (2, 4, 16, 16) and out["pred_masks"].dtype == torch.float32 and float(out["pred_masks"].abs().max()) > 0
    for name in ("pred_masks", "pred_logits", "pred_boxes"):
        assert torch.equal(out[name], out0[name]), name
    assert set(losses) == set(losses0) and {"loss_mask", "loss_dice"} <= set(losses)
    print("identity pairs: losses", losses, "forward()", losses0)
    for k_ in losses0:
        assert abs(losses[k_] - losses0[k_]) <= 1e-6 * abs(losses0[k_]), (k_, losses[k_], losses0[k_])
    assert set(grads) == set(g0) and all(set(r[3]) == set(g0) for r in runs) and len(g0) > 250
    assert all(n in g0 for n in CHECKS)
    noisy, worst, bad = {}, 0.0, {}
    for n in g0:
        spread = max(float((runs[i][3][n] - runs[j][3][n]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2)))
        diff = min(float((grads[n] - r[3][n]).abs().max()) for r in runs) if spread else float((grads[n] - g0[n]).abs().max())   # from the nearest of forward()'s runs
        if spread == 0.0:
            if not torch.equal(grads[n], g0[n]):
                bad[n] = ("bit-equal among three runs of forward()", diff)
            continue
        noisy[n] = (diff, spread)
        worst = max(worst, diff / (4 * spread))
        if diff > 4 * spread:
            bad[n] = (diff, spread)
    print(f"identity pairs: {len(g0) - len(noisy)} gradients bit-equal, {len(noisy)} with run-to-run noise, worst difference / (4 x spread) {worst:.3f}")
    rb.record("pair_masks.identity.gradients", "64x64 pairs (0,0),(1,1)", worst, file=FILE,
              extra={"parameters": len(g0), "noisy_in_forward": len(noisy), "noisy": {n: [float(f"{v:.3e}") for v in dv] for n, dv in sorted(noisy.items())}})
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ shared pairs
_ORACLE = {}


def _oracle_masks(sd, spec):
    """pred_masks of the fp32 oracle, as tests/test_gpu_zz_zzzz_mask_sweep_model.py builds it: the ResNet once per image, everything else on the
    expanded batch.  Computed once per spec and shared by the cases."""
    key = spec["seed"]
    if key not in _ORACLE:
        from oracle import model_ref
        samples, tok, pi, pc, _, _ = _batch(spec, "cpu")
        pi, pc = pi.long(), pc.long()
        with torch.no_grad():
            dsd = {k_[5:]: v for k_, v in sd.items() if k_.startswith("detr.")}
            feats = [f[pi] for f in model_ref.resnet_body(samples.tensors, dsd, "backbone.0.body.")]
            rmc = model_ref.mdetr_encode(dsd, samples.tensors[pi], samples.mask[pi], tok["input_ids"][pc], tok["attention_mask"][pc], features=feats[-1])
            rout = model_ref.mdetr_decode(dsd, rmc)
            src_proj = torch.nn.functional.conv2d(feats[-1], dsd["input_proj.weight"], dsd["input_proj.bias"])
            fmask = model_ref.downsample_mask(samples.mask[pi], feats[-1].shape[-2:])
            _ORACLE[key] = model_ref.segm_decode(sd, rmc, rout, feats, src_proj, fmask, prefix="detr.")
    return _ORACLE[key]


@pytest.mark.parametrize("dense", [False, True], ids=["matched_only", "dense"])
@pytest.mark.parametrize("spec", [SPEC_A, SPEC_B], ids=["fused_64x64", "per_op_104x136"])
def test_shared_pairs_against_forward_on_the_expanded_batch(dev, setup, monkeypatch, spec, dense):
    """(a) encode_mask_pairs / decode_mask_pairs against (b) forward() on harness.expand_pairs: every loss within 2e-3 + 2e-3 |b|, every checked
    gradient with cosine >= 0.985 and norm ratio in (0.95, 1.06) -- the bounds of tests/test_gpu_zz_pair_train.py -- and pred_masks by the mask
    sweep's rule: S = (a) against the fp32 oracle < 6e-2, D = (a) against (b) <= E = (b) against the oracle.
    dense: MATCHED_ONLY_BACKWARD off, so the backward runs on all P * Q maps (Q maps per pair, no segments); otherwise on the matched maps alone."""
    from toist_amd import kernels, segmentation
    model, criterion, weight_dict, sd = setup
    if dense:
        monkeypatch.setattr(segmentation, "MATCHED_ONLY_BACKWARD", False)
    batch = _batch(spec, dev)
    P, hw = len(spec["pairs"]), spec["hw"]
    out_b, losses_b, total_b, grads_b = _step(model, criterion, weight_dict, batch, False)
    calls = {"rows_pairs": 0, "pairs": 0, "sum_seg": 0, "sum_q": 0, "old": 0}
    spy = {"resize_add_rows_pairs": "rows_pairs", "resize_add_pairs": "pairs", "sum_queries": "old", "sum_segments": "old", "upsample_add_rows": "old",
           "upsample_add": "old", "resize_add": "old"}
    for name, slot in spy.items():
        def wrapped(*a, _real=getattr(kernels, name), _slot=slot, **kw):
            calls[_slot] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(kernels, name, wrapped)
    real_sum = kernels.sum_maps_by_image

    def sum_spy(inp, seg, *a, **kw):
        calls["sum_seg" if seg is not None else "sum_q"] += 1
        return real_sum(inp, seg, *a, **kw)

    monkeypatch.setattr(kernels, "sum_maps_by_image", sum_spy)
    out_a, losses_a, total_a, grads_a = _step(model, criterion, weight_dict, batch, True)
    # which path ran: nothing indexed by row // Q; the image terms through the table; four image sums (lay1 + three adapters)
    fused = hw == (64, 64)
    assert calls["old"] == 0, calls
    assert (calls["sum_q"], calls["sum_seg"]) == ((4, 0) if dense else (0, 4)), calls
    assert calls["rows_pairs"] == (2 if fused and not dense else 0), calls
    assert calls["pairs"] == ((1 + 2 * dense) if fused else 3), calls
    # --- losses
    assert set(losses_a) == set(losses_b) and {"loss_mask", "loss_dice"} <= set(losses_a)
    for k_ in losses_b:
        print(f"{hw} dense={dense} {k_}: shared {losses_a[k_]:.6f} expanded {losses_b[k_]:.6f}")
        assert abs(losses_a[k_] - losses_b[k_]) <= 2e-3 + 2e-3 * abs(losses_b[k_]), (k_, losses_a[k_], losses_b[k_])
    # --- gradients
    assert set(grads_a) == set(grads_b)
    assert grads_a.get("detr.backbone.0.body.layer4.2.conv3.weight") is not None
    figures = {}
    for n in CHECKS:
        a, b = grads_a[n].float().flatten(), grads_b[n].float().flatten()
        assert bool(torch.isfinite(a).all()) and float(b.norm()) > 0, n
        figures[n] = (round(float(torch.nn.functional.cosine_similarity(a, b, dim=0)), 4), round(float(a.norm() / (b.norm() + 1e-20)), 3))
    print(f"{hw} dense={dense} gradients (cos, norm ratio) against the expanded batch:", figures)
    # --- pred_masks
    ref = _oracle_masks(sd, spec)
    up = lambda v: (v + 3) // 4
    assert out_a["pred_masks"].shape == out_b["pred_masks"].shape == (P, 4, up(hw[0]), up(hw[1]))
    E, S, D = rel_err(out_b["pred_masks"], ref), rel_err(out_a["pred_masks"], ref), rel_err(out_a["pred_masks"], out_b["pred_masks"])
    print(f"pair masks {hw}: existing vs oracle {E:.3e}, shared vs oracle {S:.3e}, shared vs existing {D:.3e}")
    rb.record("pair_masks.shared", f"{hw[0]}x{hw[1]} {'dense' if dense else 'matched_only'}", S / 6e-2, file=FILE,
              extra={"existing_vs_oracle": E, "shared_vs_oracle": S, "shared_vs_existing": D, "bound": 6e-2, "total": {"shared": total_a, "expanded": total_b},
                     "min_cos": min(v[0] for v in figures.values()), "min_ratio": min(v[1] for v in figures.values()),
                     "max_ratio": max(v[1] for v in figures.values()), "gradients": figures})
    bad = {n: v for n, v in figures.items() if v[0] < GRAD_COS_MIN or not (GRAD_RATIO[0] < v[1] < GRAD_RATIO[1])}
    assert not bad, f"gradient mismatch (cos, norm ratio): {bad}\nall: {figures}"
    assert S < 6e-2, (hw, S)
    assert D <= E, (hw, D, E)


def test_a_second_consumer_of_pred_masks_takes_the_dense_backward(dev, setup, monkeypatch):
    """pred_masks read by the mask losses AND by another term: autograd sums the two gradients into a dense tensor, the zero sentinel is gone and the
    backward runs on all P * Q maps with the matched rows added in -- over pairs as in forward()."""
    from toist_amd import harness, kernels
    from toist_amd.mdetr import weighted_total
    model, criterion, weight_dict, _ = setup
    batch = _batch(SPEC_A, dev)
    seen = []
    real_sum = kernels.sum_maps_by_image
    monkeypatch.setattr(kernels, "sum_maps_by_image", lambda inp, seg, *a, **kw: (seen.append(seg is not None), real_sum(inp, seg, *a, **kw))[1])
    grads = []
    for extra in (False, True):
        model.zero_grad(set_to_none=True)
        del seen[:]
        losses, out = harness.mask_pair_train_losses(model, criterion, batch)
        total = weighted_total(losses, weight_dict)
        if extra:
            total = total + 0.0 * out["pred_masks"].sum()      # a zero gradient, but a dense one
        total.backward()
        torch.cuda.synchronize()
        assert seen == [extra is False] * 4, seen
        grads.append({n: model.get_parameter(n).grad.detach().float().flatten().clone() for n in CHECKS})
    assert kernels.sweep_check(raise_on_failure=False) == 0
    kernels.xdec_check()
    for n in CHECKS:                                           # the same gradient by either route
        cos = float(torch.nn.functional.cosine_similarity(grads[0][n], grads[1][n], dim=0))
        ratio = float(grads[1][n].norm() / (grads[0][n].norm() + 1e-20))
        assert cos >= GRAD_COS_MIN and GRAD_RATIO[0] < ratio < GRAD_RATIO[1], (n, cos, ratio)


# ------------------------------------------------------------------------------------------------------------------ frozen detector
def test_frozen_detector_trains_the_mask_head_alone(dev):
    """build_model(frozen_weights=...) -> DETRsegm(freeze_detr=True): only the mask head and bbox_attention receive gradients, and they are finite"""
    from toist_amd import harness, kernels
    from toist_amd.mdetr import weighted_total
    model, criterion, weight_dict, _ = _build(dev, frozen_weights="detr.pth")
    assert not any(p.requires_grad for p in model.detr.parameters())
    batch = _batch(SPEC_A, dev)
    losses, out = harness.mask_pair_train_losses(model, criterion, batch)
    total = weighted_total(losses, weight_dict)
    total.backward()
    torch.cuda.synchronize()
    assert kernels.sweep_check(raise_on_failure=False) == 0
    kernels.xdec_check()
    assert bool(torch.isfinite(total)) and out["pred_masks"].shape == (5, 4, 16, 16)
    with_grad = {n for n, p in model.named_parameters() if p.grad is not None}
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert with_grad == trainable and with_grad and all(n.startswith(("mask_head.", "bbox_attention.")) for n in with_grad)
    assert {"mask_head.lay1.weight", "mask_head.adapter3.weight", "mask_head.out_lay.bias", "bbox_attention.q_linear.weight"} <= with_grad
    for n in sorted(with_grad):
        g = model.get_parameter(n).grad
        assert bool(torch.isfinite(g).all()), n
    assert float(model.mask_head.adapter3.weight.grad.abs().sum()) > 0 and float(model.bbox_attention.k_linear.weight.grad.abs().sum()) > 0
