"""toist_amd.harness.CapturedMaskPairTrainStep: the shared-image training step WITH the mask head and the mask losses replayed from one hipGraph per
bucket, fed with batches of two image sizes and different PAIRINGS -- against the same steps launched eagerly through DETRsegm.encode_mask_pairs /
decode_mask_pairs on the same padded inputs (dropout off), by the protocol and the bounds of
tests/test_gpu_zz_pair_train_captured.py::test_captured_pair_step_matches_eager_on_a_mixed_stream.
(The file builds captured steps, so it sorts behind every older GPU test file: DESIGN 8 item 6.)"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, CAPTIONS, PAIRS, QUERIES, MAX_T = 2, 3, 4, 4, 4
SPREAD = [(0, 0), (1, 1), (0, 2), (1, 0)]
ALL_ON_ONE = [(0, 0), (0, 1), (0, 2), (0, 0)]              # image 0 has all four pairs (caption 0 twice), image 1 has none
REPEATED = [(1, 2), (1, 2), (0, 1), (1, 0)]
CROSSED = [(1, 0), (0, 1), (1, 2), (0, 2)]
# (height, width, seed, pairing): two image sizes -> two buckets at pad_hw = 64 (64 x 64; 96 x 128 pads to 128 x 128, so that bucket's ground-truth
# masks and predictions are larger than the batch's own: StaticTargets.valid_hw).  Steps 0, 2, 3 and 5 carry the SAME images, captions and
# targets under different pairings.
STREAM = [(64, 64, 60, SPREAD), (96, 128, 61, ALL_ON_ONE), (64, 64, 60, ALL_ON_ONE), (64, 64, 60, REPEATED), (96, 128, 62, CROSSED), (64, 64, 60, CROSSED)]
TOKENS = 8


def _model(dev):
    import toist_amd
    from toist_amd import harness
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=QUERIES, dropout=0.0)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    for n, b in model.named_buffers():
        if n.endswith("bn3.weight"):
            b.mul_(0.3)
    model.to(dev).train()
    model.detr.transformer.text_encoder.config.hidden_dropout_prob = 0.0
    model.detr.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    criterion.train()
    assert "masks" in criterion.losses
    return model, criterion, weight_dict


def _opt_of(model):
    from toist_amd.optim import FusedClipAdamWEMA
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return FusedClipAdamWEMA([{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n], "lr": 1e-4},
                              {"params": [p for n, p in named if "backbone" in n], "lr": 1e-5},
                              {"params": [p for n, p in named if "text_encoder" in n], "lr": 5e-5}], weight_decay=1e-4, max_norm=0.1)


def _pair_batch(h, w, seed, pairing, B=BATCH, T=CAPTIONS, device="cpu"):
    from toist_amd import harness
    return harness.synthetic_pair_batch(B, T, pairing, height=h, width=w, tokens=TOKENS, seed=seed, max_targets=3, with_masks=True, device=device)


def test_captured_mask_pair_step_matches_eager_on_a_mixed_stream(dev):
    import toist_amd
    from toist_amd import engine, harness, kernels
    from toist_amd.matcher import StaticTargets
    from toist_amd.misc import NestedTensor
    from toist_amd.transformer import TokenizedText
    model0, criterion, weight_dict = _model(dev)
    old_seed, old_reuse = kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    try:
        cap_model, eag_model = copy.deepcopy(model0), copy.deepcopy(model0)
        cap = harness.CapturedMaskPairTrainStep(cap_model, criterion, _opt_of(cap_model), weight_dict, batch=BATCH, captions=CAPTIONS, pairs=PAIRS,
                                                max_targets_per_image=MAX_T, pad_hw=64, pad_tokens=8)
        assert cap.masks and isinstance(cap, harness.CapturedPairTrainStep)
        eag_opt, cap_opt = _opt_of(eag_model), cap.optimizer
        got, ref, keys, drift = [], [], [], []
        for h, w, seed, pairing in STREAM:
            samples, tok, pi, pc, targets, pmap = _pair_batch(h, w, seed, pairing)
            assert sum(len(t["boxes"]) for t in targets) > 0
            key = cap.bucket_of(samples, tok)
            keys.append(key)
            # both loops start every step from the SAME weights and optimizer moments: each step is an independent comparison
            with torch.no_grad():
                for p_e, p_c in zip(eag_model.parameters(), cap_model.parameters()):
                    p_e.copy_(p_c)
                for a_e, a_c in zip(eag_opt.exp_avg + eag_opt.exp_avg_sq, cap_opt.exp_avg + cap_opt.exp_avg_sq):
                    a_e.copy_(a_c)
                eag_opt.state.copy_(cap_opt.state)
            engine.bump_weight_epoch()
            got.append(float(cap.step(samples.to(dev), tok.to(dev), pi, pc, targets, pmap).detach()))
            # the same step, eagerly, on the same padded inputs
            Hp, Wp, Lp = key
            img, msk = torch.zeros(BATCH, 3, Hp, Wp), torch.ones(BATCH, Hp, Wp, dtype=torch.bool)
            img[:, :, :h, :w] = samples.tensors
            msk[:, :h, :w] = samples.mask
            ids, att = torch.full((CAPTIONS, Lp), 1, dtype=torch.int64), torch.zeros(CAPTIONS, Lp, dtype=torch.int64)
            ids[:, :TOKENS] = tok["input_ids"]
            att[:, :TOKENS] = tok["attention_mask"]
            s2, t2 = NestedTensor(img.to(dev), msk.to(dev)), TokenizedText({"input_ids": ids.to(dev), "attention_mask": att.to(dev)})
            st = StaticTargets(PAIRS, MAX_T, QUERIES, 256, dev, mask_hw=(Hp, Wp))
            st.load(targets, pmap, None)
            eag_opt.zero_grad(set_to_none=True)
            mc = eag_model.encode_mask_pairs(s2, t2, pi, pc)
            out = eag_model.decode_mask_pairs(mc)
            assert out["pred_masks"].shape == (PAIRS, QUERIES, Hp // 4, Wp // 4) and out["pred_masks"].requires_grad
            losses = criterion(mc, out, st, None, None)
            assert {"loss_mask", "loss_dice"} <= set(losses)
            total = toist_amd.weighted_total(losses, weight_dict)
            total.backward()
            eag_opt.step()
            ref.append(float(total.detach()))
            worst = 0.0
            for (n, p), (_, q) in zip(cap_model.named_parameters(), eag_model.named_parameters()):
                if p.requires_grad:
                    worst = max(worst, float((p - q).detach().abs().max()))
            drift.append(worst)
        torch.cuda.synchronize()
        kernels.xdec_check()
        assert kernels.sweep_check(raise_on_failure=False) == 0
        print("captured mask pair step: loss", got, "eager", ref, "drift", drift, "buckets", sorted(set(keys)))
        buckets = len(set(keys))
        assert buckets == 2 and cap.captures == buckets and cap.replays == len(STREAM) - buckets, (keys, cap.captures, cap.replays)
        assert all(map(lambda v: v == v and abs(v) < 1e6, got)), got
        bound = lambda b: 2e-3 * abs(b) + 1e-4
        for i, (a, b) in enumerate(zip(got, ref)):
            assert abs(a - b) <= bound(b), (i, keys[i], got, ref)
        assert max(drift) <= 4e-4, drift
        # the graph re-reads the tables: steps 2, 3 and 5 replay one graph on the same images, captions and targets, only the pairing differs -- the
        # eager losses of two pairings lie more than twice the bound apart, so a replay within the bound of its own twin did not use the other table
        for i, j in ((2, 3), (3, 5), (2, 5)):
            assert abs(ref[i] - ref[j]) > 2 * max(bound(ref[i]), bound(ref[j])) and got[i] != got[j], (i, j, got, ref)
        assert len(cap._buckets) <= cap.max_graphs
    finally:
        kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS = old_seed, old_reuse


def test_captured_mask_pair_step_refuses_before_any_upload(dev):
    from toist_amd import engine, harness, kernels
    model, criterion, weight_dict = _model(dev)
    old_seed, old_reuse = kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS
    try:
        with pytest.raises(ValueError, match="mask head"):                                       # a detection model: CapturedPairTrainStep is its step
            harness.CapturedMaskPairTrainStep(model.detr, criterion, None, weight_dict, batch=BATCH, captions=CAPTIONS, pairs=PAIRS)
        with pytest.raises(ValueError):
            harness.CapturedMaskPairTrainStep(model, criterion, None, weight_dict, batch=BATCH, captions=CAPTIONS, pairs=0)
        cap = harness.CapturedMaskPairTrainStep(model, criterion, _opt_of(model), weight_dict, batch=BATCH, captions=CAPTIONS, pairs=PAIRS,
                                                max_targets_per_image=MAX_T, pad_hw=64, pad_tokens=8)
        with pytest.raises(ValueError, match="exactly 4 pairs"):
            cap.step(*_pair_batch(64, 64, 3, SPREAD[:3], device=dev))
        with pytest.raises(ValueError, match="2 images and 3 captions"):
            cap.step(*_pair_batch(64, 64, 3, SPREAD, B=3, device=dev))
        samples, tok, pi, pc, targets, pmap = _pair_batch(64, 64, 3, SPREAD, device=dev)
        by_size = [{**{k_: v for k_, v in t.items() if k_ != "masks"}, "mask_size": (64, 64)} for t in targets]
        with pytest.raises(ValueError, match="mask_size"):
            cap.step(samples, tok, pi, pc, by_size, pmap)
        with pytest.raises(ValueError, match="masks"):                                           # mask losses, but a target without its masks
            cap.step(samples, tok, pi, pc, [{k_: v for k_, v in t.items() if k_ != "masks"} for t in targets], pmap)
        with pytest.raises(ValueError, match="target_masks"):
            cap.step(samples, tok, pi, pc, targets, pmap, target_masks=object())
        with pytest.raises(ValueError, match="outside"):
            cap.step(samples, tok, [0, 2, 1, 0], pc, targets, pmap)
        assert cap.captures == 0 and cap.replays == 0 and not cap._buckets and not cap._ready   # nothing was built, uploaded or launched
        assert kernels.sweep_check(raise_on_failure=False) == 0
    finally:
        kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS = old_seed, old_reuse
