"""toist_amd.harness.CapturedPairTrainStep: the shared-image training step replayed from one hipGraph per bucket, fed with batches of different
image sizes, caption lengths and PAIRINGS -- against the same steps launched eagerly through MDETR.encode_pairs on the same padded inputs (dropout
off), by the protocol and the bounds of tests/test_gpu_captured_step.py::test_captured_step_matches_eager_on_a_mixed_stream.
(The file sorts behind every older GPU test file on purpose: DESIGN 8 item 6.)"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, CAPTIONS, PAIRS = 2, 3, 4
SPREAD = [(0, 0), (1, 1), (0, 2), (1, 0)]
ALL_ON_ONE = [(0, 0), (0, 1), (0, 2), (0, 0)]              # image 0 has all four pairs (caption 0 twice), image 1 has none
REPEATED = [(1, 2), (1, 2), (0, 1), (1, 0)]
CROSSED = [(1, 0), (0, 1), (1, 2), (0, 2)]
# (height, width, tokens, seed, pairing): two image sizes and two caption lengths -> two buckets at pad_hw = 64, pad_tokens = 8 (both sizes pad to
# 128 x 192; 12 tokens pad to 16, 7 to 8).  Steps 0, 2, 3 and 7 carry the SAME images, captions and targets under different pairings.
STREAM = [(128, 160, 12, 50, SPREAD), (96, 192, 7, 51, ALL_ON_ONE), (128, 160, 12, 50, ALL_ON_ONE), (128, 160, 12, 50, SPREAD),
          (96, 192, 7, 52, REPEATED), (96, 192, 12, 53, CROSSED), (128, 160, 7, 54, SPREAD), (128, 160, 12, 50, REPEATED)]


def _model(dev):
    import toist_amd
    from toist_amd import harness
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=2, num_queries=20, dropout=0.0, contrastive_align_loss=True)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    model.transformer.text_encoder.config.hidden_dropout_prob = 0.0
    model.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    criterion.train()
    return model, criterion, weight_dict


def _opt_of(model):
    from toist_amd.optim import FusedClipAdamWEMA
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return FusedClipAdamWEMA([{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n], "lr": 1e-4},
                              {"params": [p for n, p in named if "backbone" in n], "lr": 1e-5},
                              {"params": [p for n, p in named if "text_encoder" in n], "lr": 5e-5}], weight_decay=1e-4, max_norm=0.1)


def test_captured_pair_step_matches_eager_on_a_mixed_stream(dev):
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
        cap = harness.CapturedPairTrainStep(cap_model, criterion, _opt_of(cap_model), weight_dict, batch=BATCH, captions=CAPTIONS, pairs=PAIRS,
                                            max_targets_per_image=6, pad_hw=64, pad_tokens=8)
        eag_opt, cap_opt = _opt_of(eag_model), cap.optimizer
        got, ref, keys, drift = [], [], [], []
        for h, w, tokens, seed, pairing in STREAM:
            samples, tok, pi, pc, targets, pmap = harness.synthetic_pair_batch(BATCH, CAPTIONS, pairing, height=h, width=w, tokens=tokens, seed=seed,
                                                                               max_targets=5)
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
            ids[:, :tokens] = tok["input_ids"]
            att[:, :tokens] = tok["attention_mask"]
            s2, t2 = NestedTensor(img.to(dev), msk.to(dev)), TokenizedText({"input_ids": ids.to(dev), "attention_mask": att.to(dev)})
            st = StaticTargets(PAIRS, 6, 20, 256, dev)
            st.load(targets, pmap, criterion.token_masks_host(targets, None))
            eag_opt.zero_grad(set_to_none=True)
            mc = eag_model.encode_pairs(s2, t2, pi, pc)
            out = eag_model.decode(mc)
            total = toist_amd.weighted_total(criterion(mc, out, st, None, None), weight_dict)
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
        print("captured pair step: loss", got, "eager", ref, "drift", drift, "buckets", sorted(set(keys)))
        buckets = len(set(keys))
        assert buckets == 2 and cap.captures == buckets and cap.replays == len(STREAM) - buckets, (keys, cap.captures, cap.replays)
        assert all(map(lambda v: v == v and abs(v) < 1e6, got)), got
        bound = lambda b: 2e-3 * abs(b) + 1e-4
        for i, (a, b) in enumerate(zip(got, ref)):
            assert abs(a - b) <= bound(b), (i, keys[i], got, ref)
        assert max(drift) <= 4e-4, drift
        # the graph re-reads the tables: steps 2, 3 and 7 replay one graph on the same images, captions and targets, only the pairing differs -- the
        # eager losses of two pairings lie more than twice the bound apart, so a replay within the bound of its own twin did not use the other table
        for i, j in ((2, 3), (3, 7), (2, 7)):
            assert abs(ref[i] - ref[j]) > 2 * max(bound(ref[i]), bound(ref[j])) and got[i] != got[j], (i, j, got, ref)
        assert len(cap._buckets) <= cap.max_graphs
    finally:
        kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS = old_seed, old_reuse


def test_captured_pair_step_refuses_bad_batches_before_any_launch(dev):
    from types import SimpleNamespace
    from toist_amd import engine, harness, kernels
    model, criterion, weight_dict = _model(dev)
    old_seed, old_reuse = kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS
    try:
        with pytest.raises(ValueError, match="mask losses"):
            harness.CapturedPairTrainStep(model, SimpleNamespace(losses=["labels", "boxes", "cardinality", "masks"]), None, weight_dict, batch=BATCH,
                                          captions=CAPTIONS, pairs=PAIRS)
        cap = harness.CapturedPairTrainStep(model, criterion, _opt_of(model), weight_dict, batch=BATCH, captions=CAPTIONS, pairs=PAIRS,
                                            max_targets_per_image=6, pad_hw=64, pad_tokens=8)
        mk = lambda B=BATCH, T=CAPTIONS, pairs=SPREAD: harness.synthetic_pair_batch(B, T, pairs, height=64, width=64, tokens=8, seed=3, max_targets=2,
                                                                                      device=dev)
        with pytest.raises(ValueError, match="exactly 4 pairs"):
            cap.step(*mk(pairs=SPREAD[:3]))
        with pytest.raises(ValueError, match="2 images and 3 captions"):
            cap.step(*mk(B=3))
        with pytest.raises(ValueError, match="2 images and 3 captions"):
            cap.step(*mk(T=2, pairs=[(0, 0), (1, 1), (1, 0), (0, 1)]))
        samples, tok, pi, pc, targets, pmap = mk()
        for bad_i, bad_c in (([0, 2, 1, 0], pc), (pi, [0, 3, 1, -1]), (pi.to(dev), torch.tensor([0, 3, 1, 2], dtype=torch.int32, device=dev))):
            with pytest.raises(ValueError, match="outside"):
                cap.step(samples, tok, bad_i, bad_c, targets, pmap)
        assert cap.captures == 0 and cap.replays == 0 and not cap._buckets            # nothing was built, uploaded or launched
        assert kernels.sweep_check(raise_on_failure=False) == 0
    finally:
        kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS = old_seed, old_reuse
