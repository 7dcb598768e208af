"""SetCriterion on captions padded to a bucket's Lp tokens, with the live-token word of matcher.LiveStaticTargets, against the same criterion on the
captions truncated to their own L: one set of model-shaped outputs (pred_logits, pred_boxes, proj_queries identical in both runs), the same keys, the
detection terms bit-identical (no token enters them; with two images every per-layer sum of the kernels' atomics has one order), the
contrastive-alignment terms within 1e-4 relative.  Single model and the paired (noun, pronoun) criterion of the distillation recipe with softkd and
nsthl2 on, the two sides with different L under one Lp."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
B, Q, K, LAYERS, D, DT = 2, 20, 256, 3, 64, 32
LP = 16


def _criterion(dev, pair):
    from toist_amd.matcher import HungarianMatcher
    from toist_amd.mdetr import SetCriterion
    args = types.SimpleNamespace(num_queries=Q, nsthl2_loss=pair, softkd_loss=pair)
    return SetCriterion(args, 255, matcher=HungarianMatcher(1.0, 5.0, 2.0), eos_coef=0.1, temperature=0.07,
                        losses=["labels", "boxes", "cardinality", "contrastive_align"] + (["nsthl2", "softkd"] if pair else [])).to(dev)


def _model_outputs(seed, dev):
    """What does not depend on the caption length: stacked logits / boxes / query projections of one model, as leaves."""
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(LAYERS, B, Q, K, generator=g) * 2).to(dev).requires_grad_(True)
    raw = torch.randn(LAYERS, B, Q, 4, generator=g)
    bx = torch.cat([torch.sigmoid(raw[..., :2]) * 0.6 + 0.2, torch.sigmoid(raw[..., 2:]) * 0.35 + 0.05], -1).to(dev).requires_grad_(True)
    pq = torch.nn.functional.normalize(torch.randn(LAYERS, B, Q, D, generator=g), dim=-1).to(dev).requires_grad_(True)
    return lg, bx, pq


def _outputs(lg, bx, pq, pt):
    return {"pred_logits": lg[-1], "pred_boxes": bx[-1], "proj_queries": pq[-1], "proj_tokens": pt,
            "_stacked": {"pred_logits": lg, "pred_boxes": bx, "proj_queries": pq},
            "aux_outputs": [{"pred_logits": lg[i], "pred_boxes": bx[i], "proj_queries": pq[i], "proj_tokens": pt} for i in range(LAYERS - 1)]}


def _tokens(seed, L_own, dev):
    """Token projections and text memory of a caption of L_own tokens inside LP positions: the padded rows hold other (finite) values, as the
    text encoder's outputs at pad positions do."""
    g = torch.Generator().manual_seed(seed)
    pt = torch.nn.functional.normalize(torch.randn(B, LP, D, generator=g), dim=-1)
    pt[:, L_own:] *= 7.0
    text = torch.randn(LP, B, DT, generator=g)
    return pt.to(dev), text.to(dev)


def _static(crit, dev, tok, targets, pmap, captions, pronoun, tokens, live):
    from toist_amd.distill import DistillTables
    from toist_amd.matcher import LiveStaticTargets, StaticTargets
    host_t = [{k_: (v.cpu() if torch.is_tensor(v) else v) for k_, v in t.items()} for t in targets]
    if live is None:
        st = StaticTargets(B, 6, Q, K, dev).load(host_t, pmap.cpu(), crit.token_masks_host(host_t, tok))
    else:
        st = LiveStaticTargets(B, 6, Q, K, dev).load(host_t, pmap.cpu(), crit.token_masks_host(host_t, tok), live_tokens=live)
    if captions is not None:           # (the paired criterion reads the side's caption tables)
        st.distill = DistillTables(B, tokens, dev, pronoun_side=pronoun).load(tok, host_t, captions)
    return st


def _compare(padded, cut, exact_prefixes=("loss_ce", "loss_bbox", "loss_giou", "cardinality_error", "loss_softkd")):
    assert set(padded) == set(cut), sorted(set(padded) ^ set(cut))
    for k_ in sorted(cut):
        a, b = float(padded[k_]), float(cut[k_])
        name = k_.split("noun_")[-1].split("sth_")[-1]
        print(f"{k_}: padded {a!r} truncated {b!r}")
        if name.startswith(exact_prefixes):
            assert a == b, (k_, a, b)
        elif "contrastive" in name:
            assert abs(a - b) <= 1e-4 * abs(b), (k_, a, b)
        else:      # loss_nsthl2: a weighted sum over Lp tokens (zero weights beyond L) against the sum over L: fp32 reassociation of <= 16 terms
            assert name == "loss_nsthl2" and abs(a - b) <= 1e-5 * abs(b) + 1e-9, (k_, a, b)


@pytest.mark.parametrize("seed,L_own", [(3, 12), (4, 9)])
def test_single_model_criterion_on_a_padded_caption(dev, seed, L_own):
    from toist_amd import harness
    crit = _criterion(dev, pair=False)
    _, tok, targets, pmap = harness.synthetic_batch(B, 64, 64, tokens=L_own, seed=seed, max_targets=5)
    lg, bx, pq = _model_outputs(seed, dev)
    pt, _ = _tokens(seed + 50, L_own, dev)
    pt.requires_grad_(True)
    padded = crit(None, _outputs(lg, bx, pq, pt), _static(crit, dev, tok, targets, pmap, None, False, LP, L_own), None, None)
    sum(v for k_, v in padded.items() if "contrastive" in k_).backward()
    g_pq, g_pt = pq.grad.clone(), pt.grad.clone()
    pq.grad = pt.grad = None
    cut = crit(None, _outputs(lg, bx, pq, pt[:, :L_own].contiguous()), _static(crit, dev, tok, targets, pmap, None, False, L_own, None), None, None)
    _compare(padded, cut)
    sum(v for k_, v in cut.items() if "contrastive" in k_).backward()
    if sum(len(t["boxes"]) for t in targets):
        assert float(g_pq.abs().max()) > 0
    assert float((g_pq - pq.grad).abs().max()) <= 2e-3 * float(pq.grad.abs().max()) + 1e-7
    assert float((g_pt - pt.grad).abs().max()) <= 2e-3 * float(pt.grad.abs().max()) + 1e-7
    assert not g_pt[:, L_own:].any()


@pytest.mark.parametrize("seed,L_noun,L_sth", [(5, 12, 10), (6, 9, 11)])
def test_paired_criterion_with_two_caption_lengths_under_one_bucket(dev, seed, L_noun, L_sth):
    from toist_amd import harness
    from toist_amd.matcher import check_lsap_pending
    crit = _criterion(dev, pair=True)
    batch = harness.synthetic_distill_batch(B, 64, 64, tokens=L_noun, tokens_pronoun=L_sth, seed=seed, max_targets=5)
    sides = []
    for i, L_own in enumerate((L_noun, L_sth)):
        lg, bx, pq = _model_outputs(seed + 10 * i, dev)
        pt, text = _tokens(seed + 50 + i, L_own, dev)
        sides.append((lg, bx, pq, pt, text, L_own))

    def run(padded):
        outs, mcs, sts = [], [], []
        for i, (lg, bx, pq, pt, text, L_own) in enumerate(sides):
            n = LP if padded else L_own
            outs.append(_outputs(lg, bx, pq, pt[:, :n].contiguous()))
            mcs.append({"text_memory": text[:n]})
            sts.append(_static(crit, dev, batch["tokenized"][i], batch["targets"][i], batch["positive_map"][i], batch["captions"][i], i == 1, n,
                               L_own if padded else None))
        losses = crit(mcs, outs, sts, None, None)
        torch.cuda.synchronize()
        check_lsap_pending()
        return {k_: v.detach().clone() for k_, v in losses.items()}

    padded, cut = run(True), run(False)
    assert {"noun_loss_contrastive_align", "sth_loss_contrastive_align_0", "loss_nsthl2", "loss_softkd", "loss_softkd_1"} <= set(padded)
    _compare(padded, cut)
