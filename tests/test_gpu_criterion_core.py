"""The list-of-dicts and the StaticTargets front ends of the pair losses share one device-table core (matcher.pair_slots, mdetr._softkd,
segmentation._mask_losses).  Both front ends against the CPU oracle at the counts where a shared slot table can go wrong: an image without
targets, a batch without any pair (Mtot == 0), an image whose targets use up every query (an LSAP problem of size 0), and a static capacity
larger than Mtot."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
L, B, Q, K = 2, 2, 6, 8
CAP_PER_IMAGE = 6


def close(got, want):
    return abs(float(got) - float(want)) <= 1e-4 * abs(float(want)) + 1e-6


def model_side(seed, counts):
    """(outputs dict with L layers, host targets, host positive map) of one model: fp32 random logits, boxes in range."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(L, B, Q, K, generator=g) * 2
    boxes = torch.cat([0.3 + 0.4 * torch.rand(L, B, Q, 2, generator=g), 0.1 + 0.2 * torch.rand(L, B, Q, 2, generator=g)], -1)
    targets, pms = [], []
    for i, t in enumerate(counts):
        targets.append({"boxes": torch.cat([0.3 + 0.4 * torch.rand(t, 2, generator=g), 0.1 + 0.2 * torch.rand(t, 2, generator=g)], -1),
                        "labels": torch.ones(t, dtype=torch.int64)})
        pm = torch.zeros(t, K)
        pm[:, 1 + i:4 + i] = 1.0 / 3
        pms.append(pm)
    return logits, boxes, targets, torch.cat(pms)


def outputs_of(logits, boxes, dev, grad):
    lg = logits.to(dev).requires_grad_(grad)
    layers = [{"pred_logits": lg[l], "pred_boxes": boxes[l].to(dev)} for l in range(L)]
    out = dict(layers[-1])
    out["aux_outputs"] = layers[:-1]
    return lg, out


def to_dev(targets, dev):
    return [{k_: v.to(dev) for k_, v in t.items()} for t in targets]


def criterion():
    from toist_amd.matcher import HungarianMatcher
    from toist_amd.mdetr import SetCriterion
    args = types.SimpleNamespace(num_queries=Q, nsthl2_loss=False, softkd_loss=True)
    return SetCriterion(args, K - 1, matcher=HungarianMatcher(1, 5, 2), eos_coef=0.1, losses=["labels", "boxes", "cardinality", "softkd"], temperature=0.07)


def static_image(targets, pm, dev, **kw):
    from toist_amd.matcher import StaticTargets
    return StaticTargets(B, CAP_PER_IMAGE, Q, K=K, device=dev, **kw).load(targets, pm)


@pytest.mark.parametrize("counts", [(0, 3), (0, 0), (6, 1)])
def test_softkd_of_both_front_ends_against_the_oracle(dev, counts):
    from oracle import distill_ref
    crit = criterion()
    (lg_n, bx_n, t_n, pm_n), (lg_s, bx_s, t_s, pm_s) = model_side(11, counts), model_side(12, counts)
    # the oracle pairs the queries through the product's own assignment (the matcher has its own bit-exact tests)
    m_n = crit.matcher.match_layers(lg_n.to(dev), bx_n.to(dev), to_dev(t_n, dev), pm_n.to(dev))
    m_s = crit.matcher.match_layers(lg_s.to(dev), bx_s.to(dev), to_dev(t_s, dev), pm_s.to(dev))
    want = [distill_ref.loss_softkd(lg_n[l], lg_s[l], bx_n[l], bx_s[l], m_n.to_list(l), m_s.to_list(l)) for l in range(L)]
    got = {}
    for path in ("list", "static"):
        leaf_n, out_n = outputs_of(lg_n, bx_n, dev, True)
        leaf_s, out_s = outputs_of(lg_s, bx_s, dev, True)
        if path == "list":
            losses = crit(None, [out_n, out_s], [to_dev(t_n, dev), to_dev(t_s, dev)], [pm_n.to(dev), pm_s.to(dev)])
        else:
            st_n, st_s = static_image(t_n, pm_n, dev), static_image(t_s, pm_s, dev)
            assert st_n.cap > sum(min(Q, c) for c in counts)
            losses = crit(None, [out_n, out_s], [st_n, st_s], None)
        got[path] = [float(losses["loss_softkd_0"].detach()), float(losses["loss_softkd"].detach())]
        print(path, counts, got[path], [float(w) for w in want])
        for l in range(L):
            assert close(got[path][l], want[l]), (path, l, got[path][l], float(want[l]))
        (losses["loss_softkd"] + losses["loss_softkd_0"]).backward()          # the cross loss reaches the student's logits only
        assert leaf_s.grad is not None and float(leaf_s.grad.abs().sum()) > 0 and bool(torch.isfinite(leaf_s.grad).all())
        assert leaf_n.grad is None
    for l in range(L):
        assert close(got["static"][l], got["list"][l]), (l, got)


def test_softkd_refuses_unequal_counts_on_both_front_ends(dev):
    crit = criterion()
    (lg_n, bx_n, t_n, pm_n), (lg_s, bx_s, t_s, pm_s) = model_side(11, (1, 2)), model_side(12, (2, 1))
    _, out_n = outputs_of(lg_n, bx_n, dev, False)
    _, out_s = outputs_of(lg_s, bx_s, dev, True)
    with pytest.raises(ValueError):
        crit(None, [out_n, out_s], [to_dev(t_n, dev), to_dev(t_s, dev)], [pm_n.to(dev), pm_s.to(dev)])
    losses = crit(None, [out_n, out_s], [static_image(t_n, pm_n, dev), static_image(t_s, pm_s, dev)], None)
    assert all(bool(torch.isnan(losses[k_])) for k_ in ("loss_softkd_0", "loss_softkd"))
    assert bool(torch.isfinite(losses["sth_loss_ce"]))


@pytest.mark.parametrize("counts", [(0, 3), (2, 1)])
def test_mask_losses_of_both_front_ends(dev, counts):
    from oracle import model_ref
    from toist_amd.matcher import HungarianMatcher
    from toist_amd.segmentation import mask_losses, mask_losses_static
    TH = TW = 8
    logits, boxes, targets, pm = model_side(21, counts)
    g = torch.Generator().manual_seed(5)
    for t in targets:
        t["masks"] = torch.rand(t["boxes"].shape[0], TH, TW, generator=g) > 0.6
    pred = torch.randn(B, Q, 4, 4, generator=g) * 2
    num_boxes = float(max(sum(counts), 1))
    matcher = HungarianMatcher(1, 5, 2)
    match = matcher.match_layers(logits.to(dev), boxes.to(dev), to_dev(targets, dev), pm.to(dev))
    p_ref = pred.clone().requires_grad_(True)
    ref = model_ref.loss_masks(p_ref, targets, match.to_list(L - 1), num_boxes)
    (ref["loss_mask"] * 1.5 + ref["loss_dice"] * 0.7).backward()
    p_list = pred.to(dev).requires_grad_(True)
    got = mask_losses({"pred_masks": p_list}, to_dev(targets, dev), match, L - 1, torch.tensor(num_boxes, device=dev))
    (got["loss_mask"] * 1.5 + got["loss_dice"] * 0.7).backward()
    for k_ in ("loss_mask", "loss_dice"):
        print(counts, k_, float(got[k_]), float(ref[k_]))
        assert close(got[k_], ref[k_]), (k_, float(got[k_]), float(ref[k_]))
    err = float((p_list.grad.cpu() - p_ref.grad).abs().max())
    assert err <= 1e-3 * float(p_ref.grad.abs().max()) + 1e-8, err
    # the static image of the same batch: capacity 12 > Mtot, layer L - 1 of a two-layer assignment
    st = static_image(targets, pm, dev, mask_hw=(TH, TW), mask_pred_of=lambda side: side // 2)
    match_st = matcher.match_layers_static(logits.to(dev), boxes.to(dev), st)
    p_st = pred.to(dev).requires_grad_(True)
    got_st = mask_losses_static({"pred_masks": p_st}, st, match_st, L - 1, L)
    (got_st["loss_mask"] * 1.5 + got_st["loss_dice"] * 0.7).backward()
    for k_ in ("loss_mask", "loss_dice"):
        assert close(got_st[k_], got[k_]), (k_, float(got_st[k_]), float(got[k_]))
    err = float((p_st.grad - p_list.grad).abs().max())
    assert err <= 1e-3 * float(p_list.grad.abs().max()) + 1e-8, err
