"""The live-token entry points of the contrastive-alignment kernels (csrc/contrastive.hip: toist_contrastive_fwd_live / _bwd_ws_live): a launch on
proj_tokens padded to T columns with a device word that says Tl of them are live must be the launch on proj_tokens[:, :Tl] -- loss and both gradients
-- and must write zeros into the dead rows of d proj_tokens.  Against fp32 autograd through oracle/model_ref.loss_contrastive_align on the truncated
inputs with the bounds of test_gpu_criterion.py::test_contrastive_align_gradients_vs_oracle (loss 1e-4 relative, gradients 2e-3 * scale + 1e-7), and
against the truncated call of the existing entry points.

The assignment is the device matcher's, computed once per Q and used by every call and by the oracle, so it is identical by construction.  One of
the three images has no target, so every layer's loss is the sum of two block terms and a zero: the order of the forward's atomics cannot change it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
L, B, D, SIZES = 6, 3, 64, [3, 0, 2]
W = [0.3, 1.0, 0.7, 1.3, 0.9, 1.1]           # unequal upstream weights of the six layers
GARBAGE = 3.0e18                             # large and finite: a product of two of them is inf, any read of a dead column shows


def _spans(Tl):
    """Spans of the five targets inside the first Tl tokens: one ends at the last live token; beyond 64 / 128 tokens some sit in the upper mask words."""
    if Tl == 1:
        per = [[(0, 0)], [(0, 0)], [(0, 0)], [(0, 0)], [(0, 0)]]
    elif Tl <= 16:
        per = [[(1, 2)], [(2, 3)], [(1, 1), (4, Tl - 1)], [(0, 1)], [(Tl - 2, Tl - 1)]]
    elif Tl <= 72:
        per = [[(1, 2), (60, Tl - 1)], [(2, 3)], [(1, 1), (62, 63)], [(0, 1)], [(Tl - 1, Tl - 1)]]
    else:
        per = [[(1, 2), (127, 129)], [(100, 110)], [(1, 1), (120, Tl - 1)], [(63, 64)], [(Tl - 3, Tl - 1)]]
    return [per[:3], [], per[3:]]


@functools.lru_cache(maxsize=None)
def _setup(Q):
    """Per Q, once: model-shaped outputs, targets, the device assignment of every layer and its host copy for the oracle."""
    from toist_amd.matcher import HungarianMatcher
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11 + Q)
    logits = torch.randn(L, B, Q, 256, generator=g) * 2
    raw = torch.randn(L, B, Q, 4, generator=g)
    boxes = torch.cat([torch.sigmoid(raw[..., :2]) * 0.6 + 0.2, torch.sigmoid(raw[..., 2:]) * 0.35 + 0.05], -1)
    targets, rows = [], []
    for n in SIZES:
        targets.append({"boxes": torch.cat([torch.rand(n, 2, generator=g) * 0.6 + 0.2, torch.rand(n, 2, generator=g) * 0.35 + 0.05], -1).to(dev)})
        pm = torch.rand(n, 256, generator=g)
        rows.append(pm / pm.sum(-1, keepdim=True))
    match = HungarianMatcher(1.0, 5.0, 2.0).match_layers(logits.to(dev), boxes.to(dev), targets, torch.cat(rows).to(dev))
    idx = [match.to_list(l) for l in range(L)]
    raw_q = torch.randn(L, B, Q, D, generator=g)
    return match, idx, raw_q


@functools.lru_cache(maxsize=None)
def _tokens(T):
    return torch.randn(B, T, D, generator=torch.Generator().manual_seed(100 + T))


@functools.lru_cache(maxsize=None)
def _oracle(Q, T, Tl):
    """fp32 autograd through the oracle on the TRUNCATED inputs -> (weighted total, d raw_q, d raw_t[:, :Tl])."""
    from oracle import model_ref
    _, idx, raw_q = _setup(Q)
    rq, rt = raw_q.clone().requires_grad_(True), _tokens(T)[:, :Tl].clone().requires_grad_(True)
    pq, pt = torch.nn.functional.normalize(rq, dim=-1), torch.nn.functional.normalize(rt, dim=-1)
    tot = 0
    for l in range(L):
        tot = tot + W[l] * model_ref.loss_contrastive_align({"proj_queries": pq[l], "proj_tokens": pt}, _spans(Tl), idx[l], float(sum(SIZES)))["loss_contrastive_align"]
    tot.backward()
    return float(tot), rq.grad, rt.grad


def _tok_mask(Tl, dev):
    from toist_amd.mdetr import SetCriterion
    rows = []
    for i, sp in enumerate(_spans(Tl)):
        rows += SetCriterion._span_bits({"boxes": torch.zeros(len(sp), 4), "token_spans": sp}, i, None)
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 4).to(dev)


def _device(Q, raw_t, Tl, live, dev):
    """l2_normalize -> _ContrastiveFn -> weighted total -> backward on the device; live = the word's value or None.  -> (total, losses, d raw_q, d raw_t)."""
    from toist_amd.mdetr import _ContrastiveFn, l2_normalize
    match, _, raw_q = _setup(Q)
    word = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
    dq, dt = raw_q.to(dev).requires_grad_(True), raw_t.to(dev).requires_grad_(True)
    nq = l2_normalize(dq)
    if live is not None and live < raw_t.shape[1]:
        # the padded rows reach the kernel as garbage (they are no unit vectors: a bucket's padded positions hold whatever the text encoder made of pad tokens)
        nt = torch.cat([l2_normalize(dt[:, :live]), dt[:, live:] * 0 + GARBAGE], 1)
    else:
        nt = l2_normalize(dt)
    losses = _ContrastiveFn.apply(nq, nt.contiguous(), match, _tok_mask(Tl, dev), torch.tensor([float(sum(SIZES))], device=dev), 0.07, word)
    total = (losses * torch.tensor(W, device=dev)).sum()
    total.backward()
    return float(total), losses.detach().clone(), dq.grad, dt.grad


CASES = [(16, 1), (16, 7), (16, 16), (72, 64), (72, 65), (200, 130), (200, 200)]


@pytest.mark.parametrize("Q", [20, 100])
@pytest.mark.parametrize("T,Tl", CASES)
def test_live_tokens_equal_the_truncated_launch_and_the_oracle(dev, Q, T, Tl):
    """T = 16: staged tokens, one mask word.  T = 72: Tl = 64 / 65 on the two sides of a mask-word boundary, a span ending at the last live token.
    T = 200: tokens read from L2, spans in upper words.  Six layers with unequal upstream weights, one image without targets.
    The live launch and the launch on proj_tokens[:, :Tl] run the same arithmetic in the same order (the kernel replaces its token count by the live
    one and keeps every loop), so they are asserted BIT-IDENTICAL -- per-layer losses and both gradients -- which is tighter than the oracle bounds the
    issue allows between them; the dead rows of d proj_tokens are exactly zero."""
    raw_t = _tokens(T)
    ref_tot, ref_dq, ref_dt = _oracle(Q, T, Tl)
    tot_live, losses_live, dq_live, dt_live = _device(Q, raw_t, Tl, Tl, dev)
    tot_cut, losses_cut, dq_cut, dt_cut = _device(Q, raw_t[:, :Tl].contiguous(), Tl, None, dev)
    # against the oracle: the bounds of test_contrastive_align_gradients_vs_oracle
    print(f"Q={Q} T={T} Tl={Tl}: total live {tot_live!r} cut {tot_cut!r} oracle {ref_tot!r}")
    for tot in (tot_live, tot_cut):
        assert abs(tot - ref_tot) <= 1e-4 * abs(ref_tot), (tot, ref_tot)
    for got, ref, name in [(dq_live, ref_dq, "d proj_queries"), (dt_live[:, :Tl], ref_dt, "d proj_tokens")]:
        err, scale = float((got.cpu() - ref).abs().max()), float(ref.abs().max())
        print(f"  {name}: max err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-3 * scale + 1e-7, f"{name}: max err {err} (scale {scale})"
    # against the truncated call
    assert torch.equal(losses_live, losses_cut), (losses_live, losses_cut)
    assert torch.equal(dq_live, dq_cut), float((dq_live - dq_cut).abs().max())
    assert torch.equal(dt_live[:, :Tl], dt_cut), float((dt_live[:, :Tl] - dt_cut).abs().max())
    assert torch.isfinite(dt_live).all() and not dt_live[:, Tl:].any()
    if Tl == T:          # every column live: the new entry points against the old ones on the same [B, T, D] tokens
        assert T == raw_t.shape[1] and torch.equal(dt_live, dt_cut)


@pytest.mark.parametrize("T,Tl", [(16, 7), (72, 65), (200, 130)])
def test_dead_rows_are_written_not_left_as_found(dev, T, Tl):
    """The launcher itself, with every buffer the kernels write prefilled with large finite garbage -- d proj_queries, the dead rows of d proj_tokens
    (its live rows are += : the caller zeroes them), the whole per-layer workspace -- and garbage in the padded rows of proj_tokens: the dead rows of
    d proj_tokens and of the workspace come out as exact zeros, everything else as from the truncated launch on clean buffers."""
    from toist_amd import kernels as k
    Q = 20
    match, _, raw_q = _setup(Q)
    pq = torch.nn.functional.normalize(raw_q, dim=-1).to(dev)
    pt_cut = torch.nn.functional.normalize(_tokens(T)[:, :Tl], dim=-1).to(dev).contiguous()
    pt = torch.full((B, T, D), GARBAGE, device=dev)
    pt[:, :Tl] = pt_cut
    tok_mask, nb = _tok_mask(Tl, dev), torch.tensor([float(sum(SIZES))], device=dev)
    up = torch.tensor(W, device=dev)
    word = torch.tensor([Tl], dtype=torch.int32, device=dev)
    args = (tok_mask, match.tgt_off_dev, match.match_off_dev, match.src, match.tgt, nb, 0.07)

    losses = torch.zeros(L, device=dev)
    k.contrastive_fwd(pq, pt, *args, losses, live_tokens=word)
    losses_cut = torch.zeros(L, device=dev)
    k.contrastive_fwd(pq, pt_cut, *args, losses_cut)
    assert torch.isfinite(losses).all() and torch.equal(losses, losses_cut)

    dpq, dpt, ws = torch.full_like(pq, GARBAGE), torch.full_like(pt, GARBAGE), torch.full((L * B * T * D,), GARBAGE, device=dev)
    dpt[:, :Tl] = 0
    k.contrastive_bwd(pq, pt, *args, up, dpq, dpt, live_tokens=word, workspace=ws)
    dpq_cut, dpt_cut = torch.empty_like(pq), torch.zeros_like(pt_cut)
    k.contrastive_bwd(pq, pt_cut, *args, up, dpq_cut, dpt_cut)
    assert torch.equal(dpq, dpq_cut) and torch.equal(dpt[:, :Tl], dpt_cut)
    assert not dpt[:, Tl:].any()
    ws = ws.view(L, B, T, D)
    assert torch.isfinite(ws).all() and not ws[:, :, Tl:].any() and bool(ws[:, :, :Tl].any())
    # a word beyond the bucket is clamped to it; a word below zero leaves no live column (nothing to align: zero loss, zero gradients)
    pt_all = torch.nn.functional.normalize(_tokens(T), dim=-1).to(dev)
    over, full = torch.zeros(L, device=dev), torch.zeros(L, device=dev)
    k.contrastive_fwd(pq, pt_all, *args, over, live_tokens=torch.tensor([T + 1000], dtype=torch.int32, device=dev))
    k.contrastive_fwd(pq, pt_all, *args, full)
    assert torch.equal(over, full)
    none = torch.full((L,), 5.0, device=dev)
    k.contrastive_fwd(pq, pt, *args, none, live_tokens=torch.tensor([-3], dtype=torch.int32, device=dev))
    assert bool((none == 5.0).all())
