"""Run-to-run determinism of the training step and of the three gradient reductions that fold in a fixed order instead of adding with
float atomics: the bias column sums of a split-K weight-gradient GEMM (TOIST_GEMM_COLSUM_SLICES + the split-K fold), the text embedding
backward (toist_embed_bwd: the first token that reads a table row adds all its readers in token order) and the contrastive token gradient
(toist_contrastive_bwd_ws: the layers folded in order; its values are pinned to the oracle by
test_gpu_criterion.py::test_contrastive_align_gradients_vs_oracle).  References are float64 torch math on the same bf16 inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows,feat,cols", [(576, 104, 96), (1000, 200, 64), (3328, 256, 256)])
@pytest.mark.parametrize("split", [1, 2, 3, 4, 5, 7, None])
@pytest.mark.parametrize("defer", [False, True])
def test_wgrad_bias_column_sums(dev, rows, feat, cols, split, defer):
    """ops.linear_wgrad(dy, x, bias_out=b): dw += dy^T x and b += sum over rows of dy, split and unsplit, deferred fold or not, output
    widths that are not a multiple of the 64-wide tile (104, 200) and row counts that leave a short last k-tile (1000) or -- 576 rows in
    4 slices of 3 k-tiles -- possibly an empty last slice.  Two runs give the same bits."""
    from toist_amd import kernels, ops
    g = torch.Generator().manual_seed(rows + feat + cols)
    dy = torch.randn(rows, feat, generator=g).to(torch.bfloat16).to(dev)
    x = torch.randn(rows, cols, generator=g).to(torch.bfloat16).to(dev)
    w0 = torch.randn(feat, cols, generator=g).to(dev)
    b0 = torch.randn(feat, generator=g).to(dev)
    ref_w = w0.double() + dy.double().t() @ x.double()
    ref_b = b0.double() + dy.double().sum(0)
    runs = []
    for _ in range(2):
        w, b = w0.clone(), b0.clone()
        ops.linear_wgrad(dy, x, out=w, bias_out=b, split_k=split, defer=defer)
        kernels.flush_reductions()
        torch.cuda.synchronize()
        runs.append((w, b))
    w, b = runs[0]
    tol = 2e-5 * rows      # fp32 sums of `rows` exact bf16 products
    assert torch.allclose(b.double(), ref_b, rtol=1e-5, atol=tol), float((b.double() - ref_b).abs().max())
    assert torch.allclose(w.double(), ref_w, rtol=1e-5, atol=tol), float((w.double() - ref_w).abs().max())
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])


@pytest.mark.parametrize("D", [64, 200, 768])
def test_embed_bwd_against_index_add(dev, D):
    """toist_embed_bwd against index_add on float64: repeated word ids (the <s> / </s> of every caption and a repeated word), the padding
    id in both tables (no gradient into the padding row), D % 64 != 0, accumulation into non-zero table gradients.  Two runs: same bits."""
    from toist_amd import kernels
    pad = 1
    ids = torch.tensor([[0, 17, 17, 33, 2, 1, 1], [0, 40, 17, 2, 1, 1, 1], [0, 5, 6, 7, 8, 9, 2]], dtype=torch.int64)
    mask = ids != pad
    pos = torch.where(mask, torch.cumsum(mask.long(), 1) + pad, torch.full_like(ids, pad))     # RoBERTa's position ids
    ids, pos = ids.reshape(-1), pos.reshape(-1)
    n = ids.numel()
    gen = torch.Generator().manual_seed(D)
    grad = torch.randn(n, D, generator=gen).to(torch.bfloat16)
    word0, pos0, type0 = torch.randn(50, D, generator=gen), torch.randn(12, D, generator=gen), torch.randn(D, generator=gen)
    gd = grad.double()
    keep_w, keep_p = ids != pad, pos != pad
    ref_word = word0.double().index_add(0, ids[keep_w], gd[keep_w])
    ref_pos = pos0.double().index_add(0, pos[keep_p], gd[keep_p])
    ref_type = type0.double() + gd.sum(0)
    runs = []
    for _ in range(2):
        w, p, t = word0.to(dev), pos0.to(dev), type0.to(dev)
        kernels.embed_bwd(grad.to(dev), ids.to(dev), pos.to(dev), pad, w, p, t)
        torch.cuda.synchronize()
        runs.append((w.cpu(), p.cpu(), t.cpu()))
    for got, ref in zip(runs[0], (ref_word, ref_pos, ref_type)):
        assert torch.allclose(got.double(), ref, rtol=1e-6, atol=1e-5), float((got.double() - ref).abs().max())
    assert torch.equal(runs[0][0][pad], word0[pad]) and torch.equal(runs[0][1][pad], pos0[pad])     # padding rows untouched
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


def test_training_step_repeats_bit_for_bit(dev):
    """configs[1]'s step (B = 8, 640 x 640, 16-token captions, the default detection recipe with contrastive_align, dropout on) twice on the
    same weights, batch and dropout seeds: loss, predictions and every parameter gradient are bit-identical."""
    import toist_amd
    from toist_amd import harness, kernels
    from toist_amd.mdetr import weighted_total
    args = harness.default_args(device="cuda", contrastive_align_loss=True)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    criterion.train()
    samples, tok, targets, pmap = harness.synthetic_batch(8, 640, 640, tokens=16, seed=1000, device=dev)
    named = [(n_, p) for n_, p in model.named_parameters() if p.requires_grad]
    old_seed = kernels.SEED_DEV
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    step0 = model.transformer._step        # the per-call dropout seed counter: restarted so both runs draw the same masks
    runs = []
    try:
        for _ in range(2):
            for _, p in named:
                p.grad = None
            model.transformer._step = step0
            kernels.SEED_DEV.fill_(1000003)
            mc = model(samples, tok, encode_and_save=True)
            out = model(samples, tok, encode_and_save=False, memory_cache=mc)
            total = weighted_total(criterion(mc, out, targets, pmap, None), weight_dict)
            total.backward()
            torch.cuda.synchronize()
            runs.append((total.detach().clone(), out["_stacked"]["pred_logits"].detach().clone(), out["_stacked"]["pred_boxes"].detach().clone(),
                         {n_: p.grad.detach().clone() for n_, p in named if p.grad is not None}))
            del mc, out, total
        kernels.xdec_check()
    finally:
        kernels.SEED_DEV = old_seed
    (l0, lg0, bx0, g0), (l1, lg1, bx1, g1) = runs
    # the loss terms are summed over images with float atomics (no gradient reads those sums): the loss may differ in its last bits only
    assert torch.allclose(l0, l1, rtol=1e-6, atol=0) and torch.equal(lg0, lg1) and torch.equal(bx0, bx1)
    assert set(g0) == set(g1) and len(g0) > 400
    differing = [n_ for n_ in g0 if not torch.equal(g0[n_], g1[n_])]
    assert not differing, differing


def test_bench_dump_outputs_repeat(dev, tmp_path):
    """`bench.py --dump-outputs DIR` run twice with the same arguments writes the same arrays, bit for bit (the timed path's last step after
    the warm-up replays: a rounding difference anywhere in the step would have grown by then)."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        lines = [l_ for l_ in r.stdout.splitlines() if l_.startswith('{"metric"')]
        assert r.returncode == 0 and lines, r.stderr[-3000:]
        res = json.loads(lines[-1])
        assert res["steps"] == 2 and res["ms_per_step"] > 0
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert set(dumps[0]) == {"loss.npy", "pred_logits.npy", "pred_boxes.npy", "params_sample.npy"}
    for f, a in dumps[0].items():
        b = dumps[1][f]
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), f
        if f == "loss.npy":      # per-term loss sums still use float atomics (no gradient reads them): rounding only
            assert np.allclose(a, b, rtol=1e-6, atol=0), (a, b)
        else:
            assert np.array_equal(a, b), (f, float(np.abs(a.astype(np.float64) - b).max()))
