"""Shared-image training on the device: toist_sweep_assemble_bwd against a sequential fp32 reference (bit for bit), MDETR.encode_pairs with identity
pairs against MDETR.encode (bit for bit), and with shared images and captions against the fp32 oracle and the per-sample path on the expanded batch.
(The file sorts behind every older GPU test file on purpose: DESIGN 8 item 6.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------------- the kernel
def _reference(d_seq, pi, pc, B, HW, T, L):
    """The definition: per destination an fp32 accumulator, pairs added in ascending order, one rounding to bf16 (host tensors)."""
    P, S, D = d_seq.shape
    d_img, d_txt = torch.zeros(B, HW, D, dtype=torch.float32), torch.zeros(T, L, D, dtype=torch.float32)
    for p in range(P):
        i, t = int(pi[p]), int(pc[p])
        if not (0 <= i < B and 0 <= t < T):
            continue                                       # a bad entry on EITHER side: the pair adds to neither output
        g = d_seq[p].float()
        d_img[i] += g[:HW]
        d_txt[t] += g[HW:]
    return d_img.to(BF16), d_txt.to(BF16)


def _poisoned(shape, dev):
    """bf16 NaN bit patterns (0x7FC1): whatever the launch leaves unwritten shows"""
    return torch.full(shape, 0x7FC1, dtype=torch.int16, device=dev).view(BF16)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int16), b.cpu().view(torch.int16))


def _tables(pi, pc, dev):
    return torch.tensor(pi, dtype=torch.int32, device=dev), torch.tensor(pc, dtype=torch.int32, device=dev)


# case A: B = 3, T = 2, HW = 5, L = 3, P = 7.  Image 1 has no pair; the pair (0, 1) is listed twice; image 0 is named by four pairs, the last of
# them with caption T: that pair, like the ones naming image -1 and image B, adds to neither side
A_IMAGE, A_CAPTION = [0, 0, 2, 0, -1, 3, 0], [0, 1, 1, 1, 0, 1, 2]
A_EXTENTS = (3, 5, 2, 3)                                   # B, HW, T, L


def _case_a(D, seed=0):
    B, HW, T, L = A_EXTENTS
    g = torch.Generator().manual_seed(seed + D)
    return torch.randn(len(A_IMAGE), HW + L, D, generator=g).to(BF16)


@pytest.mark.parametrize("D", [8, 256, 264])               # one active lane; one pass of the 32 lanes; a second pass of the lane loop
def test_assemble_bwd_is_the_sequential_fp32_sum(dev, D):
    from toist_amd import kernels
    B, HW, T, L = A_EXTENTS
    d_seq = _case_a(D)
    want_img, want_txt = _reference(d_seq, A_IMAGE, A_CAPTION, B, HW, T, L)
    assert not bool(want_img[1].view(torch.int16).any()) and bool(want_img[0].view(torch.int16).any())          # image 1: no pair -> zeros
    pi, pc = _tables(A_IMAGE, A_CAPTION, dev)
    out = (_poisoned((B, HW, D), dev), _poisoned((T, L, D), dev))
    d_img, d_txt = kernels.sweep_assemble_bwd(d_seq.to(dev), pi, pc, B, HW, T, L, out=out)
    torch.cuda.synchronize()
    assert d_img is out[0] and d_txt is out[1]
    assert _bits_equal(d_img, want_img) and _bits_equal(d_txt, want_txt)
    fresh = kernels.sweep_assemble_bwd(d_seq.to(dev), pi, pc, B, HW, T, L)                                      # buffers of the launcher's own
    assert _bits_equal(fresh[0], want_img) and _bits_equal(fresh[1], want_txt)


def test_assemble_bwd_without_pairs_writes_zeros(dev):
    from toist_amd import kernels
    B, HW, T, L, D = 3, 5, 2, 3, 256
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    out = (_poisoned((B, HW, D), dev), _poisoned((T, L, D), dev))
    d_img, d_txt = kernels.sweep_assemble_bwd(torch.zeros(0, HW + L, D, dtype=BF16, device=dev), empty, empty, B, HW, T, L, out=out)
    torch.cuda.synchronize()
    assert not bool(d_img.view(torch.int16).any()) and not bool(d_txt.view(torch.int16).any())


@pytest.mark.parametrize("D", [8, 264])
def test_assemble_bwd_skips_a_null_output(dev, D):
    from toist_amd import kernels
    B, HW, T, L = A_EXTENTS
    d_seq = _case_a(D)
    want_img, want_txt = _reference(d_seq, A_IMAGE, A_CAPTION, B, HW, T, L)
    pi, pc = _tables(A_IMAGE, A_CAPTION, dev)
    keep = _poisoned((T, L, D), dev)
    d_img, none = kernels.sweep_assemble_bwd(d_seq.to(dev), pi, pc, B, HW, T, L, want_txt=False, out=(_poisoned((B, HW, D), dev), keep))
    torch.cuda.synchronize()
    assert none is None and _bits_equal(d_img, want_img)
    assert bool((keep.view(torch.int16) == 0x7FC1).all())                         # the skipped half was not touched
    keep = _poisoned((B, HW, D), dev)
    none, d_txt = kernels.sweep_assemble_bwd(d_seq.to(dev), pi, pc, B, HW, T, L, want_img=False, out=(keep, _poisoned((T, L, D), dev)))
    torch.cuda.synchronize()
    assert none is None and _bits_equal(d_txt, want_txt)
    assert bool((keep.view(torch.int16) == 0x7FC1).all())
    assert kernels.sweep_assemble_bwd(d_seq.to(dev), pi, pc, B, HW, T, L, want_img=False, want_txt=False) == (None, None)


def _case_d():
    """HW = L = 1, D = 8, P = 5000 over B = 3, T = 2: sums of ~1700 / 2500 terms per element, a pair table far larger than anything a workgroup
    could stage.  Magnitudes 2^-8 .. 2^8 with random 8-bit mantissas and signs; pair p + 2496 (a multiple of 6: same image, same caption) carries
    the NEGATED values of pair p < 2496, so the exact sum of a destination is that of its last few pairs (of magnitude 2^-8) while the running fp32 sum climbs to
    ~2^13 and back: what the small terms lose on the way depends on the order of the additions, and it is far more than one bf16 ulp of the result."""
    P, B, T = 5000, 3, 2
    g = torch.Generator().manual_seed(7)
    mag = torch.exp2(torch.randint(-8, 9, (P, 2, 8), generator=g).float()) * (1 + torch.randint(0, 128, (P, 2, 8), generator=g).float() / 128)
    val = mag * (torch.randint(0, 2, (P, 2, 8), generator=g).float() * 2 - 1)
    val[2496:4992] = -val[:2496]
    val[4992:] *= torch.exp2(-8 - val[4992:].abs().log2().floor())               # the eight pairs without a partner: magnitude 2^-8, mantissa kept
    d_seq = val.to(BF16)
    assert torch.equal(d_seq.float(), val)                                        # every value is a bf16 number
    return d_seq, [p % B for p in range(P)], [p % T for p in range(P)], (B, 1, T, 1)


def test_assemble_bwd_adds_in_pair_order_over_a_long_table(dev):
    from toist_amd import kernels
    d_seq, pi, pc, (B, HW, T, L) = _case_d()
    want_img, want_txt = _reference(d_seq, pi, pc, B, HW, T, L)
    # the input makes the order visible: the exact (fp64) sums, rounded once, are NOT what the sequential fp32 sum gives
    exact_img, exact_txt = torch.zeros(B, 1, 8, dtype=torch.float64), torch.zeros(T, 1, 8, dtype=torch.float64)
    exact_img.index_add_(0, torch.tensor(pi), d_seq[:, :1].double())
    exact_txt.index_add_(0, torch.tensor(pc), d_seq[:, 1:].double())
    assert not _bits_equal(exact_img.to(BF16), want_img) and not _bits_equal(exact_txt.to(BF16), want_txt)
    rev_img, _ = _reference(d_seq.flip(0), pi[::-1], pc[::-1], B, HW, T, L)
    assert not _bits_equal(rev_img, want_img)                                     # nor what the descending order gives
    ti, tc = _tables(pi, pc, dev)
    d_img, d_txt = kernels.sweep_assemble_bwd(d_seq.to(dev), ti, tc, B, HW, T, L, out=(_poisoned((B, 1, 8), dev), _poisoned((T, 1, 8), dev)))
    torch.cuda.synchronize()
    assert _bits_equal(d_img, want_img) and _bits_equal(d_txt, want_txt)


def test_assemble_bwd_repeats_bit_for_bit(dev):
    from toist_amd import kernels
    d_seq, pi, pc, (B, HW, T, L) = _case_d()
    ti, tc = _tables(pi, pc, dev)
    on_dev = d_seq.to(dev)
    first = kernels.sweep_assemble_bwd(on_dev, ti, tc, B, HW, T, L)
    second = kernels.sweep_assemble_bwd(on_dev, ti, tc, B, HW, T, L)
    torch.cuda.synchronize()
    assert first[0].data_ptr() != second[0].data_ptr()
    assert _bits_equal(first[0], second[0]) and _bits_equal(first[1], second[1])
    d_a = _case_a(256).to(dev)
    pa, ca = _tables(A_IMAGE, A_CAPTION, dev)
    runs = [kernels.sweep_assemble_bwd(d_a, pa, ca, *A_EXTENTS) for _ in range(2)]
    torch.cuda.synchronize()
    assert _bits_equal(runs[0][0], runs[1][0]) and _bits_equal(runs[0][1], runs[1][1])


def test_assemble_bwd_launcher_refuses_bad_arguments(dev):
    from toist_amd import kernels
    B, HW, T, L = A_EXTENTS
    d_seq = _case_a(16).to(dev)
    pi, pc = _tables(A_IMAGE, A_CAPTION, dev)
    with pytest.raises(TypeError):
        kernels.sweep_assemble_bwd(d_seq.float(), pi, pc, B, HW, T, L)
    with pytest.raises(TypeError):
        kernels.sweep_assemble_bwd(d_seq, pi.long(), pc.long(), B, HW, T, L)
    with pytest.raises(ValueError):
        kernels.sweep_assemble_bwd(d_seq.transpose(0, 1), pi, pc, B, HW, T, L)          # [S, P, D]: neither the shape nor contiguous
    with pytest.raises(ValueError):
        kernels.sweep_assemble_bwd(d_seq[:, :, ::2], pi, pc, B, HW, T, L)               # the right shape for D = 8, not contiguous
    with pytest.raises(ValueError):
        kernels.sweep_assemble_bwd(d_seq, pi, pc, B, HW + 1, T, L)                      # S != HW + L
    with pytest.raises(ValueError):
        kernels.sweep_assemble_bwd(d_seq, pi[:6], pc, B, HW, T, L)
    with pytest.raises(ValueError):
        kernels.sweep_assemble_bwd(d_seq, pi, pc, B, HW, T, L, out=(torch.empty(B, HW, 8, dtype=BF16, device=dev), None))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        kernels.sweep_assemble_bwd(d_seq[:, :, :12].contiguous(), pi, pc, B, HW, T, L)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------- identity pairs
def _small_model(dev, **over):
    """the small detection model of tests/test_gpu_captured_step.py"""
    import toist_amd
    from toist_amd import harness
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=2, num_queries=20, dropout=0.0, contrastive_align_loss=True, **over)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    model.transformer.text_encoder.config.hidden_dropout_prob = 0.0
    model.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    criterion.train()
    return model, criterion, weight_dict


def _to_dev(targets, dev):
    return [{k_: (v.to(dev) if torch.is_tensor(v) else v) for k_, v in t.items()} for t in targets]


def test_identity_pairs_equal_encode_bit_for_bit(dev):
    """One pair per image and caption, p = (p, p): every launch sees the shapes and bits of MDETR.encode's, and the assembly's backward is a copy
    (bf16 -> fp32 -> bf16 of ONE term).  Bounds: what tests/test_gpu_determinism.py::test_training_step_repeats_bit_for_bit gives the existing step
    against itself -- predictions and every parameter gradient equal, the loss (summed over images with float atomics) within rtol 1e-6."""
    from toist_amd import harness, kernels
    from toist_amd.mdetr import weighted_total
    model, criterion, weight_dict = _small_model(dev)
    samples, tok, pi, pc, targets, pmap = harness.synthetic_pair_batch(2, 2, [(0, 0), (1, 1)], height=128, width=160, tokens=12, seed=21, max_targets=4,
                                                                       device=dev)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    old_seed = kernels.SEED_DEV
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    step0 = model.transformer._step
    runs = []
    try:
        for shared in (False, True):
            for _, p in named:
                p.grad = None
            model.transformer._step = step0
            kernels.SEED_DEV.fill_(1000003)
            mc = model.encode_pairs(samples, tok, pi, pc) if shared else model.encode(samples, tok)
            out = model.decode(mc)
            total = weighted_total(criterion(mc, out, targets, pmap, None), weight_dict)
            total.backward()
            torch.cuda.synchronize()
            runs.append((total.detach().clone(), out["_stacked"]["pred_logits"].detach().clone(), out["_stacked"]["pred_boxes"].detach().clone(),
                         {n: p.grad.detach().clone() for n, p in named if p.grad is not None}, mc["_native"]["memory"].detach().clone()))
            if shared:
                assert mc["_native"]["pair_image"].tolist() == [0, 1] and mc["_native"]["pair_caption"].tolist() == [0, 1]
                assert torch.equal(mc["tokenized"]["input_ids"], tok["input_ids"])
            del mc, out, total
        kernels.xdec_check()
    finally:
        kernels.SEED_DEV = old_seed
    (l0, lg0, bx0, g0, m0), (l1, lg1, bx1, g1, m1) = runs
    print("identity pairs: loss", float(l0), float(l1), "gradients", len(g0), len(g1))
    assert torch.equal(m0, m1)
    assert torch.equal(lg0, lg1) and torch.equal(bx0, bx1)
    assert set(g0) == set(g1) and len(g0) > 300
    differing = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not differing, differing
    assert torch.allclose(l0, l1, rtol=1e-6, atol=0), (float(l0), float(l1))


# ------------------------------------------------------------------------------------------------------------------------- shared images and captions
# the project's own constants: tests/test_gpu_model.py (GRAD_COS_MIN, GRAD_RATIO, the loss bounds and the checked tensors of test_criterion_and_gradients)
GRAD_COS_MIN = 0.985
GRAD_RATIO = (0.95, 1.06)
CHECKS = ["class_embed.weight", "bbox_embed.layers.2.weight", "bbox_embed.layers.0.bias", "query_embed.weight",
          "transformer.decoder.layers.5.linear2.weight", "transformer.decoder.layers.0.cross_attn_image.in_proj_weight",
          "transformer.decoder.norm.weight", "transformer.encoder.layers.5.self_attn.in_proj_weight",
          "transformer.decoder.layers.3.self_attn.in_proj_weight", "transformer.decoder.layers.0.self_attn.in_proj_bias",
          "transformer.decoder.layers.5.cross_attn_image.in_proj_bias", "transformer.decoder.layers.2.cross_attn_image.out_proj.weight",
          "transformer.decoder.layers.1.norm1.weight", "transformer.decoder.layers.4.norm4.bias", "transformer.encoder.layers.2.self_attn.in_proj_bias",
          "transformer.encoder.layers.0.linear1.weight", "transformer.encoder.layers.0.norm1.bias", "input_proj.weight",
          "transformer.resizer.fc.weight", "transformer.text_encoder.encoder.layer.11.output.dense.weight",
          "transformer.text_encoder.encoder.layer.0.attention.self.query.weight",
          "transformer.text_encoder.embeddings.position_embeddings.weight", "backbone.0.body.layer4.2.conv3.weight",
          "backbone.0.body.layer4.0.downsample.0.weight", "backbone.0.body.layer3.10.conv2.weight", "backbone.0.body.layer2.0.conv1.weight"]
SHARED_PAIRS = [(0, 0), (0, 1), (1, 1)]                    # image 0 and caption 1 are each shared by two pairs


def _oracle_model(dev):
    """the model and the perturbed FrozenBN statistics of tests/test_gpu_model.py::setup"""
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(harness.default_args(device="cuda"))
    g = torch.Generator().manual_seed(1)
    for n, b in model.named_buffers():
        if n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
        elif n.endswith("running_mean"):
            b.copy_(torch.randn(b.shape, generator=g) * 0.1)
        elif n.endswith("bn1.weight") or n.endswith("bn2.weight") or n.endswith("bn3.weight") or n.endswith("downsample.1.weight"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.4 + 0.8)
        elif "bn" in n and n.endswith(".bias") or n.endswith("downsample.1.bias"):
            b.copy_(torch.randn(b.shape, generator=g) * 0.05)
    for n, b in model.named_buffers():
        if n.endswith("bn3.weight"):
            b.mul_(0.3)
    sd = {k_: v.detach().clone().float() for k_, v in model.state_dict().items()}
    return model.to(dev).eval(), criterion, weight_dict, sd


def test_shared_pairs_against_the_oracle_and_the_expanded_batch(dev):
    """P = 3 problems on 2 images and 2 captions, three ways: (a) encode_pairs, (b) encode on harness.expand_pairs, (c) the fp32 oracle with autograd on
    the expanded batch.  (a) is held to what tests/test_gpu_model.py::test_criterion_and_gradients asks of the existing path, and may not be worse
    than (b) by more than half of (b)'s own distance from the cosine bound.
    Measured (MI355X): see profiles/pair_train.json "gradient_parity"."""
    from oracle import model_ref
    from toist_amd import harness, kernels
    model, criterion, weight_dict, sd = _oracle_model(dev)
    batch = harness.synthetic_pair_batch(2, 2, SHARED_PAIRS, height=128, width=160, tokens=16, seed=6, max_targets=4)
    samples, tok, pi, pc, targets, pmap = batch
    ex_samples, ex_tok, _, _ = harness.expand_pairs(*batch)
    t_dev, params = _to_dev(targets, dev), dict(model.named_parameters())

    def run(shared):
        model.zero_grad(set_to_none=True)
        if shared:
            mc = model.encode_pairs(samples.to(dev), tok.to(dev), pi, pc)
        else:
            mc = model(ex_samples.to(dev), ex_tok.to(dev), encode_and_save=True)
        out = model.decode(mc)
        losses = criterion(mc, out, t_dev, pmap.to(dev), None)
        total = sum(losses[k_] * weight_dict[k_] for k_ in losses if k_ in weight_dict)
        total.backward()
        torch.cuda.synchronize()
        grads = {n: (None if params[n].grad is None else params[n].grad.detach().float().cpu().clone()) for n in CHECKS}
        return out, losses, float(total), grads, criterion.last_match

    out_b, losses_b, total_b, grads_b, _ = run(False)
    out_a, losses_a, total_a, grads_a, match = run(True)
    kernels.xdec_check()
    assert grads_a["backbone.0.body.layer4.2.conv3.weight"] is not None
    assert grads_a["transformer.text_encoder.encoder.layer.11.output.dense.weight"] is not None

    # --- the oracle on (a)'s own outputs: matcher indices bit-identical, every loss equal ---
    lay = out_a["_stacked"]
    L = lay["pred_logits"].shape[0]
    ref_out = {"pred_logits": lay["pred_logits"][-1].detach().cpu().float(), "pred_boxes": lay["pred_boxes"][-1].detach().cpu().float(),
               "aux_outputs": [{"pred_logits": lay["pred_logits"][i].detach().cpu().float(), "pred_boxes": lay["pred_boxes"][i].detach().cpu().float()}
                               for i in range(L - 1)]}
    ref_losses, ref_idx = model_ref.set_criterion(ref_out, targets, pmap, return_indices=True)
    for pos, l in enumerate([L - 1] + list(range(L - 1))):
        for (gi, gj), (ri, rj) in zip(match.to_list(l), ref_idx[pos]):
            assert torch.equal(gi, ri) and torch.equal(gj, rj), f"layer {l}: assignment differs"
    assert set(ref_losses) == set(losses_a), (sorted(ref_losses), sorted(losses_a))
    for k_ in ref_losses:
        a, b = float(losses_a[k_]), float(ref_losses[k_])
        print(f"loss {k_}: shared {a:.6f} oracle on its outputs {b:.6f}")
        assert abs(a - b) <= 2e-3 + 2e-3 * abs(b), f"{k_}: {a} vs {b}"

    # --- (c): fp32 autograd through the oracle on the expanded batch ---
    sdr = {k_: v.clone().requires_grad_(v.is_floating_point() and "running" not in k_ and ".bn" not in k_ and "downsample.1" not in k_)
           for k_, v in sd.items()}
    rmc = model_ref.mdetr_encode(sdr, ex_samples.tensors, ex_samples.mask, ex_tok["input_ids"], ex_tok["attention_mask"])
    rl = model_ref.set_criterion(model_ref.mdetr_decode(sdr, rmc), targets, pmap)
    rtotal = sum(rl[k_] * weight_dict[k_] for k_ in rl if k_ in weight_dict)
    rtotal.backward()
    print(f"total: shared {total_a:.6f} expanded {total_b:.6f} oracle {float(rtotal):.6f}")
    figures = {"shared": {}, "expanded": {}}
    for name, grads in (("shared", grads_a), ("expanded", grads_b)):
        for n in CHECKS:
            g, r = grads[n], sdr[n].grad
            assert g is not None, f"no grad for {n} ({name})"
            cos = float(torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0))
            figures[name][n] = (round(cos, 4), round(float(g.norm() / (r.norm() + 1e-20)), 3))
    worst = {name: {"min_cos": min(v[0] for v in f.values()), "min_ratio": min(v[1] for v in f.values()), "max_ratio": max(v[1] for v in f.values())}
             for name, f in figures.items()}
    print("gradient parity, worst cases:", worst)
    from test_gpu_model import _dump_measured              # the suite's writer of measured figures: same directory as model_grad_parity.json
    _dump_measured("pair_train_grad_parity.json", {"pairs": SHARED_PAIRS, "total": {"shared": total_a, "expanded": total_b, "oracle": float(rtotal)},
                                                   "worst": worst, **figures})
    assert abs(total_a - float(rtotal)) < 0.05 * abs(float(rtotal)) + 0.05, (total_a, float(rtotal))
    bad = {n: v for n, v in figures["shared"].items() if v[0] < GRAD_COS_MIN or not (GRAD_RATIO[0] < v[1] < GRAD_RATIO[1])}
    assert not bad, f"gradient mismatch (cos, norm ratio): {bad}\nall: {figures['shared']}"
    # a sharing bug that drops part of an image's gradient can pass an absolute bound on some tensor; it cannot stay this close to the expanded batch
    behind = {n: (figures["shared"][n][0], figures["expanded"][n][0]) for n in CHECKS
              if figures["shared"][n][0] < figures["expanded"][n][0] - (figures["expanded"][n][0] - GRAD_COS_MIN) / 2}
    assert not behind, f"(cos shared, cos expanded): {behind}"
    frozen = params["backbone.0.body.layer1.0.conv1.weight"]
    assert frozen.grad is None and not frozen.requires_grad


def test_frozen_text_side_runs_with_a_null_caption_gradient(dev, monkeypatch):
    """freeze_text_encoder=True freezes RoBERTa; the resizer behind it still trains, so the caption tokens still want their gradient.  With the resizer
    frozen as well nothing on the text side requires one, and the assembly's backward runs with a null d_txt."""
    from toist_amd import harness, kernels
    from toist_amd.mdetr import weighted_total
    model, criterion, weight_dict = _small_model(dev, freeze_text_encoder=True)
    assert not any(p.requires_grad for p in model.transformer.text_encoder.parameters())
    batch = harness.synthetic_pair_batch(2, 2, SHARED_PAIRS, height=128, width=160, tokens=12, seed=8, max_targets=3, device=dev)
    calls, real = [], kernels.sweep_assemble_bwd

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append((out[0] is not None, out[1] is not None))
        return out

    monkeypatch.setattr(kernels, "sweep_assemble_bwd", spy)
    for freeze_resizer, want in ((True, (True, False)), (False, (True, True))):
        for p in model.transformer.resizer.parameters():
            p.requires_grad_(not freeze_resizer)
        model.zero_grad(set_to_none=True)
        del calls[:]
        losses, _ = harness.pair_train_losses(model, criterion, batch)
        total = weighted_total(losses, weight_dict)
        total.backward()
        torch.cuda.synchronize()
        assert calls == [want], calls
        assert bool(torch.isfinite(total))
        assert model.input_proj.weight.grad is not None and dict(model.named_parameters())["backbone.0.body.layer4.2.conv3.weight"].grad is not None
        assert all(p.grad is None for p in model.transformer.text_encoder.parameters())
        assert (model.transformer.resizer.fc.weight.grad is None) == freeze_resizer
    kernels.xdec_check()
