"""Task sweep on the device: toist_sweep_assemble against index_select + cat (bit for bit), the three sweep stages of MDETR against the per-pair path
(bit for bit where every launch sees the same shapes) and against the fp32 oracle, harness.evaluate_sweep's chunking, keying and prototype choice.
(The file sorts behind every other GPU test file on purpose: DESIGN 8 item 6.)"""
import copy
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------------- the kernel
def _inputs(B, T, HW, L, D, dev, seed=0, guard=0):
    """Random sweep inputs.  guard: that many extra images / captions of random data in FRONT of and BEHIND the ones handed to the kernel, in the same
    allocation: an index one past either end still reads valid memory (and gives wrong values, not a fault)."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda n, rows: torch.randn(n + 2 * guard, rows, D, generator=g).to(BF16).to(dev)
    pad = lambda n, rows: (torch.rand(n + 2 * guard, rows, generator=g) < 0.3).to(dev)
    cut = lambda t, n: t[guard:guard + n]
    return (cut(mk(B, HW), B), cut(mk(B, HW), B), cut(pad(B, HW), B), cut(mk(T, L), T), cut(pad(T, L), T))


def _reference(img_tok, img_pos, img_pad, txt_tok, txt_pad, pi, pc):
    pi, pc = pi.long(), pc.long()
    tokens = torch.cat([img_tok.index_select(0, pi), txt_tok.index_select(0, pc)], dim=1)
    pos = torch.cat([img_pos.index_select(0, pi), torch.zeros(pi.numel(), txt_tok.shape[1], img_tok.shape[2], dtype=BF16, device=img_tok.device)], dim=1)
    pad = torch.cat([img_pad.index_select(0, pi), txt_pad.index_select(0, pc)], dim=1).view(torch.uint8)
    return tokens, pos, pad


def _poisoned(P, S, D, dev):
    """Output buffers full of NaN bit patterns (bf16 0x7FC1, bytes 0xFF): whatever the launch leaves unwritten shows."""
    nan = lambda: torch.full((P, S, D), 0x7FC1, dtype=torch.int16, device=dev).view(BF16)
    return nan(), nan(), torch.full((P, S), 0xFF, dtype=torch.uint8, device=dev)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == BF16 else torch.equal(a, b)


SHAPES = {
    "one": (1, 1, 1, 1, 1, 8),
    "odd": (3, 5, 7, 35, 7, 256),
    "product": (2, 14, 28, 400, 16, 256),
    "stride": (2, 2, 3000, 3, 2, 8),                # P * S = 15000 rows: more than one pass of the grid (1024 workgroups x 8 rows)
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_assemble_is_a_bit_exact_copy(dev, name):
    from toist_amd import kernels
    from toist_amd.sweep import pair_tables
    B, T, P, HW, L, D = SHAPES[name]
    ins = _inputs(B, T, HW, L, D, dev, seed=len(name))
    if name == "odd":
        pairs = [(2, 4), (0, 0), (2, 4), (0, 3), (2, 1), (0, 2), (2, 0)]          # a repeated pair; image 1 is not used
    elif name == "stride":
        g = torch.Generator().manual_seed(3)
        pairs = list(zip(torch.randint(0, B, (P,), generator=g).tolist(), torch.randint(0, T, (P,), generator=g).tolist()))
    else:
        pairs = None
    pi, pc, live = pair_tables(B, T, pairs)
    assert live == P
    pi, pc = pi.to(dev), pc.to(dev)
    out = kernels.sweep_assemble(*ins, pi, pc, out=_poisoned(P, HW + L, D, dev))
    want = _reference(*ins, pi, pc)
    for got, ref, what in zip(out, want, ("tokens", "pos", "key_pad")):
        assert got.shape == ref.shape and _bits_equal(got, ref), (name, what)
    assert not bool(out[1][:, HW:].view(torch.int16).any())                        # the caption rows of pos are zeros, all of them written
    fresh = kernels.sweep_assemble(*ins, pi, pc)                                    # buffers of the launcher's own
    assert all(_bits_equal(a, b) for a, b in zip(fresh, want))


@pytest.mark.parametrize("table,value", [("image", "past"), ("image", -1), ("caption", "past"), ("caption", -1)])
def test_a_bad_table_entry_is_never_an_index(dev, table, value):
    """pair 2 names image B (or caption T, or -1): the neighbouring image exists in memory (the inputs are slices of a larger allocation), so a launch
    without the guard reads it and fails here BY VALUE.  The guarded launch zeroes the pair, reports 3 and leaves every other pair right."""
    from toist_amd import kernels
    B, T, P, HW, L, D = 3, 4, 6, 9, 5, 64
    ins = _inputs(B, T, HW, L, D, dev, seed=11, guard=1)
    good_i, good_c = [0, 1, 2, 2, 1, 0], [3, 2, 1, 0, 1, 2]
    bad_i, bad_c = list(good_i), list(good_c)
    (bad_i if table == "image" else bad_c)[2] = value if value != "past" else (B if table == "image" else T)
    as_dev = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    assert kernels.sweep_check(raise_on_failure=False) == 0
    out = kernels.sweep_assemble(*ins, as_dev(bad_i), as_dev(bad_c), out=_poisoned(P, HW + L, D, dev), check=False)
    assert int(kernels.sweep_status(dev).item()) == 3
    want = _reference(*ins, as_dev(good_i), as_dev(good_c))
    keep = torch.tensor([0, 1, 3, 4, 5], device=dev)
    for got, ref, what in zip(out, want, ("tokens", "pos", "key_pad")):
        assert not bool(got[2].view(torch.int16 if got.dtype == BF16 else torch.uint8).any()), what        # pair 2: zeros, padding bytes included
        assert _bits_equal(got[keep], ref[keep]), what
    with pytest.raises(ValueError, match="pair 2"):
        kernels.sweep_check()
    assert kernels.sweep_check(raise_on_failure=False) == 0                          # read and cleared
    with pytest.raises(ValueError, match="pair 2"):                                  # the launcher reads the word itself unless told not to
        kernels.sweep_assemble(*ins, as_dev(bad_i), as_dev(bad_c))
    assert int(kernels.sweep_status(dev).item()) == 0


def test_launcher_refuses_bad_shapes(dev):
    from toist_amd import kernels
    ins = list(_inputs(2, 2, 4, 3, 16, dev))
    pi = torch.zeros(3, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        kernels.sweep_assemble(ins[0], ins[1][:, :3], *ins[2:], pi, pi)
    with pytest.raises(ValueError):
        kernels.sweep_assemble(*ins, pi, pi[:2])
    with pytest.raises(TypeError):
        kernels.sweep_assemble(*ins, pi.long(), pi.long())
    odd = [t[..., :12].contiguous() if t.dtype == BF16 else t for t in ins]           # D = 12: not a multiple of 8
    with pytest.raises(RuntimeError, match="multiple of 8"):
        kernels.sweep_assemble(*odd, pi, pi)


# ------------------------------------------------------------------------------------------------------------------------- the model
def _tune_bn(model):
    """non-trivial FrozenBN statistics, damped so that 33 residual blocks keep the activations in range (as tests/test_gpu_model.py does)"""
    g = torch.Generator().manual_seed(1)
    for n, b in model.named_buffers():
        if n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
        elif n.endswith("running_mean"):
            b.copy_(torch.randn(b.shape, generator=g) * 0.1)
        elif n.endswith(("bn1.weight", "bn2.weight", "bn3.weight", "downsample.1.weight")):
            b.copy_(torch.rand(b.shape, generator=g) * 0.4 + 0.8)
        elif "bn" in n and n.endswith(".bias") or n.endswith("downsample.1.bias"):
            b.copy_(torch.randn(b.shape, generator=g) * 0.05)
    for n, b in model.named_buffers():
        if n.endswith("bn3.weight"):
            b.mul_(0.3)


@pytest.fixture(scope="module")
def small(dev):
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cuda", enc_layers=1, dec_layers=2, num_queries=20))[0]
    _tune_bn(model)
    sd = {k_: v.detach().clone().float() for k_, v in model.state_dict().items()}
    return model.to(dev).eval(), sd


H, W, TOKENS = 160, 192, 16
PAIRS = [(1, 2), (0, 0), (1, 2), (0, 1), (1, 0)]              # B = 2, T = 3: a repeated pair, every image and caption used


def _batch(n_images, n_captions, dev, seed=5):
    """n_images images of H x W (image 1 padded on the right) and n_captions tokenized captions (caption 1 two tokens shorter)"""
    from toist_amd import harness
    samples, _, _, _ = harness.synthetic_batch(n_images, H, W, tokens=TOKENS, seed=seed, max_targets=0)
    _, tok, _, _ = harness.synthetic_batch(n_captions, 32, 32, tokens=TOKENS, seed=seed + 1, max_targets=0)
    if n_images > 1:
        samples.tensors[1, :, :, W - 40:] = 0
        samples.mask[1, :, W - 40:] = True
    if n_captions > 1:
        tok["input_ids"][1, -3], tok["input_ids"][1, -2:] = 2, 1
        tok["attention_mask"][1, -2:] = 0
    return samples, tok


def _repeat(samples, tok, pairs):
    """the batch the reference's loader would build for `pairs`: one sample per (image, caption)"""
    from toist_amd.misc import NestedTensor
    from toist_amd.transformer import TokenizedText
    pi, pc = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    return (NestedTensor(samples.tensors[pi].contiguous(), samples.mask[pi].contiguous()),
            TokenizedText({"input_ids": tok["input_ids"][pc].contiguous(), "attention_mask": tok["attention_mask"][pc].contiguous()}))


def _compare_outputs(a, b):
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
    assert len(a["aux_outputs"]) == len(b["aux_outputs"]) > 0
    for x, y in zip(a["aux_outputs"], b["aux_outputs"]):
        assert torch.equal(x["pred_logits"], y["pred_logits"]) and torch.equal(x["pred_boxes"], y["pred_boxes"])


def test_identity_sweep_equals_the_forward_bit_for_bit(dev, small):
    """P = B = T, pair p = (p, p): every launch of the sweep sees the shapes and the bits of model(...)'s, so the outputs are EQUAL."""
    model, _ = small
    samples, tok = _batch(2, 2, dev)
    samples, tok = samples.to(dev), tok.to(dev)
    with torch.no_grad():
        mc = model(samples, tok, encode_and_save=True)
        out = model(samples, tok, encode_and_save=False, memory_cache=mc)
        mc_s = model.encode_sweep(samples, tok, pairs=[(0, 0), (1, 1)])
        out_s = model.decode(mc_s)
    torch.cuda.synchronize()
    assert torch.equal(mc_s["_native"]["memory"], mc["_native"]["memory"])
    assert torch.equal(mc_s["_native"]["pos"], mc["_native"]["pos"]) and torch.equal(mc_s["mask"], mc["mask"])
    _compare_outputs(out_s, out)
    assert torch.equal(mc_s["img_memory"], mc["img_memory"]) and torch.equal(mc_s["text_memory_resized"], mc["text_memory_resized"])
    assert torch.equal(mc_s["text_attention_mask"], mc["text_attention_mask"]) and torch.equal(mc_s["tokenized"]["input_ids"], tok["input_ids"])


def test_sweep_pairs_equals_the_stages_composed_by_hand(dev, small):
    """B = 2, T = 3, 5 pairs: the kernel inside the model against index_select / cat in torch feeding encode_native."""
    from toist_amd.transformer import EncodedText, TokenizedText
    model, _ = small
    samples, tok = _batch(2, 3, dev)
    pi = torch.tensor([p[0] for p in PAIRS], device=dev)
    pc = torch.tensor([p[1] for p in PAIRS], device=dev)
    with torch.no_grad():
        state = model.sweep_images(samples.to(dev))
        text = model.sweep_text(tok)
        mc = model.sweep_pairs(state, text, [p[0] for p in PAIRS], [p[1] for p in PAIRS])
        out = model.decode(mc)
        T, L = text.key_pad.shape
        d = state.tok.shape[-1]
        by_hand = EncodedText(TokenizedText({"input_ids": text.tokenized["input_ids"][pc], "attention_mask": text.tokenized["attention_mask"][pc]}),
                              text.flat.view(T, L, d).index_select(0, pc).reshape(-1, d), text.key_pad.index_select(0, pc))
        mc_h = model.transformer.encode_native(state.tok.index_select(0, pi), state.pos.index_select(0, pi), state.mask.flatten(1).index_select(0, pi),
                                               model.query_embed.weight, by_hand)
        out_h = model.decode(mc_h)
    assert mc["_native"]["B"] == len(PAIRS) and mc["mask"].shape == (len(PAIRS), state.tok.shape[1] + L)
    assert torch.equal(mc["_native"]["memory"], mc_h["_native"]["memory"]) and torch.equal(mc["_native"]["pos"], mc_h["_native"]["pos"])
    assert torch.equal(mc["mask"], mc_h["mask"]) and torch.equal(mc["text_attention_mask"], mc_h["text_attention_mask"])
    assert torch.equal(mc["tokenized"]["input_ids"], by_hand.tokenized["input_ids"])
    _compare_outputs(out, out_h)
    assert torch.equal(mc["_native"]["memory"].view(5, -1)[0], mc["_native"]["memory"].view(5, -1)[2])        # the repeated pair: the same rows twice


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def test_sweep_against_the_fp32_oracle(dev, small):
    """The 5 pairs through oracle/model_ref.py on the repeated images (fp32, CPU); the bounds are those tests/test_gpu_model.py asserts for the per-pair
    path, which runs here on the same pairs as the control.  Both sets of measured errors are written out as task_sweep_parity.json, beside
    the figures tests/test_gpu_model.py leaves (its _dump_measured)."""
    from oracle import model_ref
    model, sd = small
    samples, tok = _batch(2, 3, dev)
    rep_s, rep_t = _repeat(samples, tok, PAIRS)
    rmc = model_ref.mdetr_encode(sd, rep_s.tensors, rep_s.mask, rep_t["input_ids"], rep_t["attention_mask"])
    rout = model_ref.mdetr_decode(sd, rmc)
    with torch.no_grad():
        mc = model.encode_sweep(samples.to(dev), tok.to(dev), pairs=PAIRS)
        out = model.decode(mc)
        mc_c = model(rep_s.to(dev), rep_t.to(dev), encode_and_save=True)
        out_c = model(rep_s.to(dev), rep_t.to(dev), encode_and_save=False, memory_cache=mc_c)
    measured = {}
    for name, m, o in (("sweep", mc, out), ("per_pair", mc_c, out_c)):
        measured[name] = {"img_memory_rel": _rel(m["img_memory"], rmc["img_memory"]), "logits_rel": _rel(o["pred_logits"], rout["pred_logits"]),
                          "boxes_max_abs": float((o["pred_boxes"].float().cpu() - rout["pred_boxes"]).abs().max()),
                          "mask_equal": bool(torch.equal(m["mask"].cpu(), rmc["mask"]))}
    measured["bounds"] = {"img_memory_rel": 4e-2, "logits_rel": 5e-2, "boxes_max_abs": 2e-2}
    measured["shape"] = {"images": 2, "captions": 3, "pairs": PAIRS, "hw": [H, W], "tokens": TOKENS, "enc_layers": 1, "dec_layers": 2, "queries": 20}
    print("task sweep parity:", json.dumps(measured))
    from test_gpu_model import _dump_measured
    _dump_measured("task_sweep_parity.json", measured)
    for name in ("sweep", "per_pair"):
        e = measured[name]
        assert e["mask_equal"], name
        assert e["img_memory_rel"] < 4e-2 and e["logits_rel"] < 5e-2 and e["boxes_max_abs"] < 2e-2, (name, e)


def _eval_batch(dev, seed=5):
    samples, tok = _batch(2, 3, dev, seed=seed)
    return {"samples": samples.to(dev), "image_ids": [41, 7], "orig_sizes": [(320, 384), (200, 301)]}, tok.to(dev)


TASKS = [("cut", "use something to cut"), ("sit", "sit on something"), ("dig", "dig with something")]


def test_evaluate_sweep_chunks_and_keys(dev, small):
    """Every (image_id, task) exactly once; the chunked loop (max_pairs = 4: groups of 2 captions and 1 caption on both images) against the unchunked
    one within PostProcess's fixture tolerances (the group shapes differ), and against PostProcess on the per-pair path."""
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess
    model, _ = small
    batch, tok = _eval_batch(dev)
    seen, raw = [], []
    whole = harness.evaluate_sweep(model, PostProcess(), [batch], TASKS, dev, tokenized=tok,
                                   observe=lambda mc, out, gi, gc: (seen.append(gi.numel()), raw.append((out, gi.tolist(), gc.tolist()))))
    assert seen == [6]
    chunked = harness.evaluate_sweep(model, PostProcess(), [batch], TASKS, dev, tokenized=tok, max_pairs=4, observe=lambda mc, out, gi, gc: seen.append(gi.numel()))
    assert seen == [6, 4, 2]
    same = harness.evaluate_sweep(model, PostProcess(), [batch], TASKS, dev, tokenized=tok, max_pairs=6)
    want_keys = sorted((i, t[0]) for i in batch["image_ids"] for t in TASKS)
    assert sorted(whole) == want_keys and sorted(chunked) == want_keys and len(whole) == 6
    # the pair stage's own outputs through PostProcess with each pair's image size, keyed by hand: what the loop must have returned
    out, gi, gc = raw[0]
    assert list(zip(gi, gc)) == [(i, t) for i in range(2) for t in range(3)]
    by_hand = PostProcess()(out, torch.tensor([batch["orig_sizes"][i] for i in gi], device=dev))
    worst = {"scores": 0.0, "boxes": 0.0}
    for p, (i, t) in enumerate(zip(gi, gc)):
        key = (batch["image_ids"][i], TASKS[t][0])
        a, b, c, r = whole[key], chunked[key], same[key], by_hand[p]
        assert set(a) == {"scores", "labels", "boxes"} and a["scores"].shape == (20,) and a["boxes"].shape == (20, 4)
        for k_ in ("scores", "labels", "boxes"):
            assert torch.equal(a[k_], c[k_]) and torch.equal(a[k_], r[k_]), (key, k_)          # the same group shapes: equal
        worst = {k_: max(worst[k_], float((a[k_] - b[k_]).abs().max())) for k_ in worst}
        print("chunked against whole", key, worst)
        assert torch.allclose(a["scores"], b["scores"], rtol=1e-5, atol=1e-6) and torch.allclose(a["boxes"], b["boxes"], rtol=0, atol=1e-3), (key, worst)
        assert torch.equal(a["labels"], b["labels"])


def test_evaluate_sweep_explicit_pairs_and_two_batches(dev, small):
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess
    model, _ = small
    b0, tok = _eval_batch(dev)
    b1, _ = _eval_batch(dev, seed=9)
    b1["image_ids"], b1["pairs"] = [3, 4], [(1, 2), (0, 0), (1, 0)]
    got = harness.evaluate_sweep(model, PostProcess(), [b0, b1], TASKS, dev, tokenized=tok, max_pairs=2)
    assert sorted(got) == sorted([(i, t[0]) for i in (41, 7) for t in TASKS] + [(4, "dig"), (3, "cut"), (4, "cut")])
    with pytest.raises(ValueError):
        harness.evaluate_sweep(model, PostProcess(), [b0], TASKS + [("cut", "again")], dev, tokenized=tok)
    with pytest.raises(ValueError):
        harness.evaluate_sweep(model, PostProcess(), [b0], TASKS[:2], dev, tokenized=tok)                  # 2 tasks, 3 tokenized captions


def test_prototype_choice_in_the_sweep(dev):
    """cluster=True: evaluate_sweep(cluster_criterion=...) against ClusterCriterion.infer_choice on the per-pair path from the same memory state -- the
    same caption rows replaced, img_memory_mod within the tolerances of test_gpu_captured_eval.py::test_prototype_choice_inside_the_graph; the banks
    are filled as there.  The three captions hold 'something' at different tokens, so the lookup must follow the pair table."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess
    args = harness.default_args(device="cuda", distillation=True, cluster=True, cluster_memory_size=32, num_queries=20, enc_layers=1, dec_layers=2)
    torch.manual_seed(0)
    model, _, cc, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    cc.to(dev)
    cc.full_label.fill_(1)
    cc.update_count.fill_(100)
    cc.sync_host_state()
    cc_ref = copy.deepcopy(cc)
    cc_ref.sync_host_state()
    tasks = [("cut", "use the something to cut the paper up", "task_3_train.json"), ("sit", "something to sit on comfortably now", "task_7_train.json"),
             ("dig", "dig a deep hole with something big", "task_11_train.json")]
    samples, tok = _batch(2, 3, dev)
    tok["input_ids"][1], tok["attention_mask"][1] = tok["input_ids"][2].flip(0), 1                 # (SyntheticCaptions: 4 characters per token, no padding)
    tok["input_ids"][1, 0], tok["input_ids"][1, -1] = 0, 2
    tok = harness.SyntheticCaptions(dict(tok)).to(dev)
    batch = {"samples": samples.to(dev), "image_ids": [1, 2], "orig_sizes": [(H, W), (H, W)]}
    grabbed = []
    got = harness.evaluate_sweep(model, PostProcess(), [batch], tasks, dev, cluster_criterion=cc, tokenized=tok,
                                 observe=lambda mc, out, gi, gc: grabbed.append((mc["img_memory_mod"].clone(), mc["img_memory"].clone())))
    assert len(got) == 6 and len(grabbed) == 1
    pairs = [(i, t) for i in range(2) for t in range(3)]
    rep_s, rep_t = _repeat(samples, tok, pairs)
    rep_t = harness.SyntheticCaptions(dict(rep_t))
    with torch.no_grad():
        mc = model(rep_s.to(dev), rep_t.to(dev), encode_and_save=True)
        mc = cc_ref.infer_choice(mc, [tasks[t][2] for _, t in pairs], [tasks[t][1] for _, t in pairs])
    mod, mem = grabbed[0]
    print("prototype choice: img_memory max abs diff", float((mem - mc["img_memory"]).abs().max()), "img_memory_mod", float((mod - mc["img_memory_mod"]).abs().max()))
    changed = (mod[-TOKENS:] != mem[-TOKENS:]).any(-1)
    assert bool(changed.any()) and torch.equal(changed, (mc["img_memory_mod"][-TOKENS:] != mc["img_memory"][-TOKENS:]).any(-1))      # the same rows were replaced
    assert len({tuple(changed[:, p].nonzero().flatten().tolist()) for p in range(3)}) == 3               # ... and they differ from caption to caption
    assert torch.allclose(mod, mc["img_memory_mod"], rtol=1e-3, atol=1e-4), float((mod - mc["img_memory_mod"]).abs().max())
    assert torch.allclose(cc.cluster_centers, cc_ref.cluster_centers, rtol=1e-3, atol=1e-4)
    with pytest.raises(ValueError, match="dataset name"):
        harness.evaluate_sweep(model, PostProcess(), [batch], [t[:2] for t in tasks], dev, cluster_criterion=cc, tokenized=tok)


def test_mask_head_models_are_refused():
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cpu", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=4))[0].eval()
    samples, tok, _, _ = harness.synthetic_batch(1, 64, 64, tokens=6, seed=1, max_targets=0)
    with torch.no_grad():
        for call in (lambda: model.encode_sweep(samples, tok), lambda: model.sweep_images(samples), lambda: model.sweep_text(tok),
                     lambda: model.sweep_pairs(None, None, [0], [0])):
            with pytest.raises(NotImplementedError, match="DETRsegm sweeps"):
                call()


def test_gradients_enabled_raise(dev, small):
    model, _ = small
    samples, tok = _batch(2, 2, dev)
    with pytest.raises(RuntimeError, match="inference only"):
        model.encode_sweep(samples.to(dev), tok.to(dev))
    with torch.no_grad():
        state = model.sweep_images(samples.to(dev))
        text = model.sweep_text(tok)
    with pytest.raises(RuntimeError, match="inference only"):
        model.sweep_pairs(state, text, [0], [0])
