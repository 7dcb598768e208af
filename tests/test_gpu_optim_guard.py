"""The optimizer tail's non-finite guard on the GPU (FusedClipAdamWEMA(skip_nonfinite=True): csrc/optim.hip finish_norm_guarded_kernel + the
early return of adamw_ema_kernel) and its wiring into the captured steps.  A skipped step must be NO step: every comparison with the state before
it is torch.equal, i.e. bit for bit.  What an APPLIED step computes is pinned against oracle/optim_ref.py at the tolerances of
tests/test_gpu_optim.py (fp32 arithmetic in another association order: rtol 1e-5)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 8192
SHAPES = [(33, 17), (5,), (1,), (CHUNK * 2 + 5,), (64, 16, 3, 3), (3, 7, 1, 1), (CHUNK,), (257, 129)]
GROUP_OF = [0, 0, 0, 0, 1, 1, 2, 2]
GROUPS = [(3e-3, 1e-4), (1e-4, 0.05), (5e-5, 1e-4)]


@pytest.fixture(autouse=True)
def _leave_process_state_as_found():
    """The model tests below replace the device seed word and advance it, and the captured steps switch the gradient-buffer reuse on: later tests of the
    process (their dropout masks depend on the seed word) must find both as they were."""
    from toist_amd import engine, kernels
    seed, reuse, failed = kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS, kernels.XDEC_FAILED
    yield
    kernels.SEED_DEV, engine.REUSE_GRAD_BUFFERS, kernels.XDEC_FAILED = seed, reuse, failed


class _Set:
    """The tensor set of test_fused_tail_matches_oracle: every path of the kernels (vector and scalar tails, a partly filled chunk, a channels_last
    weight with a folded row scale, an EMA-only tensor, two bf16 compute copies, three groups).  Seeded: two sets start identical."""

    def __init__(self, dev, **opt_kw):
        from toist_amd import engine, optim
        g = torch.Generator().manual_seed(11)
        self.dev = dev
        self.cpu_p = [torch.randn(s, generator=g) for s in SHAPES]
        self.params = [torch.nn.Parameter(p.clone().to(dev)) for p in self.cpu_p]
        self.params[4] = torch.nn.Parameter(self.cpu_p[4].clone().to(dev).contiguous(memory_format=torch.channels_last))
        scale = (torch.rand(64, generator=g) + 0.5).to(dev)
        self.frozen_src = torch.randn(300, generator=g).to(dev)
        self.emas = [p.detach().clone() for p in self.params]
        self.frozen_ema = self.frozen_src.clone()
        self.cache = {}
        fold = lambda m: (m.detach() * scale.view(-1, 1, 1, 1)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        fold.elementwise, fold.row_scale = True, scale
        self.w_conv = engine.compute_copy(self.params[4], fold, self.cache, "conv")
        self.w_lin = engine.compute_copy(self.params[7], engine._cast_bf16, self.cache, "lin")
        groups = [{"params": self.params[:4], "lr": 3e-3}, {"params": self.params[4:6], "lr": 1e-4, "weight_decay": 0.05},
                  {"params": self.params[6:], "lr": 5e-5}]
        self.opt = optim.FusedClipAdamWEMA(groups, lr=1e-4, weight_decay=1e-4, max_norm=0.1,
                                           ema=list(zip(self.params, self.emas)) + [(self.frozen_src, self.frozen_ema)], ema_decay=0.99, **opt_kw)

    def step(self, grads):
        for i, (p, gr) in enumerate(zip(self.params, grads)):
            if gr is None:
                p.grad = None
            else:
                gd = gr.to(self.dev)
                p.grad = gd.contiguous(memory_format=torch.channels_last) if i == 4 else gd
        self.opt.step()

    def tensors(self):
        """every piece of training state the tail writes"""
        return ([p.detach() for p in self.params] + self.opt.exp_avg + self.opt.exp_avg_sq + self.emas + [self.frozen_ema, self.w_conv, self.w_lin])

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in self.tensors()]

    def equals(self, snap):
        torch.cuda.synchronize()
        return [i for i, (a, b) in enumerate(zip(self.tensors(), snap)) if not torch.equal(a, b)]


def _good_grads():
    """g1 .. g5 (one parameter has no gradient in g3, as in the oracle test)"""
    g = torch.Generator().manual_seed(12)
    out = []
    for t in range(1, 6):
        grads = [torch.randn(s, generator=g) * (5.0 if t % 2 else 1e-3) for s in SHAPES]
        if t == 3:
            grads[1] = None
        out.append(grads)
    return out


def _bad(kind, g3):
    bad = [None if x is None else x.clone() for x in g3]
    if kind == "nan_tail":            # the last element of a partly filled chunk: the scalar tail path of sqnorm
        bad[3][2 * CHUNK + 4] = float("nan")
    elif kind == "inf_single":
        bad[2][0] = float("inf")
    else:                             # every gradient finite, the fp32 sum of squares is not
        bad = [None if x is None else torch.full_like(x, 1e20) for x in g3]
    return bad


@pytest.fixture(scope="module")
def oracle_run():
    """oracle/optim_ref.py over g1, g2, g4, g5 from the set's initial values: what a run that never saw the bad step must hold (computed once)"""
    from oracle import optim_ref
    g = torch.Generator().manual_seed(11)
    cpu_p = [torch.randn(s, generator=g) for s in SHAPES]
    torch.rand(64, generator=g)
    frozen = torch.randn(300, generator=g)
    gs = _good_grads()
    p, m, v, e = [x.clone() for x in cpu_p], [torch.zeros_like(x) for x in cpu_p], [torch.zeros_like(x) for x in cpu_p], [x.clone() for x in cpu_p]
    fe = frozen.clone()
    for t, grads in enumerate([gs[0], gs[1], gs[3], gs[4]], start=1):
        p, m, v, e, _ = optim_ref.tail_step(p, grads, m, v, GROUP_OF, GROUPS, t, 0.1, emas=e, ema_decay=0.99)
        fe = optim_ref.ema_update(fe, frozen, 0.99)
    return p, m, v, e, fe


@pytest.mark.parametrize("kind", ["nan_tail", "inf_single", "overflow"])
def test_a_bad_step_is_no_step_bit_for_bit(dev, oracle_run, kind):
    gs = _good_grads()
    bad = _bad(kind, gs[2])
    a, b = _Set(dev, skip_nonfinite=True), _Set(dev)
    assert not a.equals(b.snapshot())
    a.step(gs[0])
    a.step(gs[1])
    snap = a.snapshot()
    before = a.opt.device_state()
    a.step(bad)
    st = a.opt.device_state()
    print(kind, st)
    assert st["skipped"] is True and st["skipped_total"] == 1 and st["veto_mask"] == 1 and st["step"] == 2
    assert st["clip_coef"] == 0.0 and not torch.isfinite(torch.tensor(st["grad_norm"]))
    assert st["bias1"] == before["bias1"] and st["bias2_sqrt"] == before["bias2_sqrt"]
    assert a.equals(snap) == []
    a.step(gs[3])
    st = a.opt.device_state()
    assert st["skipped"] is False and st["skipped_total"] == 1 and st["veto_mask"] == 0 and st["step"] == 3
    a.step(gs[4])
    for grads in (gs[0], gs[1], gs[3], gs[4]):
        b.step(grads)
    assert a.equals(b.snapshot()) == []
    sa, sb = a.opt.device_state(), b.opt.device_state()
    assert sa["step"] == 4 == sb["step"] and sb["skipped"] is False and sb["skipped_total"] == 0
    assert sa["grad_norm"] == sb["grad_norm"] and sa["clip_coef"] == sb["clip_coef"]
    # the expected values come from the oracle, not from the code under test
    ref_p, ref_m, ref_v, ref_e, ref_fe = oracle_run
    for i in range(len(SHAPES)):
        torch.testing.assert_close(b.params[i].detach().cpu(), ref_p[i], rtol=1e-5, atol=1e-7, msg=lambda m: f"p[{i}]: {m}")
        torch.testing.assert_close(b.opt.exp_avg[i].cpu(), ref_m[i], rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(b.opt.exp_avg_sq[i].cpu(), ref_v[i], rtol=1e-5, atol=1e-12)
        torch.testing.assert_close(b.emas[i].cpu(), ref_e[i], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(b.frozen_ema.cpu(), ref_fe, rtol=1e-6, atol=1e-7)


def test_default_is_unchanged_a_bad_step_reaches_the_weights(dev):
    """skip_nonfinite is off by default: the NaN gradient poisons the parameters (as with torch.optim.AdamW) and nothing reports a skip."""
    gs = _good_grads()
    b = _Set(dev)
    assert b.opt.skip_nonfinite is False
    b.step(gs[0])
    b.step(_bad("nan_tail", gs[2]))
    st = b.opt.device_state()
    assert st["skipped"] is False and st["skipped_total"] == 0 and st["step"] == 2
    assert not all(bool(torch.isfinite(p).all()) for p in b.params)
    with pytest.raises(ValueError):
        b.opt.add_veto(torch.zeros(1, dtype=torch.int32, device=dev))


def test_veto_words(dev):
    gs = _good_grads()
    a = _Set(dev, skip_nonfinite=True)
    iw = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(9)]
    fw = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(9)]
    assert a.opt.add_veto(iw[0]) == 2 and a.opt.add_veto(fw[0]) == 1 << 9
    a.step(gs[0])
    snap = a.snapshot()
    assert a.opt.device_state()["step"] == 1
    iw[0].fill_(1)
    a.step(gs[1])                       # finite gradients, vetoed by the integer word
    st = a.opt.device_state()
    assert st["skipped"] and st["veto_mask"] == 2 and st["step"] == 1 and st["skipped_total"] == 1 and a.equals(snap) == []
    iw[0].zero_()
    fw[0].fill_(float("nan"))
    a.step(gs[1])                       # ... by the float word
    st = a.opt.device_state()
    assert st["skipped"] and st["veto_mask"] == 1 << 9 and st["step"] == 1 and st["skipped_total"] == 2 and a.equals(snap) == []
    fw[0].fill_(float("-inf"))
    iw[0].fill_(-7)
    a.step(_bad("inf_single", gs[2]))   # all three reasons at once
    assert a.opt.device_state()["veto_mask"] == 1 | 2 | 1 << 9 and a.equals(snap) == []
    fw[0].fill_(3.0)
    iw[0].zero_()
    a.step(gs[1])                       # both words back to normal: the step applies
    st = a.opt.device_state()
    assert not st["skipped"] and st["veto_mask"] == 0 and st["step"] == 2 and st["skipped_total"] == 3
    assert len(a.equals(snap)) > len(SHAPES)
    # the last slot of each table is read too: word 7 -> bit 8, float word 7 -> bit 16
    for j in range(1, 8):
        assert a.opt.add_veto(iw[j]) == 1 << (1 + j) and a.opt.add_veto(fw[j]) == 1 << (9 + j)
    assert a.opt.add_veto(iw[3]) == 1 << 4          # registering a word twice takes no second slot
    snap = a.snapshot()
    iw[7].fill_(1)
    fw[7].fill_(float("inf"))
    a.step(gs[3])
    assert a.opt.device_state()["veto_mask"] == (1 << 8) | (1 << 16) and a.equals(snap) == []
    with pytest.raises(ValueError):
        a.opt.add_veto(iw[8])
    with pytest.raises(ValueError):
        a.opt.add_veto(fw[8])


def test_deferred_ema_of_a_skipped_step_is_skipped(dev):
    gs = _good_grads()
    a = _Set(dev, skip_nonfinite=True, defer_ema=True)
    assert a.opt.defer_ema
    a.step(gs[0])
    a.opt.ema_update()
    snap = a.snapshot()
    assert not torch.equal(a.emas[0], a.cpu_p[0].to(dev))          # the good step was averaged
    a.step(_bad("nan_tail", gs[2]))
    a.opt.ema_update()
    assert a.opt.device_state()["skipped"] and a.equals(snap) == []
    a.step(gs[1])
    a.opt.ema_update()
    assert a.opt.device_state()["step"] == 2 and len(a.equals(snap)) > len(SHAPES)


# ---- the small model of test_late_group_survives_in_place_zero_grad ------------------------------------------------------------------------
def _small_model(dev):
    import toist_amd
    from toist_amd import harness, kernels
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=1, num_queries=20, dropout=0.0)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    model.transformer.text_encoder.config.hidden_dropout_prob = 0.0
    model.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    return model, criterion, weight_dict


def _state(model, opt, ema=()):
    torch.cuda.synchronize()
    return [p.detach().clone() for p in model.parameters()] + [t.clone() for t in opt.exp_avg + opt.exp_avg_sq] + [t.clone() for t in ema]


def _same(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]


def test_late_group_of_a_skipped_step_is_skipped(dev):
    from toist_amd import harness
    from toist_amd.optim import FusedClipAdamWEMA
    model, criterion, weight_dict = _small_model(dev)
    samples, tok, targets, pmap = harness.synthetic_batch(2, 128, 160, tokens=12, seed=5, device=dev, max_targets=4)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = FusedClipAdamWEMA([{"params": [p for n, p in named if "text_encoder" not in n], "lr": 1e-4},
                             {"params": [p for n, p in named if "text_encoder" in n], "lr": 5e-5, "late": True}], weight_decay=1e-4, max_norm=0.1,
                            skip_nonfinite=True)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    opt.add_veto(word)
    text_w = model.transformer.text_encoder.encoder.layer[0].output.dense.weight
    w0 = text_w.detach().clone()

    def step():
        opt.zero_grad(set_to_none=True)
        mc = model(samples, tok, encode_and_save=True)
        out = model(samples, tok, encode_and_save=False, memory_cache=mc)
        losses = criterion(mc, out, targets, pmap, None)
        sum(losses[k_] * weight_dict[k_] for k_ in losses if k_ in weight_dict).backward()
        opt.step()

    step()
    assert opt._late_pending
    opt.finish()
    snap = _state(model, opt)
    assert not torch.equal(text_w, w0) and opt.device_state()["step"] == 1
    word.fill_(1)
    step()
    assert opt._late_pending                # the late launch of the vetoed step is still issued: it must return without writing
    opt.finish()
    st = opt.device_state()
    assert st["skipped"] and st["veto_mask"] == 2 and st["step"] == 1
    assert _same(_state(model, opt), snap) == []


class _ScaledCE:
    """The criterion, with loss_ce multiplied by a device word of the test: a captured torch multiply, so a replay reads the word's current value --
    a certain way to a non-finite loss (a NaN pixel is not: ReLU epilogues may flush it).  Returns a plain dict: the total is then summed key by key."""

    def __init__(self, inner, word):
        self._inner, self._word = inner, word

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def __call__(self, *a, **kw):
        losses = dict(self._inner(*a, **kw))
        losses["loss_ce"] = losses["loss_ce"] * self._word[0]
        return losses


def _captured(dev):
    from toist_amd import harness
    from toist_amd.optim import FusedClipAdamWEMA
    model, criterion, weight_dict = _small_model(dev)
    src = [v for v in model.state_dict().values() if v.is_floating_point()]
    ema = [v.detach().clone() for v in src]
    opt = FusedClipAdamWEMA([{"params": [p for p in model.parameters() if p.requires_grad], "lr": 1e-4}], weight_decay=1e-4, max_norm=0.1,
                            ema=list(zip(src, ema)), ema_decay=0.99, skip_nonfinite=True)
    word = torch.ones(1, dtype=torch.float32, device=dev)
    cap = harness.CapturedTrainStep(model, _ScaledCE(criterion, word), opt, weight_dict, batch=2, max_targets_per_image=6)
    batch = harness.synthetic_batch(2, 128, 160, tokens=12, seed=5, max_targets=4)
    return model, opt, ema, word, cap, batch


def test_captured_step_skips_a_nonfinite_loss(dev):
    model, opt, ema, word, cap, (samples, tok, targets, pmap) = _captured(dev)
    assert cap.resolve_skipped() is None
    l1 = float(cap.step(samples, tok, targets, pmap).detach())          # eager, then captured
    assert cap.resolve_skipped() is None
    l2 = float(cap.step(samples, tok, targets, pmap).detach())          # replay
    assert cap.resolve_skipped() is None and cap.captures == 1 and cap.replays == 1
    snap = _state(model, opt, ema)
    assert opt.device_state()["step"] == 2
    word.fill_(float("nan"))
    l3 = float(cap.step(samples, tok, targets, pmap).detach())
    assert l3 != l3 or abs(l3) == float("inf"), l3             # precondition: the loss of this replay is not finite
    assert cap.resolve_skipped() == "nonfinite" and cap.skipped == 1
    st = opt.device_state()
    print(l1, l2, l3, st)
    assert st["step"] == 2 and st["veto_mask"] & (1 << 9)      # the step's own loss word is the first float veto
    assert _same(_state(model, opt, ema), snap) == []
    word.fill_(1.0)
    w = model.class_embed.weight.detach().clone()
    l4 = float(cap.step(samples, tok, targets, pmap).detach())
    assert cap.resolve_skipped() is None and cap.skipped == 1
    assert l4 == l4 and abs(l4) != float("inf")
    assert opt.device_state()["step"] == 3 and not torch.equal(model.class_embed.weight, w)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert cap.captures == 1 and cap.replays == 3


def test_captured_step_skips_on_the_decoder_status_word(dev, monkeypatch):
    """The wiring only: the test itself sets the sticky status word, no launch is made to fail."""
    from toist_amd import kernels
    monkeypatch.setattr(kernels, "XDEC_FAILED", False)          # restored afterwards: later tests see the launches as they were
    model, opt, ema, word, cap, (samples, tok, targets, pmap) = _captured(dev)
    ctl = kernels._XDEC_CTL[dev]
    try:
        cap.step(samples, tok, targets, pmap)
        cap.step(samples, tok, targets, pmap)
        assert cap.resolve_skipped() is None and cap.captures == 1
        snap = _state(model, opt, ema)
        step = opt.device_state()["step"]
        ctl[-1] = 1
        loss = float(cap.step(samples, tok, targets, pmap).detach())
        assert loss == loss and abs(loss) != float("inf")      # the loss is finite, yet the step is skipped
        assert cap.resolve_skipped() == "xdec" and cap.skipped == 1
        assert kernels.XDEC_FAILED is True and int(ctl[-1]) == 0
        assert opt.device_state()["step"] == step and _same(_state(model, opt, ema), snap) == []
        w = model.class_embed.weight.detach().clone()
        loss = float(cap.step(samples, tok, targets, pmap).detach())    # the same batch: eagerly on the per-op launches, captured again
        assert cap.captures == 2 and cap.resolve_skipped() is None
        assert loss == loss and abs(loss) != float("inf")
        assert opt.device_state()["step"] == step + 1 and not torch.equal(model.class_embed.weight, w)
    finally:
        ctl[-1] = 0


def test_captured_distill_step_skips_both_models(dev):
    import toist_amd
    from toist_amd import engine, harness, kernels
    from toist_amd.optim import FusedClipAdamWEMA
    args = harness.default_args(device="cuda", distillation=True, cluster=True, nsthl2_loss=True, softkd_loss=True, cluster_memory_size=32,
                                num_queries=20, enc_layers=1, dec_layers=2, dropout=0.0)
    torch.manual_seed(0)
    model, criterion, cc, weight_dict = toist_amd.build_model(args)
    noun, _, _, _ = toist_amd.build_model(args)
    for m_ in (model, noun):
        m_.to(dev).train()
        m_.transformer.text_encoder.config.hidden_dropout_prob = 0.0
        m_.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    cc.to(dev)
    cc.full_label.fill_(1)
    cc.update_count.fill_(100)
    cc.sync_host_state()
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    saved = engine.REUSE_GRAD_BUFFERS
    try:
        opts = [FusedClipAdamWEMA([{"params": [p for p in x.parameters() if p.requires_grad]}], lr=1e-5, weight_decay=1e-4, max_norm=0.1,
                                  skip_nonfinite=True) for x in (model, noun)]
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        for o in opts:
            o.add_veto(word)
        cap = harness.CapturedDistillStep(model, noun, criterion, cc, opts, weight_dict, batch=2, image_hw=(128, 160), tokens=16, max_targets_per_image=6)
        batch = harness.synthetic_distill_batch(2, 128, 160, tokens=16, seed=40, device=dev, max_targets=4)
        for side_t in batch["targets"]:
            for i, t in enumerate(side_t):
                t["dataset_name"] = f"task_{(3, 7)[i]}_train.json"
        cap.step(batch)
        cap.step(batch)
        assert cap.resolve_skipped() is None and cap.captures == 1
        snap = _state(model, opts[0]) + _state(noun, opts[1])
        steps = [o.device_state()["step"] for o in opts]
        word.fill_(1)
        cap.step(batch)
        assert cap.resolve_skipped() == "nonfinite" and cap.skipped == 1
        assert [o.device_state()["step"] for o in opts] == steps
        assert all(o.device_state()["veto_mask"] == 2 for o in opts)
        assert _same(_state(model, opts[0]) + _state(noun, opts[1]), snap) == []
        word.zero_()
        loss = float(cap.step(batch))
        assert cap.resolve_skipped() is None and loss == loss
        assert [o.device_state()["step"] for o in opts] == [s + 1 for s in steps]
        moved = _same(_state(model, opts[0]) + _state(noun, opts[1]), snap)
        assert len(moved) > len(snap) // 2
        assert cap.captures == 1
    finally:
        engine.REUSE_GRAD_BUFFERS = saved
