"""Host logic of the bucketed CapturedDistillStep and of the live-token word of matcher.LiveStaticTargets, on CPU tensors: the bucket key of a pair batch,
the errors that are raised before anything touches a device, the arena layout with the word, caption tables of a bucket longer than the caption."""
import pytest
import torch


def _step(batch=2, pad_hw=64, pad_tokens=8):
    """What bucket_of_pair reads (the constructor needs a GPU)."""
    from toist_amd import captured
    cap = captured.CapturedDistillStep.__new__(captured.CapturedDistillStep)
    cap.B, cap.pad_hw, cap.pad_tokens, cap.bucketed = batch, pad_hw, pad_tokens, True
    return cap


def test_bucket_key_of_a_pair_batch():
    from toist_amd import harness
    for hw, ln, ls, pad_hw, pad_tokens, want in (((120, 150), 12, 10, 64, 8, (128, 192, 16)), ((128, 160), 9, 11, 64, 8, (128, 192, 16)),
                                                 ((128, 160), 16, 17, 32, 8, (128, 160, 24)), ((100, 130), 16, 14, 64, 8, (128, 192, 16)),
                                                 ((37, 41), 9, 12, 1, 1, (37, 41, 12))):
        batch = harness.synthetic_distill_batch(2, *hw, tokens=ln, tokens_pronoun=ls, seed=1, max_targets=3)
        assert [int(t["input_ids"].shape[1]) for t in batch["tokenized"]] == [ln, ls]
        assert _step(pad_hw=pad_hw, pad_tokens=pad_tokens).bucket_of_pair(batch) == want      # the LONGER caption of the two sides decides Lp


def test_errors_before_any_device_work():
    from toist_amd import captured, harness
    from toist_amd.misc import NestedTensor
    for kw in ({"image_hw": (128, 160)}, {"tokens": 16}):
        with pytest.raises(ValueError, match="image_hw AND tokens"):
            captured.CapturedDistillStep(None, None, None, None, [], {}, batch=2, **kw)
    batch = harness.synthetic_distill_batch(2, 96, 128, tokens=12, tokens_pronoun=10, seed=2, max_targets=3)
    other = dict(batch, samples=[batch["samples"][0], NestedTensor(torch.zeros(2, 3, 96, 160), torch.zeros(2, 96, 160, dtype=torch.bool))])
    with pytest.raises(ValueError, match="same images"):
        _step().bucket_of_pair(other)
    with pytest.raises(ValueError, match="batches of 2 pairs"):
        _step().bucket_of_pair(harness.synthetic_distill_batch(3, 96, 128, tokens=12, tokens_pronoun=10, seed=2, max_targets=3))
    assert _step(batch=3).bucket_of_pair(harness.synthetic_distill_batch(3, 96, 128, tokens=12, tokens_pronoun=10, seed=2, max_targets=3)) == (128, 128, 16)


def test_live_static_targets_pack_carries_the_word_behind_the_seven_views():
    from toist_amd.matcher import LiveStaticTargets, StaticTargets
    B, per, K = 2, 3, 8
    views, total0 = StaticTargets.arena_views(B, B * per, K)
    total = total0 + 16

    host_only = lambda cls: cls(B, per, 10, K, device="cpu")         # (a host-only instance: ordinary buffers, no GPU runtime)
    targets = [{"boxes": torch.rand(2, 4)}, {"boxes": torch.rand(1, 4)}]
    pm, masks = torch.rand(3, K), torch.tensor([[6, 0, 0, 0], [1, 0, 0, 0], [1 << 40, 0, 0, 0]], dtype=torch.int64)
    st = host_only(LiveStaticTargets)
    own = st._stage.open()
    assert own.numel() == total
    host, sizes = st.pack(targets, pm, masks, out=own, live_tokens=11)
    word = st._live_word(host)
    assert sizes == [2, 1] and (word.dtype, word.tolist()) == (torch.int32, [11]) and word.data_ptr() == host.data_ptr() + total0
    ref, _ = host_only(StaticTargets).pack(targets, pm, masks, out=torch.zeros(total0, dtype=torch.uint8))
    assert torch.equal(host[:total0], ref)                           # the seven segments sit where they sat and hold what they held
    assert views(host)[3].tolist() == [0, 2, 3] and views(host)[5].tolist() == [3.0]
    host, _ = st.pack(targets, pm, masks, out=own, live_tokens=9)      # each side of a pair packs its own count
    assert st._live_word(host).tolist() == [9]
    with pytest.raises(ValueError, match="live_tokens"):
        st.pack(targets, pm, masks, out=own)


def test_caption_tables_of_a_longer_bucket_are_zero_beyond_the_caption():
    from toist_amd import harness
    from toist_amd.distill import DistillTables
    B, L, Lp = 2, 10, 16
    batch = harness.synthetic_distill_batch(B, 64, 64, tokens=12, tokens_pronoun=L, seed=4, max_targets=3)
    for t in batch["targets"][1]:
        assert len(t["boxes"]) > 0
    wide, own = DistillTables(B, Lp, "cpu", pronoun_side=True), DistillTables(B, L, "cpu", pronoun_side=True)
    vw = wide._views(wide.pack(batch["tokenized"][1], batch["targets"][1], batch["captions"][1]))
    vo = own._views(own.pack(batch["tokenized"][1], batch["targets"][1], batch["captions"][1]))
    for i in (0, 1):                   # W_span, W_sth [B, L]
        assert torch.equal(vw[i][:, :L], vo[i]) and not vw[i][:, L:].any() and bool(vo[i].any())
    for i in (2, 3):                   # sub_span, sub_sth [L, B]
        assert torch.equal(vw[i][:L], vo[i]) and not vw[i][L:].any()
    for i in (4, 5, 6, 7):             # the task grouping does not depend on the caption length
        assert torch.equal(vw[i], vo[i])
