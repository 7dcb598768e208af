"""Device-side target masks (csrc/tmask.hip through toist_amd.preprocess.DeviceTargetMasks) against the host pipeline they replace
(preprocess.transform_target's torch ops + StaticTargets' pinned mask image): the bytes are EQUAL, in dense(), inside a StaticTargets, from a
replayed graph, and the captured training step of configs[2] computes the same losses from them."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _src(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, h, w, generator=g) > 0.5


def _host(src, plan):
    from toist_amd.preprocess import transform_target
    return transform_target({"masks": src}, plan)["masks"]        # (no crop drops a dense random mask: every target stays)


def _plans():
    from toist_amd.preprocess import PrepPlan
    return {"no_resize": PrepPlan(53, 37, final=(37, 53)), "upscale": PrepPlan(53, 37, final=(64, 91)), "downscale": PrepPlan(96, 64, final=(23, 35)),
            "flip": PrepPlan(53, 37, flip=True, final=(64, 91)),
            "flip_first_crop_final": PrepPlan(96, 64, flip=True, first=(80, 120), crop=(7, 9, 60, 100), final=(96, 160)),
            "width_32": PrepPlan(32, 20, flip=True, final=(40, 64)), "width_33": PrepPlan(33, 20, flip=True, final=(40, 66)),
            "width_64": PrepPlan(64, 20, final=(40, 128)),
            # a 4.8x reduction: the first 16 output columns read source columns 0 .. 72, THREE words -- the kernel's path that reloads a word when
            # the column leaves it (up to 2x a thread's columns lie in two adjacent words); columns 16 .. 19 read one word: both paths in one workgroup
            "reduce_5x": PrepPlan(96, 64, final=(16, 20)), "reduce_5x_flip": PrepPlan(96, 64, flip=True, final=(16, 20)),
            "reduce_4x_crop": PrepPlan(96, 64, flip=True, crop=(2, 10, 60, 86), final=(21, 20))}


def test_the_plans_cover_both_column_paths_of_the_kernel():
    """Host arithmetic only: which groups of 16 output columns span more than two 32-bit source words (the kernel's reloading path)."""
    from toist_amd.preprocess import mask_index_tables
    spans = {}
    for name, plan in _plans().items():
        words = mask_index_tables(plan)[1] >> 5
        spans[name] = max(int(words[g:g + 16].max() - words[g:g + 16].min()) for g in range(0, len(words), 16))
    assert all(spans[n] >= 2 for n in ("reduce_5x", "reduce_5x_flip", "reduce_4x_crop")) and all(spans[n] <= 1 for n in ("upscale", "flip", "width_64", "downscale"))


@pytest.mark.parametrize("name", list(_plans()))
def test_dense_equals_the_host_masks(dev, name):
    from toist_amd.preprocess import DeviceTargetMasks
    plan = _plans()[name]
    tm = DeviceTargetMasks(dev, max_batch=1, max_targets_per_image=3, max_src_pixels=3 * 64 * 96, max_out_hw=(128, 160))
    src = _src(3, plan.height, plan.width, 5)
    packed = tm.pack([src], [plan])
    got = tm.dense(packed)
    want = _host(src, plan)
    assert len(got) == 1 and got[0].dtype == torch.bool and got[0].is_cuda and got[0].shape == want.shape
    assert torch.equal(got[0].cpu(), want)
    assert packed.slots == 3 and packed.counts == (3,) and packed.sizes == (tuple(plan.final),)


def _boxed_target(src, boxes):
    n = src.shape[0]
    return {"boxes": torch.tensor(boxes, dtype=torch.float32).reshape(n, 4), "labels": torch.arange(n), "masks": src}


def test_dense_with_a_dropped_target_and_an_image_without_targets(dev):
    """A crop that drops one of three targets (only the surviving rows travel), and an image with zero targets inside a batch of three."""
    from toist_amd.preprocess import DeviceTargetMasks, PrepPlan, transform_target
    tm = DeviceTargetMasks(dev, max_batch=3, max_targets_per_image=2, max_src_pixels=4 * 64 * 96, max_out_hw=(128, 160))
    crop = PrepPlan(96, 64, first=(80, 120), crop=(0, 0, 40, 60), final=(64, 96))
    tgt = _boxed_target(_src(3, 64, 96, 21), [[2, 2, 30, 20], [70, 45, 90, 60], [10, 5, 40, 30]])          # the second box lies outside the crop
    full, lean = transform_target(tgt, crop), transform_target(tgt, crop, masks=False)
    assert lean["mask_rows"].tolist() == [0, 2] and full["masks"].shape[0] == 2
    plain = PrepPlan(53, 37, flip=True, final=(64, 91))
    empty = PrepPlan(40, 30, final=(60, 80))
    src2 = _src(1, 37, 53, 22)
    packed = tm.pack([tgt["masks"], torch.zeros(0, 30, 40, dtype=torch.bool), src2], [crop, empty, plain],
                     [lean["mask_rows"], torch.zeros(0, dtype=torch.int64), torch.arange(1)])
    assert packed.slots == 3 and packed.counts == (2, 0, 1)
    got = tm.dense(packed)
    assert torch.equal(got[0].cpu(), full["masks"])
    assert tuple(got[1].shape) == (0, 60, 80)
    assert torch.equal(got[2].cpu(), _host(src2, plain))


def _ragged_batch(seed, final_hw=((100, 150), (128, 160), (77, 131))):
    """Three images with 2, 0 and 1 targets: -> (source masks, plans, host-path targets, device-path targets, positive map)."""
    from toist_amd.preprocess import PrepPlan, transform_target
    plans = [PrepPlan(96, 64, flip=True, final=final_hw[0]), PrepPlan(53, 37, final=final_hw[1]),
             PrepPlan(90, 60, first=(80, 120), crop=(3, 5, 70, 100), final=final_hw[2])]
    counts = (2, 0, 1)
    srcs, host_t, size_t = [], [], []
    for i, (p, n) in enumerate(zip(plans, counts)):
        src = _src(n, p.height, p.width, seed + i)
        tgt = _boxed_target(src, [[1, 1, p.width - 1, p.height - 1]] * n)          # boxes over the whole image: every target survives the crop
        srcs.append(src)
        host_t.append(transform_target(tgt, p))
        size_t.append(transform_target(tgt, p, masks=False))
        assert size_t[-1]["mask_rows"].tolist() == list(range(n))
    g = torch.Generator().manual_seed(seed)
    return srcs, plans, host_t, size_t, torch.rand(sum(counts), 256, generator=g)


def _static_targets(dev, mask_hw):
    from toist_amd.matcher import StaticTargets
    st = StaticTargets(3, 2, 10, 256, dev, mask_hw=mask_hw)
    st.masks.fill_(0xFF)
    return st


@pytest.mark.parametrize("mask_hw,final_hw", [((128, 160), ((100, 150), (128, 160), (77, 131))),
                                              ((40, 50), ((37, 47), (40, 50), (22, 33))),           # cap_w = 50: rows that are not 4-byte aligned
                                              # a 96-wide source reduced to 20 columns: threads on the reloading path and on the two-word path
                                              # inside one workgroup (the first image's slots), beside slots that only take the two-word path
                                              ((128, 160), ((16, 20), (128, 160), (77, 131))),
                                              # cap_w = 300 > the 256-column tile: a second tile along x, live for 44 / 24 columns and padding
                                              ((16, 300), ((16, 300), (10, 280), (12, 270)))])
def test_write_into_static_targets_equals_the_host_load(dev, mask_hw, final_hw):
    from toist_amd.preprocess import DeviceTargetMasks
    srcs, plans, host_t, size_t, pmap = _ragged_batch(31, final_hw)
    ref = _static_targets(dev, mask_hw).load(host_t, pmap)
    st = _static_targets(dev, mask_hw).load(size_t, pmap)
    assert bool((st.masks == 0xFF).all())                         # "mask_size" targets: no mask bytes travel with the targets
    tm = DeviceTargetMasks(dev, max_batch=3, max_targets_per_image=2, max_src_pixels=3 * 64 * 96, max_out_hw=mask_hw)
    packed = tm.pack(srcs, plans, [t["mask_rows"] for t in size_t])
    tm.write_into(st)
    torch.cuda.synchronize()
    tot = packed.slots
    assert tot == 3 and st.sizes == ref.sizes == [2, 0, 1]
    assert torch.equal(st.masks[:tot], ref.masks[:tot])           # live slots: the host path's bytes, zero padding included
    assert int(st.masks[:tot].max()) == 1 and bool((st.masks[0, final_hw[0][0]:] == 0).all()) and bool((st.masks[0, :, final_hw[0][1]:] == 0).all())
    assert bool((st.masks[tot:] == 0xFF).all())                   # dead slots: not written
    assert torch.equal(st.valid_hw, ref.valid_hw) and st.valid_hw.tolist()[:2] == [max(h for h, _ in final_hw), max(w for _, w in final_hw)]


def test_one_captured_launch_serves_every_pack(dev):
    from toist_amd.preprocess import DeviceTargetMasks
    mask_hw = (128, 160)
    tm = DeviceTargetMasks(dev, max_batch=3, max_targets_per_image=2, max_src_pixels=3 * 64 * 96, max_out_hw=mask_hw)
    st = _static_targets(dev, mask_hw)
    batches = [_ragged_batch(41), _ragged_batch(42, ((64, 91), (30, 40), (128, 160))), _ragged_batch(43, ((23, 35), (128, 160), (90, 100)))]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        tm.pack(batches[0][0], batches[0][1])
        tm.write_into(st)                                         # (once eagerly, then the capture of the same launch)
        with torch.cuda.graph(graph, stream=side):
            tm.write_into(st)
    torch.cuda.current_stream().wait_stream(side)
    for srcs, plans, host_t, size_t, pmap in batches:
        ref = _static_targets(dev, mask_hw).load(host_t, pmap)
        st.masks.fill_(0xFF)
        packed = tm.pack(srcs, plans)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st.masks[:packed.slots], ref.masks[:packed.slots]) and bool((st.masks[packed.slots:] == 0xFF).all())


def test_write_into_refuses_what_does_not_fit(dev):
    from toist_amd.matcher import StaticTargets
    from toist_amd.preprocess import DeviceTargetMasks
    srcs, plans, _, _, _ = _ragged_batch(51)
    tm = DeviceTargetMasks(dev, max_batch=3, max_targets_per_image=2, max_src_pixels=3 * 64 * 96, max_out_hw=(128, 160))
    tm.pack(srcs, plans)
    with pytest.raises(ValueError, match="do not fit"):
        tm.write_into(_static_targets(dev, (64, 160)))
    with pytest.raises(ValueError, match="exceeds"):
        tm.write_into(StaticTargets(4, 2, 10, 256, dev, mask_hw=(128, 160)))
    with pytest.raises(ValueError, match="without mask_hw"):
        tm.write_into(StaticTargets(3, 2, 10, 256, dev))


def _mask_step_setup(dev):
    """configs[2] on the smallest mask model of tests/test_gpu_captured_step.py + three batches of one bucket (128 x 192, 12 tokens) whose ground-truth
    masks are 64 x 96 sources resized (and, in the second batch, flipped) to 128 x 192: as host masks, and as "mask_size" targets + source masks."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.preprocess import DeviceTargetMasks, PrepPlan
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=2, num_queries=20, dropout=0.0, masks=True, mask_model="smallconv")
    torch.manual_seed(0)
    model0, criterion0, _, weight_dict = toist_amd.build_model(args)
    model0.to(dev).train()
    det = model0.detr
    det.transformer.text_encoder.config.hidden_dropout_prob = 0.0
    det.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
    criterion0.train()
    batches = []
    for i, mt in enumerate((4, 5, 3)):
        samples, tok, targets, pmap = harness.synthetic_batch(2, 128, 192, tokens=12, seed=70 + i, max_targets=mt, with_masks=True)
        plan = PrepPlan(96, 64, flip=(i == 1), final=(128, 192))
        srcs = [t["masks"][:, ::2, ::2].contiguous() for t in targets]
        host_t = [{**t, "masks": _host(s, plan)} for t, s in zip(targets, srcs)]
        size_t = [{**{k: v for k, v in t.items() if k != "masks"}, "mask_size": (128, 192)} for t in targets]
        batches.append((samples.to(dev), tok.to(dev), host_t, size_t, pmap, srcs, [plan, plan]))
    tm = DeviceTargetMasks(dev, max_batch=2, max_targets_per_image=6, max_src_pixels=12 * 64 * 96, max_out_hw=(128, 192))
    return model0, criterion0, weight_dict, batches, tm


def _three_steps(dev, setup, on_device):
    """A fresh CapturedTrainStep on a copy of the model: the three batches -> their total losses (step 1 eager, steps 2-3 replays)."""
    from toist_amd import harness, kernels
    from toist_amd.optim import FusedClipAdamWEMA
    model0, criterion0, weight_dict, batches, tm = setup
    model, criterion = copy.deepcopy(model0), copy.deepcopy(criterion0)
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    # lr = 0: the whole step runs (forward, backward, clip + AdamW + EMA) and leaves the weights where they were.  What is compared is what a batch's
    # mask bytes do to its loss, and that must not ride on the update: the gradients of a masks step are not bit-reproducible, and the first AdamW
    # steps move every weight by about lr * sign(g), so a last-bit difference of a near-zero gradient flips a whole update -- with lr = 1e-4 two
    # HOST-fed runs of these batches differed from each other by up to 2.3e-3 (of 28.8) at step 2 and 0.15 (of 26.3) at step 3, measured on an MI355X
    opt = FusedClipAdamWEMA([{"params": [p for p in model.parameters() if p.requires_grad], "lr": 0.0}], weight_decay=1e-4, max_norm=0.1)
    cap = harness.CapturedTrainStep(model, criterion, opt, weight_dict, batch=2, max_targets_per_image=6, pad_hw=64, pad_tokens=1)
    assert cap.masks
    if on_device:
        with pytest.raises(ValueError, match="target_masks"):
            cap.step(batches[0][0], batches[0][1], batches[0][3], batches[0][4])
        assert not cap._buckets                                # refused before the bucket was touched
        srcs, plans = batches[0][5], batches[0][6]
        short = [torch.arange(max(int(m.shape[0]) - 1, 0)) for m in srcs]          # one mask fewer than the image has targets
        assert any(m.shape[0] for m in srcs)
        tm.pack(srcs, plans, short)
        with pytest.raises(ValueError, match="targets per image"):
            cap.step(batches[0][0], batches[0][1], batches[0][3], batches[0][4], target_masks=tm)          # before the launch
        assert cap.captures == 0 and cap.replays == 0
    totals = []
    for samples, tok, host_t, size_t, pmap, srcs, plans in batches:
        if on_device:
            tm.pack(srcs, plans)
            loss = cap.step(samples, tok, size_t, pmap, target_masks=tm)
        else:
            loss = cap.step(samples, tok, host_t, pmap)
        totals.append(float(loss.detach()))
    assert cap.captures == 1 and cap.replays == 2              # step 1 eager, steps 2-3 replays
    return totals


def test_captured_step_fed_with_device_masks_equals_the_host_fed_step(dev):
    """The same three batches through CapturedTrainSteps built from the same weights, one fed host masks, one fed "mask_size" targets + target_masks=.
    The bytes in StaticTargets.masks are identical (the tests above), so the two may differ only by what the step differs from itself run to run:
    host-fed against host-fed is measured first, here, in the same process.  With the weights held still (_three_steps) that measurement is
    bit-equality at every step -- on an MI355X, 16 host-fed and 8 device-fed runs gave one value per step -- so bit-equality is what is required.
    What this gives up: with lr = 0 no step sees weights that an earlier step's mask gradients moved, so the effect of the masks' gradients on LATER
    steps is not compared -- only each step's loss (detection + mask losses, through forward, backward and the optimizer tail) on fixed weights."""
    from toist_amd import engine, kernels
    old_reuse, old_seed = engine.REUSE_GRAD_BUFFERS, kernels.SEED_DEV          # (later tests draw their dropout masks from the seed word they find)
    setup = _mask_step_setup(dev)
    try:
        host_a, host_b, device = _three_steps(dev, setup, False), _three_steps(dev, setup, False), _three_steps(dev, setup, True)
    finally:
        engine.REUSE_GRAD_BUFFERS, kernels.SEED_DEV = old_reuse, old_seed
    print("host-fed", host_a, "host-fed again", host_b, "device-fed", device)
    assert all(v == v and abs(v) < 1e4 for v in host_a) and len(set(host_a)) == 3
    assert host_a == host_b, ("the host-fed step against itself", host_a, host_b)
    assert device == host_a, ("device-fed against host-fed", host_a, device)
