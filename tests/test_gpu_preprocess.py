"""csrc/prep.hip (toist_image_prep) through toist_amd.preprocess.DevicePreprocessor against Pillow's own output, tests/golden/preprocess.npz
(tests/golden/make_golden_preprocess.py).  Equality is torch.equal everywhere: the resampler is integer arithmetic and the normalisation a table of
correctly rounded fp32 values, so a single differing bit is a bug.  Neither Pillow nor the reference is imported here."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMPLE = ("upscale", "reduce", "h_only", "v_only", "reduce6", "one_pixel")


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests", "golden", "preprocess.npz")).items()}


@pytest.fixture(scope="module")
def prep(dev):
    from toist_amd.preprocess import DevicePreprocessor
    return DevicePreprocessor(dev, max_batch=4, max_src_pixels=333 * 500 + 4096, max_out_hw=(96, 100), pad_hw=1, max_mid_hw=(96, 100))


def _plan(golden, name, flip=False):
    from toist_amd.preprocess import PrepPlan
    h, w = golden[name + "_src"].shape[:2]
    return PrepPlan(w, h, flip=flip, final=tuple(golden[name + "_u8"].shape[:2]))


def _chain_plan(golden):
    from toist_amd.preprocess import PrepPlan
    flip, fh, fw, t, l, h, w, oh, ow = (int(v) for v in golden["chain_plan"])
    sh, sw = golden["chain_src"].shape[:2]
    return PrepPlan(sw, sh, flip=bool(flip), first=(fh, fw), crop=(t, l, h, w), final=(oh, ow))


@pytest.mark.parametrize("name", SIMPLE + ("flip",))
def test_fixture_case_both_modes(dev, golden, prep, name):
    """One image: the intermediate mode's uint8 image equals Pillow's resize, the final mode's fp32 planes equal ToTensor + Normalize of it; the mask is
    False on the image.  `reduce6` needs 7 chunks of source rows per tile (ksize 15, 333 rows -> 53), `one_pixel` clamps every tap to one pixel."""
    plan = _plan(golden, name, flip=(name == "flip"))
    src = golden[name + "_src"]
    u8 = prep.resize_u8([src], [plan])[0]
    assert u8.shape == golden[name + "_u8"].shape and torch.equal(u8.cpu(), golden[name + "_u8"]), name
    nt = prep.prepare([src.numpy()], [plan])
    assert tuple(nt.tensors.shape) == (1, 3) + tuple(plan.final) and nt.tensors.dtype == torch.float32 and nt.mask.dtype == torch.bool
    assert torch.equal(nt.tensors[0].cpu(), golden[name + "_f32"]), name
    assert not bool(nt.mask.any())


def test_ragged_batch_overwrites_a_poisoned_capacity(dev, golden):
    """Three images of different source and output sizes in one launch, into an output of 4 x 192 x 192 (a larger capacity than the batch: 3 images,
    extent 128 x 128 at pad_hw = 64) that was filled with NaN, under a mask filled with the WRONG value everywhere: the batch extent equals
    from_tensor_list's padded batch and mask, everything beyond is 0 / True, no NaN is left."""
    from toist_amd.misc import NestedTensor
    from toist_amd.preprocess import DevicePreprocessor
    prep = DevicePreprocessor(dev, max_batch=4, max_src_pixels=3 * 64 * 64, max_out_hw=(192, 192), pad_hw=64)
    out = NestedTensor(torch.full((4, 3, 192, 192), float("nan"), device=dev), torch.zeros(4, 192, 192, dtype=torch.bool, device=dev))
    out.mask[:3, :50, :50] = True                    # wrong inside the images too
    images = [golden[f"ragged{i}_src"] for i in range(3)]
    plans = [_plan(golden, f"ragged{i}") for i in range(3)]
    nt = prep.prepare(images, plans, out=out)
    assert tuple(nt.tensors.shape) == (3, 3, 128, 128) and tuple(nt.mask.shape) == (3, 128, 128)
    want_t, want_m = torch.zeros(4, 3, 192, 192), torch.ones(4, 192, 192, dtype=torch.bool)
    H, W = golden["ragged_batch"].shape[-2:]
    want_t[:3, :, :H, :W] = golden["ragged_batch"]
    want_m[:3, :H, :W] = golden["ragged_mask"]
    assert not bool(torch.isnan(out.tensors).any())
    assert torch.equal(out.tensors.cpu(), want_t) and torch.equal(out.mask.cpu(), want_m)
    assert torch.equal(nt.tensors.cpu(), want_t[:3, :, :128, :128]) and torch.equal(nt.mask.cpu(), want_m[:3, :128, :128])
    for i in range(3):
        h, w = plans[i].final
        assert torch.equal(nt.tensors[i, :, :h, :w].cpu(), golden[f"ragged{i}_f32"])
    # the object's own output (no `out`): the same batch
    own = prep.prepare(images, plans)
    assert torch.equal(own.tensors.cpu(), want_t[:3, :, :128, :128]) and torch.equal(own.mask.cpu(), want_m[:3, :128, :128])


def test_chain_two_launches(dev, golden, prep):
    """flip -> resize -> crop (aligned to nothing) -> resize: two launches with the uint8 image between them, next to a single-resize image in the
    same batch.  Covers the flip, the crop origin and the uint8 hand-over (its rounding is part of Pillow's result)."""
    plans = [_chain_plan(golden), _plan(golden, "upscale")]
    packed = prep.pack([golden["chain_src"], golden["upscale_src"]], plans)
    assert packed.two_stage and (packed.batch, packed.height, packed.width) == (2, 61, 82)
    nt = prep.view(packed, prep.launch())
    fh, fw = plans[0].first
    assert torch.equal(prep.mid[:3 * fh * fw].view(fh, fw, 3).cpu(), golden["chain_mid"])
    assert torch.equal(nt.tensors[0].cpu(), golden["chain_f32"])
    h, w = plans[1].final
    assert torch.equal(nt.tensors[1, :, :h, :w].cpu(), golden["upscale_f32"])
    assert not bool(nt.mask[1, :h, :w].any()) and bool(nt.mask[1, h:].all()) and bool(nt.mask[1, :, w:].all())
    assert float(nt.tensors[1, :, h:].abs().max()) == 0 and float(nt.tensors[1, :, :, w:].abs().max()) == 0


def test_one_captured_graph_serves_different_batches(dev, golden, prep):
    """launch() -- both stages -- captured ONCE, replayed after pack() of two batches that differ in image count, sizes, ksize, flips and in whether a
    first resize is used: each replay equals the eager result of the same batch, so no size is baked into the graph."""
    batches = [([golden["chain_src"], golden["reduce_src"], golden["flip_src"]], [_chain_plan(golden), _plan(golden, "reduce"), _plan(golden, "flip", flip=True)]),
               ([golden["reduce6_src"], golden["h_only_src"]], [_plan(golden, "reduce6"), _plan(golden, "h_only")])]
    eager = []
    for images, plans in batches:
        packed = prep.pack(images, plans)
        out = prep.launch()
        eager.append((packed, out.tensors.clone(), out.mask.clone()))
    assert torch.equal(eager[0][1][0, :, :61, :82].cpu(), golden["chain_f32"]) and torch.equal(eager[1][1][0, :, :53, :80].cpu(), golden["reduce6_f32"])
    assert not torch.equal(eager[0][1], eager[1][1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        prep.pack(*batches[1])
        prep.launch(first_stage=True)               # warm: nothing left to allocate inside the capture
        with torch.cuda.graph(graph, stream=side):
            prep.launch(first_stage=True)
    torch.cuda.current_stream().wait_stream(side)
    for n in (0, 1, 0):
        prep.out.tensors.fill_(float("nan"))
        prep.out.mask.fill_(False)
        prep.pack(*batches[n])
        graph.replay()
        assert torch.equal(prep.out.tensors, eager[n][1]) and torch.equal(prep.out.mask, eager[n][2]), n


def test_prepared_batch_through_captured_eval_step(dev, golden):
    """The ragged batch prepared with pad_hw = 64 IS a bucket-shaped input: CapturedEvalStep takes it through captured.upload unchanged, and its results
    equal those of the same step fed NestedTensor.from_tensor_list of the fixture's tensors (same bucket, same graph)."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.misc import NestedTensor
    from toist_amd.preprocess import DevicePreprocessor
    args = harness.default_args(device="cuda", enc_layers=1, dec_layers=2, num_queries=20)
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    _, tok, _, _ = harness.synthetic_batch(3, 128, 128, tokens=8, seed=5, max_targets=0)
    tok = tok.to(dev)
    step = harness.CapturedEvalStep(model, batch=3, masks=False, pad_hw=64, pad_tokens=8)
    plans = [_plan(golden, f"ragged{i}") for i in range(3)]
    sizes = [p.final for p in plans]
    orig = [(p.height, p.width) for p in plans]
    prep = DevicePreprocessor(dev, max_batch=3, max_src_pixels=3 * 64 * 64, max_out_hw=(128, 128), pad_hw=64)
    prepared = prep.prepare([golden[f"ragged{i}_src"] for i in range(3)], plans)
    want_in = NestedTensor.from_tensor_list([golden[f"ragged{i}_f32"] for i in range(3)]).to(dev)
    assert step.bucket_of(prepared, tok) == step.bucket_of(want_in, tok) == (128, 128, 8)

    def run(samples):
        return [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()} for r in step.step(samples, tok, orig, sizes)]

    run(want_in)                                    # the bucket's eager pass + capture; the two compared steps are both replays
    want = run(want_in)
    got = run(prepared)
    assert step.captures == 1 and step.replays == 2
    for g, w in zip(got, want):
        assert torch.equal(g["scores"], w["scores"]) and torch.equal(g["boxes"], w["boxes"]) and torch.equal(g["labels"], w["labels"])
    # and the inputs the step saw were the same bytes
    ent = next(iter(step._buckets.values()))
    assert torch.equal(ent["samples"].tensors[:, :, :90, :100].cpu(), golden["ragged_batch"]) and torch.equal(ent["samples"].mask[:, :90, :100].cpu(), golden["ragged_mask"])
