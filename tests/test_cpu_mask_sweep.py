"""Host side of the task sweep with the mask head: the pass splitting (sweep.pair_passes), what CapturedMaskSweepStep and SweepEvaluator refuse before
anything touches a device, the three new entry points in the C header and the export map, and the detection sweep's refusals on a DETRsegm, which stay."""
import fnmatch
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("toist_mask_stage_fwd_pairs", "toist_resize_add_pairs", "toist_sweep_gather")


# ------------------------------------------------------------------------------------------------------------------ pair_passes
@pytest.mark.parametrize("P,per,want", [
    (1, 8, [(0, 1)]),                                   # one pair
    (8, 8, [(0, 8)]),                                   # exactly one pass
    (5, 8, [(0, 5)]),                                   # below
    (16, 8, [(0, 8), (8, 16)]),                         # above, no remainder
    (19, 8, [(0, 8), (8, 16), (16, 19)]),               # a remainder pass
    (3, 1, [(0, 1), (1, 2), (2, 3)]),
    (112, 16, [(16 * i, 16 * i + 16) for i in range(7)]),
])
def test_pair_passes(P, per, want):
    from toist_amd.sweep import pair_passes
    got = pair_passes(P, per)
    assert got == want
    assert got[0][0] == 0 and got[-1][1] == P and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    assert all(0 < hi - lo <= per for lo, hi in got)


@pytest.mark.parametrize("P,per", [(4, 0), (4, -1), (0, 8), (-3, 8), (4, 2.5), (4, True)])
def test_pair_passes_refuses(P, per):
    from toist_amd.sweep import pair_passes
    with pytest.raises(ValueError):
        pair_passes(P, per)


# ------------------------------------------------------------------------------------------------------------------ the models
@pytest.fixture(scope="module")
def models():
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    tiny = dict(device="cpu", enc_layers=1, dec_layers=1, num_queries=4)
    det = toist_amd.build_model(harness.default_args(**tiny))[0].eval()
    seg = toist_amd.build_model(harness.default_args(masks=True, mask_model="smallconv", **tiny))[0].eval()
    assert hasattr(seg, "detr") and not hasattr(det, "detr")
    return det, seg


def test_captured_mask_sweep_step_constructor_refusals(models):
    from toist_amd import harness
    det, seg = models
    ok = dict(batch=2, captions=3, max_orig_hw=(96, 96), device="cpu")
    with pytest.raises(ValueError, match="mask head"):
        harness.CapturedMaskSweepStep(det, **ok)
    with pytest.raises(ValueError, match="cluster criterion"):
        harness.CapturedMaskSweepStep(seg, object(), **ok)
    with pytest.raises(ValueError, match="max_orig_hw"):
        harness.CapturedMaskSweepStep(seg, batch=2, captions=3, device="cpu")
    with pytest.raises(ValueError):
        harness.CapturedMaskSweepStep(seg, **ok, pairs_per_pass=0)
    with pytest.raises(ValueError):
        harness.CapturedMaskSweepStep(seg, **ok, pairs=0)
    step = harness.CapturedMaskSweepStep(seg, **ok, pairs=5, pairs_per_pass=2)           # nothing is allocated before the first step
    assert (step.pairs, step.pairs_per_pass, step.captures, step.replays) == (5, 2, 0, 0)
    assert step.capacity_words == 4 * 96 * 2
    assert harness.CapturedMaskSweepStep(seg, **ok).pairs == 6


def test_captured_mask_sweep_step_checks_sizes_on_the_host(models):
    """CapturedEvalStep.check_sizes' rules, on the object itself: the bucket, the capacity of the planes, one size per image"""
    from toist_amd import harness
    step = harness.CapturedMaskSweepStep(models[1], batch=2, captions=3, max_orig_hw=(96, 96), device="cpu")
    key = (64, 64, 6)
    assert step.check_sizes(key, [(90, 80), (96, 96)], [(64, 60), (50, 64)]) == ([(90, 80), (96, 96)], [(64, 60), (50, 64)])
    with pytest.raises(ValueError, match="max_orig_hw"):
        step.check_sizes(key, [(97, 80), (96, 96)], [(64, 60), (50, 64)])
    with pytest.raises(ValueError, match="does not fit"):
        step.check_sizes(key, [(90, 80), (96, 96)], [(65, 60), (50, 64)])
    with pytest.raises(ValueError):
        step.check_sizes(key, [(90, 80)], [(64, 60)])


def test_the_detection_sweep_still_refuses_a_mask_head(models):
    from toist_amd import harness
    _, seg = models
    for name in ("encode_sweep", "sweep_images", "sweep_text", "sweep_pairs", "sweep_stages"):
        with pytest.raises(NotImplementedError) as e:
            getattr(seg, name)(None)
        assert "task sweep with a mask head" in str(e.value) and "DETRsegm sweeps" in str(e.value), name
    with pytest.raises(NotImplementedError, match="shared-image training with a mask head"):
        seg.encode_pairs(None, None, None, None)
    with pytest.raises(NotImplementedError, match="DETRsegm sweeps"):
        harness.CapturedSweepStep(seg, batch=2, captions=3, device="cpu")
    for name in ("encode_mask_sweep", "mask_sweep_stages", "mask_sweep_pairs", "decode_mask_sweep"):
        assert callable(getattr(seg, name))


def test_mask_sweep_is_inference_only_and_needs_the_device(models):
    from toist_amd import harness
    _, seg = models
    samples, tok, _, _ = harness.synthetic_batch(1, 64, 64, tokens=6, seed=1, max_targets=0)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            seg.encode_mask_sweep(samples, tok)
    with pytest.raises(RuntimeError, match="inference only"):
        seg.encode_mask_sweep(samples, tok)
    with torch.no_grad():
        with pytest.raises(ValueError, match="encode_mask_sweep"):
            seg.decode_mask_sweep({"_native": {}})
        with pytest.raises(ValueError, match="end with 4"):
            seg.detr.sweep_images(samples, levels=(1, 2))


# ------------------------------------------------------------------------------------------------------------------ SweepEvaluator
@pytest.mark.parametrize("bad", [(), ("bbox", "keypoints"), "segm", ("segm", "segm"), None, ("mask",)])
def test_sweep_evaluator_validates_iou_types_before_anything_else(bad):
    from toist_amd.coco_eval import SweepEvaluator
    with pytest.raises(ValueError, match="iou_types"):
        SweepEvaluator({"cut": {"images": [], "annotations": [], "categories": []}}, "cuda", iou_types=bad)


def test_sweep_evaluator_segm_needs_masks():
    from toist_amd.coco_eval import SweepEvaluator
    sw = object.__new__(SweepEvaluator)                                    # (the constructor builds device evaluators)
    sw.iou_types = ("bbox", "segm")
    with pytest.raises(ValueError, match="masks"):
        sw.update_rows({"scores": torch.zeros(1, 4), "boxes": torch.zeros(1, 4, 4)}, [7], ["cut"], [0], [0])
    with pytest.raises(TypeError, match="RowMasks"):
        sw.update_rows({"scores": torch.zeros(1, 4), "boxes": torch.zeros(1, 4, 4)}, [7], ["cut"], [0], [0], masks=object())


def test_sweep_evaluator_summarize_adds_the_mask_numbers():
    import types

    import numpy as np
    from toist_amd.coco_eval import SweepEvaluator
    box = {"cut": np.arange(12, dtype=np.float64) / 20, "sit": np.full(12, 0.5)}
    seg = {"cut": np.arange(12, dtype=np.float64) / 40, "sit": np.full(12, 0.25)}

    def stub(name):
        return types.SimpleNamespace(coco_eval={"bbox": types.SimpleNamespace(stats=box[name]), "segm": types.SimpleNamespace(stats=seg[name])},
                                     summarize=lambda verbose: None)
    sw = object.__new__(SweepEvaluator)
    sw.iou_types = ("bbox", "segm")
    sw.evaluators = {name: stub(name) for name in box}
    got = sw.summarize()
    assert set(got) == {"tasks", "mAP50", "mAP", "segm"} and set(got["segm"]) == {"tasks", "mAP50", "mAP"}
    assert got["mAP50"] == pytest.approx((0.05 + 0.5) / 2) and got["segm"]["mAP50"] == pytest.approx((0.025 + 0.25) / 2)
    assert got["segm"]["mAP"] == pytest.approx(0.125) and all(got["segm"]["tasks"][n] is seg[n] for n in seg)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _prototypes():
    with open(os.path.join(ROOT, "include", "toist_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"TOIST_API\s+int\s+(\w+)\s*\(([^;]*)\)\s*;", text)}


def test_new_entry_points_are_declared_and_exported():
    protos = _prototypes()
    with open(os.path.join(ROOT, "toist_amd", "csrc", "exports.map")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    exported = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/toist_hip.h"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), f"{name} is not exported by csrc/exports.map"
        for arg in ("const int32_t* pair_image", "int n_images", "int32_t* status", "void* stream"):
            assert arg in protos[name], (name, arg)
    # the pairs form of the stage: the arguments of toist_mask_stage_fwd, then the table, the image count and the status word
    old = protos["toist_mask_stage_fwd"].replace(", void* stream", "")
    assert protos["toist_mask_stage_fwd_pairs"] == old + ", const int32_t* pair_image, int n_images, int32_t* status, void* stream"


def test_the_binding_carries_the_new_entry_points():
    from toist_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(_prototypes()[name].split(","))
