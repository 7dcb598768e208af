"""Shared-image training with the mask head, the parts that need no device: harness.synthetic_pair_batch(with_masks=True), the constructor and
table errors of harness.CapturedMaskPairTrainStep, the refusals of DETRsegm.encode_mask_pairs / decode_mask_pairs, the two refusals that stay
(DETRsegm.encode_pairs, CapturedPairTrainStep on a mask head), and the declaration, export and binding of the two new entry points."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("toist_resize_add_rows_pairs", "toist_sum_maps_by_image")


@pytest.fixture(scope="module")
def models():
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    tiny = dict(device="cpu", enc_layers=1, dec_layers=1, num_queries=4)
    det = toist_amd.build_model(harness.default_args(**tiny))
    seg = toist_amd.build_model(harness.default_args(masks=True, mask_model="smallconv", **tiny))
    assert hasattr(seg[0], "detr") and not hasattr(det[0], "detr") and "masks" in seg[1].losses
    return det, seg


# ------------------------------------------------------------------------------------------------------------------ the synthetic batch
def test_synthetic_pair_batch_with_masks_shapes():
    from toist_amd import harness
    pairs = [(0, 0), (1, 2), (1, 1), (0, 2), (1, 0)]
    plain = harness.synthetic_pair_batch(2, 3, pairs, height=48, width=80, tokens=6, seed=4, max_targets=3)
    samples, tok, pi, pc, targets, pmap = harness.synthetic_pair_batch(2, 3, pairs, height=48, width=80, tokens=6, seed=4, max_targets=3, with_masks=True)
    assert all("masks" not in t for t in plain[4])                                     # the default is unchanged
    assert tuple(samples.tensors.shape) == (2, 3, 48, 80) and tok["input_ids"].shape == (3, 6)
    assert pi.tolist() == [0, 1, 1, 0, 1] and pc.tolist() == [0, 2, 1, 2, 0] and len(targets) == 5
    assert sum(len(t["boxes"]) for t in targets) == pmap.shape[0] > 0
    for t, u in zip(targets, plain[4]):                                                # pair order, the same boxes with and without masks
        n = len(t["boxes"])
        assert torch.equal(t["boxes"], u["boxes"]) and torch.equal(t["positive_map"], u["positive_map"])
        assert t["masks"].dtype == torch.bool and tuple(t["masks"].shape) == (n, 48, 80)
        assert all(bool(m.any()) for m in t["masks"])                                  # every box has at least one pixel
    assert torch.equal(pmap, plain[5]) and torch.equal(samples.tensors, plain[0].tensors)


# ------------------------------------------------------------------------------------------------------------------ the captured step
def test_captured_mask_pair_train_step_constructor_errors(models):
    from types import SimpleNamespace
    from toist_amd import harness
    (det, det_criterion, _, _), (seg, criterion, _, weight_dict) = models
    mk = lambda model=seg, crit=criterion, **kw: harness.CapturedMaskPairTrainStep(model, crit, None, weight_dict, **{"batch": 2, "captions": 3, "pairs": 4, **kw})
    with pytest.raises(ValueError, match="mask head"):
        mk(model=det)
    for bad in ({"batch": 0}, {"captions": 0}, {"pairs": 0}, {"pairs": -1}):
        with pytest.raises(ValueError, match="CapturedMaskPairTrainStep"):
            mk(**bad)
    with pytest.raises(TypeError):
        harness.CapturedMaskPairTrainStep(seg, criterion, None, weight_dict, batch=2, captions=3)              # pairs is required
    cap = mk()
    assert isinstance(cap, harness.CapturedPairTrainStep) and cap.masks
    assert (cap.batch, cap.captions, cap.pairs, cap.num_queries, cap.captures, cap.replays) == (2, 3, 4, 4, 0, 0)
    assert not mk(crit=SimpleNamespace(losses=["labels", "boxes", "cardinality"])).masks                       # a criterion without mask losses is taken too
    # the two refusals of the detection step stay exactly as they were
    with pytest.raises(NotImplementedError, match="shared-image training with a mask head"):
        harness.CapturedPairTrainStep(seg, det_criterion, None, weight_dict, batch=2, captions=3, pairs=4)
    with pytest.raises(ValueError, match="mask losses"):
        harness.CapturedPairTrainStep(det, criterion, None, weight_dict, batch=2, captions=3, pairs=4)
    assert harness.CapturedPairTrainStep(det, det_criterion, None, weight_dict, batch=2, captions=3, pairs=4).masks is False


def test_captured_mask_pair_train_step_checks_a_batch_on_the_host(models):
    """Every refusal of step() comes before anything is uploaded or launched: on a host without a device they are all that happens."""
    from toist_amd import harness, kernels
    _, (seg, criterion, _, weight_dict) = models
    cap = harness.CapturedMaskPairTrainStep(seg, criterion, None, weight_dict, batch=2, captions=3, pairs=4)
    seed_word = kernels.SEED_DEV
    good = [(0, 0), (1, 2), (1, 1), (0, 2)]
    batch = lambda B=2, T=3, pairs=good: harness.synthetic_pair_batch(B, T, pairs, height=32, width=32, tokens=6, max_targets=2, with_masks=True)
    with pytest.raises(ValueError, match="exactly 4 pairs"):
        cap.step(*batch(pairs=good[:3]))
    with pytest.raises(ValueError, match="exactly 4 pairs"):
        cap.step(*batch(pairs=good + [(0, 0)]))
    with pytest.raises(ValueError, match="2 images and 3 captions"):
        cap.step(*batch(B=3))
    samples, tok, pi, pc, targets, pmap = batch()
    for bad_i, bad_c in (([0, 2, 1, 0], pc), ([0, -1, 1, 0], pc), (pi, [0, 3, 1, 2])):
        with pytest.raises(ValueError, match="outside"):
            cap.step(samples, tok, bad_i, bad_c, targets, pmap)
    with pytest.raises(ValueError, match="target dicts"):
        cap.step(samples, tok, pi, pc, targets[:3], pmap)
    by_size = [{**{k_: v for k_, v in t.items() if k_ != "masks"}, "mask_size": (32, 32)} for t in targets]
    with pytest.raises(ValueError, match="mask_size"):
        cap.step(samples, tok, pi, pc, by_size, pmap)
    with pytest.raises(ValueError, match="carries \"masks\""):
        cap.step(samples, tok, pi, pc, [{k_: v for k_, v in t.items() if k_ != "masks"} for t in targets], pmap)
    with pytest.raises(ValueError, match="target_masks"):
        cap.step(samples, tok, pi, pc, targets, pmap, target_masks=object())
    assert cap.captures == 0 and cap.replays == 0 and not cap._buckets and not cap._ready and kernels.SEED_DEV is seed_word      # nothing was built


# ------------------------------------------------------------------------------------------------------------------ the model's entry points
def test_encode_mask_pairs_refuses_as_encode_pairs_does(models):
    from toist_amd import harness
    (det, _, _, _), (seg, _, _, _) = models
    samples, tok, pi, pc, _, _ = harness.synthetic_pair_batch(1, 2, 2, height=64, width=64, tokens=6, max_targets=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.encode_mask_pairs(samples, tok, pi, pc)
    seg.detr.split_backward = True
    try:
        with pytest.raises(RuntimeError, match="backward cuts"):
            seg.encode_mask_pairs(samples, tok, pi, pc)
    finally:
        del seg.detr.split_backward
    with pytest.raises(ValueError, match="must end with 4"):
        det.encode_pairs(samples, tok, pi, pc, levels=(1, 2))
    with pytest.raises(ValueError, match="encode_mask_pairs"):
        seg.decode_mask_pairs({"_native": {"features": [None]}})
    with pytest.raises(NotImplementedError, match="shared-image training with a mask head"):       # the refusal beside them stays
        seg.encode_pairs(samples, tok, pi, pc)


# ------------------------------------------------------------------------------------------------------------------ the library
def _prototypes():
    with open(os.path.join(ROOT, "include", "toist_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"TOIST_API\s+int\s+(\w+)\s*\(([^;]*)\)\s*;", text)}


def test_the_new_entry_points_are_declared_exported_and_bound():
    from toist_amd import _lib
    protos = _prototypes()
    with open(os.path.join(ROOT, "toist_amd", "csrc", "exports.map")) as f:
        assert re.search(r"global:\s*toist_\*;", f.read())
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {"toist_resize_add_rows_pairs": [p, p, p, p] + [i32] * 9 + [p, p, p], "toist_sum_maps_by_image": [p, p, p, i32, i32, i32, i32, i64, p, p, p]}
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/toist_hip.h"
        for arg in ("const int32_t* pair_image", "int n_images", "int P", "int32_t* status", "void* stream"):
            assert arg in protos[name], (name, arg)
        assert _lib.SIGNATURES[name] == want[name], name
        fn = getattr(_lib.lib(), name)                                                  # exported by the built library
        assert list(fn.argtypes) == want[name] and fn.restype is ctypes.c_int
    assert "const int64_t* rows" in protos["toist_resize_add_rows_pairs"] and "const int32_t* seg" in protos["toist_sum_maps_by_image"]


def test_the_new_entry_points_refuse_on_the_host():
    """bad extents and null pointers end in an error code and a message before any launch (no pointer below is ever dereferenced)"""
    from toist_amd import _lib
    lib, some = _lib.lib(), ctypes.c_void_p(4096)
    # (in, fpn, rows, pair_image, n_images, P, n, Q, H, W, OH, OW, C, out, status, stream)
    resize = lambda ptrs=(some,) * 6, n_images=3, P=5, n=6, Q=3, H=2, W=3, OH=4, OW=6, C=16: \
        lib.toist_resize_add_rows_pairs(*ptrs[:4], n_images, P, n, Q, H, W, OH, OW, C, *ptrs[4:], None)
    for hole in range(6):
        assert resize(tuple(None if j == hole else some for j in range(6))) != _lib.TOIST_OK and "toist_resize_add_rows_pairs" in _lib.last_error()
    for bad in (dict(C=12), dict(C=0), dict(n=0), dict(P=0), dict(n_images=0), dict(Q=0), dict(H=0), dict(OH=1), dict(OW=2)):
        assert resize(**bad) != _lib.TOIST_OK, bad
    # (in, seg, pair_image, P, Q, n_images, rows, per, out, status, stream); seg may be NULL
    total = lambda ptrs=(some,) * 4, P=5, Q=3, n_images=3, rows=15, per=104: \
        lib.toist_sum_maps_by_image(ptrs[0], None, ptrs[1], P, Q, n_images, rows, per, ptrs[2], ptrs[3], None)
    for hole in range(4):
        assert total(tuple(None if j == hole else some for j in range(4))) != _lib.TOIST_OK and "toist_sum_maps_by_image" in _lib.last_error()
    for bad in (dict(per=100), dict(per=0), dict(P=0), dict(Q=0), dict(n_images=0), dict(rows=0)):
        assert total(**bad) != _lib.TOIST_OK, bad
