"""Host side of the shared-image training step: harness.synthetic_pair_batch / expand_pairs, the argument checks of CapturedPairTrainStep that need
no device, the refusals of MDETR.encode_pairs, and the declaration and binding of toist_sweep_assemble_bwd.  CPU only."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synthetic_pair_batch_shapes_and_pair_order():
    from toist_amd import harness
    from toist_amd.misc import NestedTensor
    pairs = [(1, 2), (0, 0), (1, 2), (0, 1)]
    samples, tok, pi, pc, targets, pmap = harness.synthetic_pair_batch(2, 3, pairs, height=32, width=48, tokens=7, seed=5, max_targets=3)
    assert isinstance(samples, NestedTensor) and tuple(samples.tensors.shape) == (2, 3, 32, 48) and tuple(samples.mask.shape) == (2, 32, 48)
    assert tuple(tok["input_ids"].shape) == (3, 7) and tuple(tok["attention_mask"].shape) == (3, 7)
    assert pi.dtype == torch.int32 and pc.dtype == torch.int32 and not pi.is_cuda
    assert pi.tolist() == [1, 0, 1, 0] and pc.tolist() == [2, 0, 2, 1]
    assert len(targets) == 4                                                    # one target dict per PAIR, not per image
    assert tuple(pmap.shape) == (sum(len(t["boxes"]) for t in targets), 256)
    row = 0
    for t in targets:                                                           # the positive map is the targets' rows in pair order
        n = len(t["boxes"])
        assert torch.equal(pmap[row:row + n], t["positive_map"])
        row += n
    again = harness.synthetic_pair_batch(2, 3, pairs, height=32, width=48, tokens=7, seed=5, max_targets=3)
    assert torch.equal(again[0].tensors, samples.tensors) and torch.equal(again[1]["input_ids"], tok["input_ids"])


def test_synthetic_pair_batch_counts_use_every_image_and_caption():
    from toist_amd import harness
    for B, T, P in ((8, 8, 8), (4, 2, 8), (2, 4, 8), (1, 8, 8), (2, 8, 16)):
        _, _, pi, pc, targets, _ = harness.synthetic_pair_batch(B, T, P, height=8, width=8, tokens=5, max_targets=1)
        assert pi.numel() == pc.numel() == len(targets) == P
        assert sorted(set(pi.tolist())) == list(range(B)) and sorted(set(pc.tolist())) == list(range(T))
        assert pi.tolist() == sorted(pi.tolist())                               # an image's pairs are consecutive
    _, _, pi, pc, _, _ = harness.synthetic_pair_batch(3, 3, 3, height=8, width=8, tokens=5, max_targets=1)
    assert list(zip(pi.tolist(), pc.tolist())) == [(0, 0), (1, 1), (2, 2)]       # P = B = T: the identity
    with pytest.raises(ValueError):
        harness.synthetic_pair_batch(2, 2, [(0, 2)], height=8, width=8, tokens=5)
    with pytest.raises(ValueError):
        harness.synthetic_pair_batch(2, 2, [], height=8, width=8, tokens=5)


def test_expand_pairs_builds_the_per_sample_batch():
    from toist_amd import harness
    from toist_amd.sweep import SweepTokenized
    pairs = [(1, 0), (1, 2), (0, 2), (1, 1), (1, 2)]
    batch = harness.synthetic_pair_batch(2, 3, pairs, height=16, width=24, tokens=6, seed=9, max_targets=2)
    samples, tok, pi, pc, targets, pmap = batch
    ex_samples, ex_tok, ex_targets, ex_pmap = harness.expand_pairs(*batch)
    assert tuple(ex_samples.tensors.shape) == (5, 3, 16, 24) and tuple(ex_samples.mask.shape) == (5, 16, 24)
    assert isinstance(ex_tok, SweepTokenized) and tuple(ex_tok["input_ids"].shape) == (5, 6)
    for p, (i, t) in enumerate(pairs):
        assert torch.equal(ex_samples.tensors[p], samples.tensors[i]) and torch.equal(ex_samples.mask[p], samples.mask[i])
        assert torch.equal(ex_tok["input_ids"][p], tok["input_ids"][t]) and torch.equal(ex_tok["attention_mask"][p], tok["attention_mask"][t])
    assert ex_targets is targets and ex_pmap is pmap
    assert not torch.equal(samples.tensors[0], samples.tensors[1]) and not torch.equal(tok["input_ids"][0], tok["input_ids"][2])


def _cpu_model(**over):
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    return toist_amd.build_model(harness.default_args(device="cpu", enc_layers=1, dec_layers=1, num_queries=4, **over))


def test_encode_pairs_refuses_cpu_tensors_and_backward_cuts():
    from toist_amd import harness
    model = _cpu_model()[0]
    samples, tok, pi, pc, _, _ = harness.synthetic_pair_batch(1, 2, 2, height=64, width=64, tokens=6, max_targets=0)
    for mode in (model.eval, model.train):                                     # unlike the sweep, grad and train() are no reason to refuse
        mode()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.encode_pairs(samples, tok, pi, pc)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        model.encode_pairs(samples, tok, pi, pc)
    with pytest.raises(RuntimeError, match="inference only"):                   # the task sweep keeps its own refusal, in its own words
        model.encode_sweep(samples, tok)
    model.split_backward = True
    try:
        with pytest.raises(RuntimeError, match="backward cuts"):
            model.encode_pairs(samples, tok, pi, pc)
    finally:
        del model.split_backward


def test_mask_head_model_refuses_encode_pairs_with_its_own_message():
    from toist_amd.segmentation import DETRsegm
    assert DETRsegm.encode_pairs is not DETRsegm._no_sweep
    with pytest.raises(NotImplementedError, match="shared-image training with a mask head"):
        DETRsegm.encode_pairs(None)
    with pytest.raises(NotImplementedError, match="task sweep with a mask head"):          # the sweep's message is untouched
        DETRsegm.encode_sweep(None)


def test_captured_pair_train_step_constructor_errors():
    from toist_amd import harness
    model, criterion, _, weight_dict = _cpu_model()
    mk = lambda **kw: harness.CapturedPairTrainStep(model, criterion, None, weight_dict, **{"batch": 2, "captions": 3, "pairs": 4, **kw})
    for bad in ({"batch": 0}, {"captions": 0}, {"pairs": 0}, {"pairs": -1}):
        with pytest.raises(ValueError):
            mk(**bad)
    with pytest.raises(TypeError):
        harness.CapturedPairTrainStep(model, criterion, None, weight_dict, batch=2, captions=3)          # pairs is required
    with_masks = SimpleNamespace(losses=["labels", "boxes", "masks"])
    with pytest.raises(ValueError, match="mask losses"):
        harness.CapturedPairTrainStep(model, with_masks, None, weight_dict, batch=2, captions=3, pairs=4)

    def refuse(*a, **k):
        raise NotImplementedError("mask head")

    with pytest.raises(NotImplementedError):
        harness.CapturedPairTrainStep(SimpleNamespace(detr=model, encode_pairs=refuse), criterion, None, weight_dict, batch=2, captions=3, pairs=4)
    cap = mk()
    assert (cap.batch, cap.captions, cap.pairs, cap.captures, cap.replays) == (2, 3, 4, 0, 0)


def test_captured_pair_train_step_checks_a_batch_on_the_host():
    """Every refusal of step() comes before anything is uploaded or launched: on a host without a device they are all that happens."""
    from toist_amd import harness, kernels
    model, criterion, _, weight_dict = _cpu_model()
    cap = harness.CapturedPairTrainStep(model, criterion, None, weight_dict, batch=2, captions=3, pairs=4)
    seed_word = kernels.SEED_DEV
    good = [(0, 0), (1, 2), (1, 1), (0, 2)]
    batch = lambda B=2, T=3, pairs=good: harness.synthetic_pair_batch(B, T, pairs, height=32, width=32, tokens=6, max_targets=2)
    with pytest.raises(ValueError, match="exactly 4 pairs"):
        cap.step(*batch(pairs=good[:3]))
    with pytest.raises(ValueError, match="exactly 4 pairs"):
        cap.step(*batch(pairs=good + [(0, 0)]))
    with pytest.raises(ValueError, match="2 images and 3 captions"):
        cap.step(*batch(B=3))
    with pytest.raises(ValueError, match="2 images and 3 captions"):
        cap.step(*batch(T=2, pairs=[(0, 0), (1, 1), (1, 0), (0, 1)]))
    samples, tok, pi, pc, targets, pmap = batch()
    for bad_i, bad_c in (([0, 2, 1, 0], pc), ([0, -1, 1, 0], pc), (pi, [0, 3, 1, 2]), (pi, [0, -1, 1, 2])):
        with pytest.raises(ValueError, match="outside"):
            cap.step(samples, tok, bad_i, bad_c, targets, pmap)
    with pytest.raises(ValueError, match="target dicts"):
        cap.step(samples, tok, pi, pc, targets[:3], pmap)
    assert cap.captures == 0 and cap.replays == 0 and not cap._buckets and kernels.SEED_DEV is seed_word      # nothing was built


def test_sweep_assemble_bwd_is_declared_exported_and_bound():
    from toist_amd import _lib
    with open(os.path.join(ROOT, "include", "toist_hip.h")) as f:
        header = f.read()
    assert len(re.findall(r"TOIST_API\s+int\s+toist_sweep_assemble_bwd\s*\(", header)) == 1
    assert len(re.findall(r"TOIST_API\s+int\s+toist_sweep_assemble\s*\(", header)) == 1
    with open(os.path.join(ROOT, "toist_amd", "csrc", "exports.map")) as f:
        assert re.search(r"global:\s*toist_\*;", f.read())
    p, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["toist_sweep_assemble_bwd"] == [p, p, p, i32, i32, i32, i32, i32, i32, p, p, p]
    fn = _lib.lib().toist_sweep_assemble_bwd
    assert list(fn.argtypes) == _lib.SIGNATURES["toist_sweep_assemble_bwd"] and fn.restype is ctypes.c_int
    # the host side of the entry point refuses bad extents before any launch: (d_seq, pair_image, pair_caption, P, B, HW, T, L, D, d_img, d_txt, stream)
    assert fn(None, None, None, 1, 1, 1, 1, 1, 12, None, None, None) != _lib.TOIST_OK and "multiple of 8" in _lib.last_error()
    assert fn(None, None, None, 1, 0, 1, 1, 1, 8, None, None, None) != _lib.TOIST_OK and "bad extents" in _lib.last_error()
    assert fn(None, None, None, -1, 1, 1, 1, 1, 8, None, None, None) != _lib.TOIST_OK and "bad extents" in _lib.last_error()
    assert fn(None, None, None, 4, 1, 1 << 30, 1, 1 << 30, 8, None, None, None) != _lib.TOIST_OK and "2^31" in _lib.last_error()
    assert fn(None, None, None, 1, 1, 1, 1, 1, 8, None, None, None) == _lib.TOIST_OK          # both outputs null: both sides frozen, nothing to do
    odd = ctypes.c_void_p(24)                                                               # (never dereferenced: the checks below refuse first)
    assert fn(None, None, None, 1, 1, 1, 1, 1, 8, odd, None, None) != _lib.TOIST_OK and "null pointer" in _lib.last_error()
    assert fn(None, None, None, 0, 1, 1, 1, 1, 8, odd, None, None) != _lib.TOIST_OK and "16-byte aligned" in _lib.last_error()
