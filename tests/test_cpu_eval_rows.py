"""Host side of captured evaluation scored on the device (toist_coco_masks, coco_eval.mask_row_tables, StagedGroundTruth(planes=True),
update_rows(masks=), harness.evaluate(score_rows=True)): the C-ABI entry and what it refuses before a launch, the per-batch mask tables against a
plain-Python restatement with every refusal, and what is refused before a device is touched."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared_exported_and_built_without_contraction():
    from toist_amd import _lib, kernels
    header = open(os.path.join(ROOT, "include", "toist_hip.h")).read()
    assert "toist_coco_masks" in set(re.findall(r"\b(toist_[a-z0-9_]+)\s*\(", header))
    exports = open(os.path.join(ROOT, "toist_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"global:\s*([^;]+);", exports)
    assert any(re.fullmatch(g.strip().replace("*", ".*"), "toist_coco_masks") for g in globs)
    handle = _lib.lib()
    assert "toist_coco_masks" in _lib.exported_symbols() and hasattr(handle, "toist_coco_masks")
    proto = re.search(r"TOIST_API int toist_coco_masks\((.*?)\);", header, re.S).group(1)
    assert len(_lib.SIGNATURES["toist_coco_masks"]) == len(proto.split(",")) == 22
    chunk = _lib.CONSTANTS["TOIST_COCO_MASKS_CHUNK_WORDS"]
    assert kernels.COCO_MASKS_CHUNK_WORDS == chunk and chunk >= 256 and chunk % 256 == 0 and 8 * chunk < 64 * 1024      # a chunk sits in static LDS
    assert re.search(r"evalrows\.hip\.o: FLAGS \+= -ffp-contract=off", open(os.path.join(ROOT, "toist_amd", "csrc", "Makefile")).read())


def test_the_entry_refuses_on_the_host_before_any_launch():
    from toist_amd import _lib
    handle = _lib.lib()
    # (bits, capacity_words, row_hw, R, Q, D, order, row_slot, slot_off, n_slots, gt_bits, gt_words, gt_plane_off, slot_hw, gt_parea, gt_crowd, n_gt,
    #  iou_off, iou_cap, dt_area, iou, stream) -- every pointer null: nothing can be launched
    args = lambda R=1, Q=5, D=5, cap=16, slots=1, gt_words=0, n_gt=0, iou_cap=0: (None, cap, None, R, Q, D, None, None, None, slots, None, gt_words, None,
                                                                                    None, None, None, n_gt, None, iou_cap, None, None, None)
    assert handle.toist_coco_masks(*args()) != 0 and "null table" in _lib.last_error()
    for bad in (dict(R=-1), dict(Q=-1, D=-1), dict(D=-1), dict(cap=-1), dict(slots=0), dict(gt_words=-1), dict(n_gt=-1), dict(iou_cap=-1)):
        assert handle.toist_coco_masks(*args(**bad)) != 0 and "bad extents" in _lib.last_error(), bad
    assert handle.toist_coco_masks(*args(Q=5, D=6)) != 0 and "kept detections" in _lib.last_error()
    assert handle.toist_coco_masks(*args(R=0, Q=5, D=6)) != 0                      # D > Q is refused whatever the row count
    assert handle.toist_coco_masks(*args(R=0)) == 0                               # no rows: nothing to do


def _plain_tables(slots, slot_sizes, D):
    iou_off, total = [0], 0
    for s in slots:
        total += D * int(slot_sizes[s])
        iou_off.append(total)
    return iou_off


def test_mask_row_tables_against_a_restatement_and_every_refusal():
    from toist_amd.coco_eval import MAX_DETS, mask_row_tables
    rng = np.random.default_rng(3)
    S = 9
    slot_sizes = np.array([0] + rng.integers(0, 6, S - 1).tolist())
    slot_sizes[3], slot_sizes[5] = 0, 4
    slot_hw = np.stack([rng.integers(1, 300, S), rng.integers(1, 300, S)], axis=1).astype(np.int32)
    slot_hw[0] = 0
    slots = [5, 0, 3, 1, 8, 5, 2]
    row_hw = [tuple(int(v) for v in slot_hw[s]) for s in slots]
    row_hw[1], row_hw[2] = (17, 4), (64, 9)                                      # rows without ground truth may be of any size
    for Q in (1, 7, 100, 130):
        D = min(Q, MAX_DETS[-1])
        need = max(Q * w * ((h + 63) // 64) for h, w in row_hw)
        row_slot, iou_off, hw = mask_row_tables(slots, slot_sizes, slot_hw, row_hw, Q, need)
        assert row_slot.dtype == np.int32 and iou_off.dtype == np.int64 and hw.dtype == np.int64 and hw.shape == (len(slots), 2)
        assert row_slot.tolist() == slots and hw.tolist() == [list(p) for p in row_hw]
        assert iou_off.tolist() == _plain_tables(slots, slot_sizes, D)
        # planes that overflow the capacity, by one word
        with pytest.raises(ValueError, match="capacity"):
            mask_row_tables(slots, slot_sizes, slot_hw, row_hw, Q, need - 1)
    Q, cap = 7, 7 * 300 * 5
    fewer = mask_row_tables(slots, slot_sizes, slot_hw, row_hw, Q, cap, D=3)
    assert fewer[1].tolist() == _plain_tables(slots, slot_sizes, 3)
    empty = mask_row_tables([], slot_sizes, slot_hw, [], Q, cap)
    assert empty[0].size == 0 and empty[1].tolist() == [0] and empty[2].shape == (0, 2)
    # a slot out of range
    for bad in (S, -1):
        with pytest.raises(ValueError, match=f"row 1: slot {bad}"):
            mask_row_tables([5, bad], slot_sizes, slot_hw, row_hw[:2], Q, cap)
    # a size mismatch on a row with ground truth: update()'s wording; the same mismatch on a row without is accepted
    h5, w5 = (int(v) for v in slot_hw[5])
    with pytest.raises(ValueError, match=rf"row 0: predicted masks are {h5 + 1}x{w5}, the ground truth is {h5}x{w5}"):
        mask_row_tables([5], slot_sizes, slot_hw, [(h5 + 1, w5)], Q, cap)
    with pytest.raises(ValueError, match="predicted masks are"):
        mask_row_tables([5], slot_sizes, slot_hw, [(w5, h5 + 1)], Q, cap)
    assert slot_sizes[3] == 0
    h3, w3 = (int(v) for v in slot_hw[3])
    assert mask_row_tables([3], slot_sizes, slot_hw, [(h3 + 1, w3)], Q, cap)[1].tolist() == [0, 0]
    # Q below D, sizes that are not positive, counts that leave 32 bits
    with pytest.raises(ValueError, match="8 kept detections of 7"):
        mask_row_tables([5], slot_sizes, slot_hw, [(h5, w5)], 7, cap, D=8)
    for hw in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ValueError, match="row 0: predicted masks of size"):
            mask_row_tables([0], slot_sizes, slot_hw, [hw], Q, cap)
    with pytest.raises(ValueError, match="predicted masks of size"):
        mask_row_tables([0], slot_sizes, slot_hw, [(1 << 16, 1 << 16)], 1, 1 << 40)
    with pytest.raises(ValueError, match="row sizes"):
        mask_row_tables([0, 0], slot_sizes, slot_hw, [(4, 4)], Q, cap)


def test_update_rows_without_masks_keeps_refusing_segm():
    from toist_amd.coco_eval import TDODCocoEvaluator
    ev = object.__new__(TDODCocoEvaluator)                                 # (the constructor needs a GPU; the refusals read iou_types alone)
    for types in (["segm"], ["bbox", "segm"]):
        ev.iou_types = types
        with pytest.raises(ValueError, match="bbox"):
            ev.update_rows({}, [1])
        with pytest.raises(ValueError, match="bbox"):
            ev.update_rows({}, [1], masks=None)
        with pytest.raises(TypeError, match="RowMasks"):
            ev.update_rows({}, [1], masks=object())
    ev.iou_types = ["keypoints"]
    with pytest.raises(ValueError, match="segm"):
        ev.update_rows({}, [1], masks=object())


def test_segm_rows_need_masks_and_staged_planes_before_a_device_is_touched():
    from toist_amd.coco_eval import RowMasks, StagedGroundTruth, _RowScorer
    data = {"images": [{"id": 11, "height": 70, "width": 5}], "annotations": []}
    out = {"scores": torch.zeros(1, 5), "boxes": torch.zeros(1, 5, 4)}
    plain = _RowScorer(StagedGroundTruth(data, "cpu"), "cpu")
    masks = RowMasks(torch.zeros(5 * 5 * 2, dtype=torch.int64), 50, torch.tensor([[70, 5]]), [(70, 5)])
    with pytest.raises(ValueError, match="planes"):
        plain.score(out, np.array([1]), [({}, 11)], masks=masks, types=("bbox", "segm"))
    staged = StagedGroundTruth(data, "cpu", planes=True)
    assert staged.has_planes and staged.plane_bytes == 0 and staged.slot_hw_host.tolist() == [[0, 0], [70, 5]]
    assert staged.slot_hw.dtype == torch.int32 and staged.gt_plane_off.dtype == torch.int64 and staged.gt_plane_off.tolist() == [0, 0]
    scorer = _RowScorer(staged, "cpu")
    with pytest.raises(ValueError, match="masks=RowMasks"):
        scorer.score(out, np.array([1]), [({}, 11)], types=("segm",))
    masks.capacity_words = 49                                                # the host check of the planes comes before "no CPU path"
    with pytest.raises(ValueError, match="capacity is 49"):
        scorer.score(out, np.array([1]), [({}, 11)], masks=masks, types=("segm",))
    masks.capacity_words = 50
    with pytest.raises(RuntimeError, match="no CPU path"):
        scorer.score(out, np.array([1]), [({}, 11)], masks=masks, types=("segm",))
    with pytest.raises(ValueError, match="2 rows of planes, 1 sizes"):
        RowMasks.pack([torch.zeros(1, 5, 2, dtype=torch.int64)] * 2, [(70, 5)])
    with pytest.raises(ValueError, match="for a row of size 70x6"):
        RowMasks.pack([torch.zeros(1, 5, 2, dtype=torch.int64)], [(70, 6)])
    packed = RowMasks.pack([torch.ones(2, 5, 2, dtype=torch.int64), torch.ones(2, 3, 1, dtype=torch.int64)], [(70, 5), (64, 3)])
    assert packed.capacity_words == 20 and packed.bits.numel() == 40 and packed.hw_host == [(70, 5), (64, 3)] and packed.hw_dev.tolist() == [[70, 5], [64, 3]]
    assert packed.bits.tolist() == [1] * 20 + [1] * 6 + [0] * 14


def test_evaluate_with_score_rows_needs_a_captured_step_and_row_evaluators():
    from toist_amd import harness

    class Model:
        def eval(self):
            raise AssertionError("refused before the model is touched")
    with pytest.raises(ValueError, match="captured"):
        harness.evaluate(Model(), None, None, {}, {}, [], [], "cpu", None, score_rows=True)

    class Step:
        def step_rows(self, *a, **k):
            raise AssertionError("refused before a step")
    with pytest.raises(ValueError, match="TDODCocoEvaluator"):
        harness.evaluate(Model(), None, None, {}, {}, [], [object()], "cpu", None, captured=Step(), score_rows=True)


def test_staged_planes_are_sized_before_they_are_allocated(monkeypatch):
    from toist_amd import coco_eval as C
    anns = [{"id": n + 1, "image_id": 11 + n % 2, "category_id": 1, "iscrowd": 0, "bbox": [0.0, 0.0, 2.0, 2.0], "area": 4.0,
             "segmentation": np.ones((130 if n % 2 == 0 else 64, 7), dtype=bool)} for n in range(5)]
    data = {"images": [{"id": 11, "height": 130, "width": 7}, {"id": 12, "height": 64, "width": 7}, {"id": 13, "height": 9, "width": 9}], "annotations": anns}
    gt = C.CocoGroundTruth(data)

    def no_planes(*a, **k):
        raise AssertionError("planes were built before the size check")
    monkeypatch.setattr(C.CocoGroundTruth, "planes", no_planes)
    monkeypatch.setattr(C.torch, "empty", no_planes)
    need = 8 * (3 * 7 * 3 + 2 * 7 * 1)
    for limit in (1, need - 1):
        with pytest.raises(ValueError, match=rf"take {need} bytes, above max_plane_bytes = {limit}\b"):
            C.StagedGroundTruth(gt, "cpu", planes=True, max_plane_bytes=limit)
    # the layout itself: three planes of 21 words, then two of 7 (annotation order is annotations()'s, slot by slot)
    st = object.__new__(C.StagedGroundTruth)
    st.slot_sizes = np.array([0, 3, 2, 0])
    hw, off = st._plane_layout([None, (gt, 11), (gt, 12), (gt, 13)], 5)
    assert hw.tolist() == [[0, 0], [130, 7], [64, 7], [9, 9]] and off.tolist() == [0, 21, 42, 63, 70, 77]
    # the default stays what it was: no planes, no new tables
    monkeypatch.undo()
    plain = C.StagedGroundTruth(gt, "cpu")
    assert not plain.has_planes and plain.plane_bytes == 0 and not hasattr(plain, "gt_bits") and not hasattr(plain, "slot_hw")
