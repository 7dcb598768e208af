"""Host side of the scored task sweep (coco_eval.StagedGroundTruth, row_tables, update_rows' Mailbox bookkeeping, SweepEvaluator.summarize): the
staged tables against CocoGroundTruth.annotations, the per-batch offsets, what is refused before a device is touched, the new C-ABI entry, and
the order in which queued match tables become records -- with the module-level event type stubbed, as tests/test_cpu_staging.py does."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ann(n, img, box, crowd=0, cat=1, area=None):
    return {"id": n, "image_id": img, "category_id": cat, "iscrowd": crowd, "bbox": [float(v) for v in box],
            "area": float(box[2] * box[3] if area is None else area)}


def _three_tasks():
    """Three tasks over images 11, 12, 13: task "b" does not know image 12 at all, image 13 has no annotations in "a" and "c", one annotation is
    of another category, one is a crowd, one carries an area that is not w * h."""
    imgs = lambda ids: [{"id": i, "height": 100, "width": 120} for i in ids]
    a = {"images": imgs([11, 12, 13]), "annotations": [_ann(1, 12, (1, 2, 30, 40)), _ann(2, 11, (5, 5, 10, 10), crowd=1), _ann(3, 12, (0, 0, 7, 9), cat=2),
                                                        _ann(4, 12, (50, 60, 20.5, 10.25), area=123.0), _ann(5, 11, (2, 3, 4, 5))]}
    b = {"images": imgs([13, 11]), "annotations": [_ann(1, 11, (9, 9, 9, 9)), _ann(2, 13, (1, 1, 2, 2)), _ann(3, 13, (3, 3, 4, 4), crowd=1)]}
    c = {"images": imgs([11, 12, 13]), "annotations": []}
    return {"a": a, "b": b, "c": c}


def test_staged_ground_truth_tables_follow_annotations():
    from toist_amd.coco_eval import CocoGroundTruth, StagedGroundTruth
    gts = [CocoGroundTruth(d) for d in _three_tasks().values()]
    st = StagedGroundTruth(gts, "cpu")
    assert st.slot_off.dtype == torch.int64 and st.gt_xywh.dtype == torch.float64 and st.gt_area.dtype == torch.float64 and st.gt_crowd.dtype == torch.uint8
    assert st.slot_sizes[0] == 0 and st.slot_off[0] == 0 and st.slot_off.numel() == st.slot_sizes.size + 1
    assert np.array_equal(st.slot_off.numpy(), np.concatenate([[0], np.cumsum(st.slot_sizes)]))
    assert st.n_gt == 7 and int(st.slot_off[-1]) == 7 and tuple(st.gt_xywh.shape) == (7, 4)
    seen = set()
    for t, gt in enumerate(gts):
        for img in (11, 12, 13, 99):
            (s,) = st.slots([(t, img)]).tolist()
            anns = gt.annotations(img, (1,))
            known = img in gt.img_anns
            assert (s != 0) == known, (t, img)                             # an image the ground truth does not know: the shared empty slot
            if known:
                assert s not in seen                                       # an image without annotations still owns a slot
                seen.add(s)
            lo, hi = int(st.slot_off[s]), int(st.slot_off[s + 1])
            assert hi - lo == len(anns) == st.slot_sizes[s]
            assert st.gt_xywh[lo:hi].tolist() == [a["bbox"] for a in anns]                       # annotation order is annotations()'s
            assert st.gt_area[lo:hi].tolist() == [a["area"] for a in anns]
            assert st.gt_crowd[lo:hi].tolist() == [a["iscrowd"] for a in anns]
    assert len(seen) == 3 + 2 + 3 and st.slot_sizes.size == 1 + 8
    # the category filter, the crowd flag and the annotation's own area made it through
    (s,) = st.slots([(0, 12)]).tolist()
    assert st.slot_sizes[s] == 2 and st.gt_area[int(st.slot_off[s]) + 1] == 123.0
    assert st.slots([(1, 12), (0, 13), (2, 11), (1, 13)]).tolist()[0] == 0 and st.slots([]).size == 0
    # one ground truth passed bare, and a ground truth without any annotation (the tables keep one padding entry no slot names)
    one = StagedGroundTruth(_three_tasks()["c"], "cpu")
    assert one.n_gt == 0 and one.slot_sizes.tolist() == [0, 0, 0, 0] and one.gt_area.numel() == 1 and one.slot_off.tolist() == [0] * 5


def test_row_tables_offsets_and_the_slot_check():
    from toist_amd.coco_eval import row_tables
    sizes = np.array([0, 3, 0, 5, 1])
    row_slot, iou_off, gt_off = row_tables([3, 0, 1, 1, 4, 2], sizes, 7)
    assert row_slot.dtype == np.int32 and iou_off.dtype == np.int64 and gt_off.dtype == np.int64
    assert row_slot.tolist() == [3, 0, 1, 1, 4, 2]
    assert gt_off.tolist() == [0, 5, 5, 8, 11, 12, 12] and iou_off.tolist() == [7 * g for g in gt_off.tolist()]
    empty = row_tables([], sizes, 7)
    assert empty[0].size == 0 and empty[1].tolist() == [0] and empty[2].tolist() == [0]
    with pytest.raises(ValueError, match="row 2: slot 5"):
        row_tables([0, 4, 5], sizes, 7)
    with pytest.raises(ValueError, match="row 0: slot -1"):
        row_tables([-1], sizes, 7)


def test_what_is_refused_before_a_device_is_touched():
    from toist_amd import kernels
    from toist_amd.coco_eval import TDODCocoEvaluator, _RowScorer, StagedGroundTruth
    R, Q = 2, 5
    z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype)
    with pytest.raises(RuntimeError, match="no CPU path"):
        kernels.coco_boxes(z(R, Q, dtype=torch.float32), z(R, Q, 4, dtype=torch.float32), 100, z(R, dtype=torch.int32), z(2, dtype=torch.int64), z(1, 4), z(1),
                           z(1, dtype=torch.uint8), z(R + 1, dtype=torch.int64), z(R + 1, dtype=torch.int64), 0, 0)
    ev = object.__new__(TDODCocoEvaluator)                                 # (the constructor needs a GPU; the refusal reads iou_types alone)
    ev.iou_types = ["bbox", "segm"]
    with pytest.raises(ValueError, match="bbox"):
        ev.update_rows({}, [1])
    ev.iou_types = ["segm"]
    with pytest.raises(ValueError, match="bbox"):
        ev.update_rows({}, [1])
    # host rows: the slot check first, then "no CPU path" -- nothing is launched
    scorer = _RowScorer(StagedGroundTruth(_three_tasks()["a"], "cpu"), "cpu")
    out = {"scores": z(R, Q, dtype=torch.float32), "boxes": z(R, Q, 4, dtype=torch.float32)}
    with pytest.raises(ValueError, match="slot 4"):
        scorer.score(out, np.array([1, 4]), [(None, 11), (None, 12)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        scorer.score(out, np.array([1, 3]), [(None, 11), (None, 12)])
    with pytest.raises(ValueError, match="3 rows"):
        scorer.score(out, np.array([1, 3, 0]), [(None, 11), (None, 12), (None, 13)])


def test_the_new_entry_is_declared_exported_and_checks_its_capacity():
    from toist_amd import _lib, kernels
    header = open(os.path.join(ROOT, "include", "toist_hip.h")).read()
    assert "toist_coco_boxes" in set(re.findall(r"\b(toist_[a-z0-9_]+)\s*\(", header))
    exports = open(os.path.join(ROOT, "toist_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"global:\s*([^;]+);", exports)
    assert any(re.fullmatch(g.strip().replace("*", ".*"), "toist_coco_boxes") for g in globs)
    handle = _lib.lib()
    assert "toist_coco_boxes" in _lib.exported_symbols() and hasattr(handle, "toist_coco_boxes")
    assert len(_lib.SIGNATURES["toist_coco_boxes"]) == 23
    assert kernels.COCO_BOXES_MAX_Q == _lib.CONSTANTS["TOIST_COCO_BOXES_MAX_Q"] >= 1024
    # the unit is built without contraction, as its neighbours that restate host arithmetic are
    assert re.search(r"evalbox\.hip\.o: FLAGS \+= -ffp-contract=off", open(os.path.join(ROOT, "toist_amd", "csrc", "Makefile")).read())
    # refused on the host, before any launch: more queries than the kernel ranks in LDS, bad extents, null tables; no rows = nothing to do
    args = lambda R, Q: (None, None, R, Q, 100, None, None, 1, None, None, None, 0, None, None, 0, 0, None, None, None, None, None, None, None)
    assert handle.toist_coco_boxes(*args(1, kernels.COCO_BOXES_MAX_Q + 1)) != 0 and "capacity" in _lib.last_error()
    assert handle.toist_coco_boxes(*args(-1, 5)) != 0 and "bad extents" in _lib.last_error()
    assert handle.toist_coco_boxes(*args(1, 5)) != 0 and "null table" in _lib.last_error()
    assert handle.toist_coco_boxes(*args(0, 5)) == 0


class _Device(torch.Tensor):
    """A host tensor that says it is on the device: what Mailbox.post asks before it copies."""
    is_cuda = True


def _events(monkeypatch, arrived):
    """staging.Event -> numbered stand-ins whose query() answers `n in arrived`; pinned memory -> ordinary memory; no capture."""
    from toist_amd import staging
    made = []

    class Event:
        def __init__(self):
            self.n = len(made)
            made.append(self)

        def record(self):
            pass

        def synchronize(self):
            pass

        def query(self):
            return self.n in arrived
    monkeypatch.setattr(staging, "Event", Event)
    monkeypatch.setattr(staging, "_capturing", lambda: False)
    monkeypatch.setattr(staging, "torch", types.SimpleNamespace(empty=lambda shape, dtype=None, pin_memory=False: torch.empty(shape, dtype=dtype)))


def _packed(rows, D, seed):
    """One batch's tables as the device packs them (random content of the right sizes) -> (the uint8 'device' tensor, its parts)."""
    A, T, R = 4, 10, len(rows)
    rng = np.random.default_rng(seed)
    G = sum(g for _, _, g in rows)
    scores = rng.random(R * D)
    dt_match = rng.integers(-1, 3, A * T * R * D).astype(np.int32)
    dt_ignore = rng.integers(0, 2, A * T * R * D).astype(np.uint8)
    gt_flag = rng.integers(0, 2, A * G).astype(np.uint8)
    raw = np.concatenate([scores.view(np.uint8), dt_match.view(np.uint8), dt_ignore, gt_flag])
    return torch.from_numpy(raw).as_subclass(_Device), (scores, dt_match, dt_ignore, gt_flag)


def test_queued_tables_become_records_in_posting_order_and_the_first_evaluation_wins(monkeypatch):
    from toist_amd.coco_eval import IouTypeEval, StagedGroundTruth, _RowScorer
    arrived = set()
    scorer = _RowScorer(StagedGroundTruth(_three_tasks()["c"], "cpu"), "cpu")
    _events(monkeypatch, arrived)                                                     # (after the tables are laid out: the stub leaves staging no torch)
    ev_a, ev_b = IouTypeEval("bbox"), IouTypeEval("bbox")
    ev_a.drain = ev_b.drain = scorer.drain
    D = 3
    rows1 = [(ev_a, 11, 2), (ev_b, 11, 0), (ev_a, 12, 1), (ev_a, 11, 2)]            # image 11 twice for task a inside one batch
    rows2 = [(ev_a, 12, 1), (ev_b, 13, 4)]                                            # image 12 again, one batch later
    rows3 = [(ev_b, 11, 0)]
    p1, (s1, m1, i1, f1) = _packed(rows1, D, 1)
    p2, (s2, m2, i2, f2) = _packed(rows2, D, 2)
    p3, _ = _packed(rows3, D, 3)
    for p, rows in ((p1, rows1), (p2, rows2), (p3, rows3)):
        scorer.post(p, (D, rows))
    assert len(scorer.mail) == 3 and not ev_a._records and not ev_b._records
    # the second batch has arrived, the first has not: nothing is filed out of order
    arrived.add(1)
    scorer.drain(wait=False)
    assert len(scorer.mail) == 3 and not ev_a._records
    arrived.add(0)
    scorer.drain(wait=False)
    assert len(scorer.mail) == 1 and len(scorer._meta) == 1
    assert sorted(ev_a._records) == [11, 12] and sorted(ev_b._records) == [11, 13]
    A, T = 4, 10
    rec = ev_a._records[11]                                                            # row 0 of batch 1, not row 3
    assert set(rec) == {"image_id", "scores", "dt_match", "dt_ignore", "gt_ignore"} and rec["image_id"] == 11
    assert rec["scores"].dtype == np.float64 and np.array_equal(rec["scores"], s1[:D])
    assert rec["dt_match"].dtype == np.int32 and np.array_equal(rec["dt_match"], m1[:A * T * D].reshape(A, T, D))
    assert rec["dt_ignore"].dtype == bool and np.array_equal(rec["dt_ignore"], i1[:A * T * D].reshape(A, T, D).astype(bool))
    assert rec["gt_ignore"].dtype == bool and np.array_equal(rec["gt_ignore"], f1[:A * 2].reshape(A, 2).astype(bool))
    rec = ev_a._records[12]                                                            # batch 1's row 2 won over batch 2's row 0
    assert np.array_equal(rec["scores"], s1[2 * D:3 * D]) and np.array_equal(rec["gt_ignore"], f1[A * 2:A * 3].reshape(A, 1).astype(bool))
    assert ev_b._records[11]["gt_ignore"].shape == (A, 0) and ev_b._records[11]["scores"].shape == (D,)
    rec = ev_b._records[13]                                                            # the second row of batch 2: its ground truth sits behind row 0's
    assert np.array_equal(rec["scores"], s2[D:2 * D]) and np.array_equal(rec["dt_match"], m2[A * T * D:].reshape(A, T, D))
    assert np.array_equal(rec["gt_ignore"], f2[A * 1:].reshape(A, 4).astype(bool))
    # a read of .records waits for what is left
    first = ev_b._records[11]
    assert ev_b.records[11] is first and len(scorer.mail) == 0 and not scorer._meta
    # a batch whose byte count does not match its bookkeeping is an error, not a mis-sliced record
    scorer.post(p3, (D, rows2))
    with pytest.raises(RuntimeError, match="bytes arrived"):
        scorer.drain()
    # a host tensor is not queued: update_rows says so instead of losing the batch
    with pytest.raises(RuntimeError, match="could not be queued"):
        scorer.post(torch.zeros(4, dtype=torch.uint8), (D, []))


def test_sweep_evaluator_summarize_means():
    from toist_amd.coco_eval import SweepEvaluator
    stats = {"cut": np.arange(12, dtype=np.float64) / 20, "sit": np.full(12, 0.5), "pour": -np.ones(12)}
    calls = []

    def stub(name):
        bbox = types.SimpleNamespace(stats=None)

        def summarize(verbose):
            calls.append((name, verbose))
            bbox.stats = stats[name]
        return types.SimpleNamespace(coco_eval={"bbox": bbox}, summarize=summarize)
    sw = object.__new__(SweepEvaluator)                                    # (the constructor builds device evaluators)
    sw.evaluators = {name: stub(name) for name in stats}
    got = sw.summarize()
    assert calls == [("cut", False), ("sit", False), ("pour", False)]
    assert list(got["tasks"]) == ["cut", "sit", "pour"] and all(got["tasks"][n] is stats[n] for n in stats)
    assert got["mAP50"] == pytest.approx((0.05 + 0.5 - 1.0) / 3) and got["mAP"] == pytest.approx((0.0 + 0.5 - 1.0) / 3)
    assert set(got) == {"tasks", "mAP50", "mAP"}
