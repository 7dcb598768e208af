"""A task sweep scored on the device: toist_coco_boxes (csrc/evalbox.hip) on synthetic rows against torch's device sort, numpy's fp32 / fp64
arithmetic and oracle/coco_ref.bb_iou (exact); TDODCocoEvaluator.update_rows / SweepEvaluator against update() on the same rows (records equal byte
for byte) and against oracle/coco_ref.CocoEvalRef (the 12 stats, exact); one launch replayed from a hipGraph after its tables changed; and
harness.evaluate_sweep(evaluator=) over a captured and an eager sweep of a tiny model against per-task evaluators fed by update().
(The file sorts behind every other GPU test file on purpose: DESIGN 8 item 6.  No training step is built here.)"""
import numpy as np
import pytest
import torch

from oracle import coco_ref as R

pytestmark = pytest.mark.gpu

SLOT_G = (5, 33, None, 0, 1)          # ground-truth boxes of the images a batch cycles over; None = an image id the ground truth does not know
MAX_DET = 100


def _dataset(rng, sizes=SLOT_G, first_id=100):
    """A COCO-format ground truth with one image per entry of `sizes` (None: no such image) -> (dataset, image ids, one per entry)."""
    images, anns, ids = [], [], []
    for n, G in enumerate(sizes):
        img = first_id + n
        ids.append(img)
        if G is None:
            continue
        images.append({"id": img, "height": 480, "width": 640})
        for g in range(G):
            x, y = (float(v) for v in rng.integers(0, 300, 2))
            w, h = (float(v) for v in rng.integers(8, 200, 2))
            if g % 7 == 3:
                x, w = x + 0.1, w + 0.2                                    # coordinates that are not fp32 numbers
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "iscrowd": int(g % 5 == 4), "bbox": [x, y, w, h],
                         "area": w * h if g % 3 else float(rng.integers(100, 40000))})      # small / medium / large, not always w * h
    return {"images": images, "annotations": anns}, ids


def _rows(rng, dataset, row_images, Q, nan_row=None):
    """scores f32 [R, Q] and boxes f32 [R, Q, 4] on the host: coarse scores (many exact ties), a row of all-equal scores, -0.0 / 0.0, +-inf, one NaN
    (nan_row); boxes that are a ground-truth box, touch one (w == 0), lie apart, have zero area, are inverted, and whose fp32 width is not the
    fp64 difference of their corners."""
    R_ = len(row_images)
    scores = np.round(rng.random((R_, Q)), 1).astype(np.float32)
    boxes = np.empty((R_, Q, 4), dtype=np.float32)
    by_img = {}
    for a in dataset["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a["bbox"])
    for r, img in enumerate(row_images):
        gts = by_img.get(img, [])
        if r % 4 == 1:
            scores[r] = 0.5                                                # all equal: the order is the index order
        elif Q >= 7:
            scores[r, rng.integers(0, Q, 2)] = (-0.0, 0.0)
            scores[r, (r + 3) % Q], scores[r, (r + 5) % Q] = np.inf, -np.inf
        for q in range(Q):
            x, y = rng.integers(0, 300, 2) + rng.random(2)
            w, h = rng.integers(5, 200, 2) + rng.random(2)
            kind = (q + r) % 8
            if gts and kind < 5:
                gx, gy, gw, gh = gts[q % len(gts)]
                if kind == 0:
                    x, y, w, h = gx, gy, gw, gh                            # the ground-truth box itself
                elif kind == 1:
                    x, y, w, h = gx + gw, gy, 10.0, gh                     # touches it: the intersection is 0 wide
                elif kind == 2:
                    x, y, w, h = gx + gw + 50, gy + gh + 50, 10.0, 10.0    # apart
                elif kind == 3:
                    x, y, w, h = gx + 3, gy + 2, gw * 0.75, gh * 1.25      # overlaps
                else:
                    x, y, w, h = gx + gw / 2, gy + gh / 2, 0.0, gh         # zero area inside it
            elif kind == 5:
                w = -w                                                      # inverted
            boxes[r, q] = (x, y, x + w, y + h)
        boxes[r, 0] = (0.1, 0.2, 100.3, 50.7)                              # fp32 difference != fp64 difference of the widened corners
    if nan_row is not None:
        scores[nan_row, Q // 2] = np.nan
    return scores, boxes


def _expected_row(scores, boxes, anns):
    """What one row must give, from numpy and the oracle: (order, dt_score, dt_area, iou [D, G], gt_area, gt_crowd)."""
    order = torch.sort(torch.from_numpy(scores).double(), descending=True, stable=True).indices[:MAX_DET].numpy()
    b = boxes[order]
    w32, h32 = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]                        # fp32
    xywh = np.stack([b[:, 0], b[:, 1], w32, h32], axis=1).astype(np.float64)
    crowd = [int(a["iscrowd"]) for a in anns]
    iou = R.bb_iou(xywh.tolist(), [a["bbox"] for a in anns], crowd)
    return (order.astype(np.int32), scores[order].astype(np.float64), xywh[:, 2] * xywh[:, 3], iou,
            np.array([float(a["area"]) for a in anns], dtype=np.float64), np.array(crowd, dtype=np.uint8))


def _poisoned(n, dtype, dev, guard=64):
    """n elements + a guard region, every byte 0xFF (a NaN for doubles, -1 for int32) -> (the whole buffer, its first n elements)."""
    buf = torch.full((n + guard,), 0xFF, dtype=torch.uint8, device=dev).repeat_interleave(torch.empty(0, dtype=dtype).element_size()).view(dtype)
    return buf, buf[:n]


def _untouched(t):
    return bool((t.view(torch.uint8) == 0xFF).all())


def _written(t):
    """no element is still the poison pattern (elements, not bytes: a written -1.0 holds 0xFF bytes too)"""
    width = t.element_size()
    return bool((~(t.contiguous().view(torch.uint8).view(-1, width) == 0xFF).all(dim=1)).all()) if t.numel() else True


CASES = [(3, Q) for Q in (1, 7, 64, 65, 100, 101, 257, 300)] + [(1, 100), (112, 100), (112, 7)]


@pytest.mark.parametrize("R_,Q", CASES)
def test_coco_boxes_rows_against_numpy_and_the_oracle(dev, R_, Q):
    """One launch over R rows with mixed ground-truth sizes (0, 1, 5, 33 and the shared empty slot) into poisoned outputs: the order is torch's
    device and host sort, scores / areas / IoU blocks / ground-truth copies are exact, every element of every extent is written and the guard
    regions behind the outputs are not."""
    from toist_amd import coco_eval as C, kernels as k
    rng = np.random.default_rng(1000 * R_ + Q)
    dataset, ids = _dataset(rng)
    gt = C.CocoGroundTruth(dataset)
    st = C.StagedGroundTruth(gt, dev)
    row_images = [ids[(i + Q) % len(ids)] for i in range(R_)]
    scores, boxes = _rows(rng, dataset, row_images, Q, nan_row=2 if R_ == 3 else R_ // 2)       # (not an all-equal row)
    assert np.float64(boxes[0, 0, 2] - boxes[0, 0, 0]) != np.float64(boxes[0, 0, 2]) - np.float64(boxes[0, 0, 0])      # the fp32 case is live
    D = min(Q, MAX_DET)
    slots = st.slots([(0, i) for i in row_images])
    assert (slots == 0).sum() == sum(i == ids[2] for i in row_images)
    row_slot, iou_off, gt_off = C.row_tables(slots, st.slot_sizes, D)
    n_iou, n_gt = int(iou_off[-1]), int(gt_off[-1])
    d_scores, d_boxes = torch.from_numpy(scores).to(dev), torch.from_numpy(boxes).to(dev)
    bufs = {"order": _poisoned(R_ * D, torch.int32, dev), "dt_score": _poisoned(R_ * D, torch.float64, dev), "dt_area": _poisoned(R_ * D, torch.float64, dev),
            "iou": _poisoned(n_iou, torch.float64, dev), "gt_area": _poisoned(n_gt, torch.float64, dev), "gt_crowd": _poisoned(n_gt, torch.uint8, dev)}
    out = {name: view for name, (_, view) in bufs.items()}
    out["order"] = out["order"].view(R_, D)
    up = lambda a: torch.from_numpy(a).to(dev)
    got = k.coco_boxes(d_scores, d_boxes, MAX_DET, up(row_slot), st.slot_off, st.gt_xywh, st.gt_area, st.gt_crowd, up(iou_off), up(gt_off), n_iou, n_gt, out=out)
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        assert _untouched(whole[view.numel():]), f"{name}: the guard region was written"
        assert _written(view), f"{name}: an element of a row's extent was not written"
    dev_order = torch.sort(d_scores.double(), dim=1, descending=True, stable=True).indices[:, :D].cpu().numpy()
    assert np.array_equal(got["order"].cpu().numpy(), dev_order)          # the yardstick: update() sorts on the device
    h = {name: t.cpu().numpy() for name, t in got.items()}
    for r, img in enumerate(row_images):
        anns = gt.annotations(img, (1,))
        order, sc, area, iou, ga, gc = _expected_row(scores[r], boxes[r], anns)
        G = len(anns)
        assert np.array_equal(h["order"][r], order), r                    # the host's sort agrees
        assert h["dt_score"][r * D:(r + 1) * D].tobytes() == sc.tobytes(), r
        assert np.array_equal(h["dt_area"][r * D:(r + 1) * D], area), r
        assert np.array_equal(h["iou"][iou_off[r]:iou_off[r + 1]].reshape(D, G), iou), r
        assert np.array_equal(h["gt_area"][gt_off[r]:gt_off[r + 1]], ga) and np.array_equal(h["gt_crowd"][gt_off[r]:gt_off[r + 1]], gc), r
        if G and r < 8:                                                   # and the torch ops it replaces, on the device
            xywh = torch.from_numpy(np.concatenate([boxes[r][order][:, :2], (boxes[r][order][:, 2:] - boxes[r][order][:, :2])], axis=1)).double().to(dev)
            want = C._box_iou(xywh, torch.tensor([a["bbox"] for a in anns], dtype=torch.float64, device=dev), torch.from_numpy(gc).to(dev))
            assert torch.equal(got["iou"][iou_off[r]:iou_off[r + 1]].view(D, G), want), r
    if Q >= 7:
        assert (h["iou"] > 0).any() and (h["iou"] == 0).any()
    if Q >= 64:
        assert (h["iou"] == 1.0).any()


def _predictions(scores, boxes, row_images, dev):
    """update()'s input for the rows: the FIRST row of every image id (the first evaluation wins)."""
    pred = {}
    for r, img in enumerate(row_images):
        pred.setdefault(img, {"scores": torch.from_numpy(scores[r]).to(dev), "labels": torch.ones(scores.shape[1], dtype=torch.int64, device=dev),
                              "boxes": torch.from_numpy(boxes[r]).to(dev)})
    return pred


def _same_records(got, want, note):
    assert sorted(got, key=str) == sorted(want, key=str), note
    for img in want:
        g, w = got[img], want[img]
        assert list(g) == list(w) and g["image_id"] == w["image_id"], (note, img)
        for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
            assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape and g[key].tobytes() == w[key].tobytes(), (note, img, key)


@pytest.mark.parametrize("R_,Q", [(3, 7), (3, 101), (112, 100)])
def test_update_rows_files_the_records_of_update(dev, R_, Q):
    """TDODCocoEvaluator.update_rows on a batch of rows (an image id twice in it, one row on the empty slot, one NaN score) and a second batch that
    names an image of the first again, against update() on the same rows as dicts: records, img_ids and the accumulated tables are equal."""
    from toist_amd import coco_eval as C
    rng = np.random.default_rng(7 * R_ + Q)
    dataset, ids = _dataset(rng)
    first = [ids[i % len(ids)] for i in range(R_)]
    first[-1] = first[0]                                                  # the same image twice in one batch
    second = [ids[1], 999, ids[4]]                                        # evaluated before / unknown / (for R = 3) new
    ev, ctl = C.TDODCocoEvaluator(dataset, ["bbox"], device=dev), C.TDODCocoEvaluator(dataset, ["bbox"], device=dev)
    for n, row_images in enumerate((first, second)):
        scores, boxes = _rows(rng, dataset, row_images, Q, nan_row=0 if n == 0 else None)
        out = {"scores": torch.from_numpy(scores).to(dev), "boxes": torch.from_numpy(boxes).to(dev)}
        ev.update_rows(out, row_images)
        ctl.update(_predictions(scores, boxes, row_images, dev))
    assert ev.img_ids == ctl.img_ids
    _same_records(ev.coco_eval["bbox"].records, ctl.coco_eval["bbox"].records, (R_, Q))
    assert len(ev._scorer.mail) == 0
    # padding rows behind `live` are not scored
    scores, boxes = _rows(rng, dataset, [ids[0], ids[1]], Q)
    ev2 = C.TDODCocoEvaluator(dataset, ["bbox"], device=dev)
    ev2.update_rows({"scores": torch.from_numpy(scores).to(dev), "boxes": torch.from_numpy(boxes).to(dev)}, [ids[0], ids[1]], live=1)
    assert list(ev2.coco_eval["bbox"].records) == [ids[0]] and ev2.img_ids == [ids[0]]


def test_sweep_evaluator_matches_the_oracle_exactly(dev):
    """Three tasks over 8 images, 24 rows per batch in two batches through SweepEvaluator.update_rows: per task the precision table and the 12
    stats equal oracle/coco_ref.CocoEvalRef (exact, as test_evaluator_matches_oracle_exactly holds update()), and the means are the means."""
    from toist_amd import coco_eval as C
    from toist_amd.sweep import pair_tables
    rng = np.random.default_rng(5)
    names = ["cut", "sit", "pour"]
    sizes = {"cut": (5, 33, None, 0, 1, 2, 3, 4), "sit": (1, 0, 5, 5, None, 2, 0, 7), "pour": (2, 2, 2, 2, 2, 2, 2, 2)}
    data = {n: _dataset(rng, sizes[n])[0] for n in names}
    ids = list(range(100, 108))
    sw = C.SweepEvaluator(data, dev)
    res = {n: {} for n in names}
    for lo in (0, 4):
        pi, pc, live = pair_tables(4, 3, capacity=14)                     # two padded rows, as a captured bucket has
        Q = 20
        scores = np.zeros((14, Q), dtype=np.float32)
        boxes = np.zeros((14, Q, 4), dtype=np.float32)
        for p in range(live):
            img, name = ids[lo + pi[p]], names[pc[p]]
            scores[p], boxes[p] = (a[0] for a in _rows(rng, data[name], [img], Q))
            res[name][img] = {"scores": scores[p].copy(), "labels": np.ones(Q, dtype=np.int64), "boxes": boxes[p].copy()}
        sw.update_rows({"scores": torch.from_numpy(scores).to(dev), "boxes": torch.from_numpy(boxes).to(dev)}, ids[lo:lo + 4], names, pi, pc, live)
    sw.synchronize_between_processes()
    sw.accumulate()
    got = sw.summarize()
    for n in names:
        ref = R.CocoEvalRef(data[n]["annotations"], R.detections_from_results(_fp32_widths(res[n]), "bbox"), ids, "bbox")
        ref.evaluate()
        ref.accumulate()
        want = ref.summarize()
        ev = sw.evaluators[n]
        assert ev.img_ids == ids and sorted(ev.coco_eval["bbox"].records) == ids
        assert np.array_equal(ev.coco_eval["bbox"].eval["precision"][:, :, 0], ref.precision[:, :, 0]), n
        assert np.array_equal(got["tasks"][n], want), (n, got["tasks"][n], want)
    assert got["mAP50"] == float(np.mean([got["tasks"][n][1] for n in names])) and got["mAP"] == float(np.mean([got["tasks"][n][0] for n in names]))
    assert 0.0 < got["mAP"] < 1.0


def _fp32_widths(res):
    """The oracle forms x1 - x0 in double; the evaluator (like the reference's convert_to_xywh on fp32 tensors) forms it in fp32.  Hand the oracle
    boxes whose double difference IS the fp32 one: x1 := x0 + fp32(x1 - x0), exact in double."""
    out = {}
    for img, p in res.items():
        b = p["boxes"].astype(np.float64)
        w, h = (p["boxes"][:, 2] - p["boxes"][:, 0]).astype(np.float64), (p["boxes"][:, 3] - p["boxes"][:, 1]).astype(np.float64)
        b[:, 2], b[:, 3] = b[:, 0] + w, b[:, 1] + h
        assert np.array_equal(b[:, 2] - b[:, 0], w) and np.array_equal(b[:, 3] - b[:, 1], h)
        out[img] = {"scores": p["scores"], "labels": p["labels"], "boxes": b}
    return out


def test_one_captured_launch_serves_changed_rows_and_tables(dev):
    """toist_coco_boxes reads nothing from the host: one launch captured in a hipGraph, replayed after the rows, row_slot and the offsets changed
    on the device, gives what an eager launch on the new content gives -- inside fixed-capacity outputs whose tails stay untouched."""
    from toist_amd import coco_eval as C, kernels as k
    rng = np.random.default_rng(11)
    dataset, ids = _dataset(rng)
    st = C.StagedGroundTruth(dataset, dev)
    R_, Q = 6, 65
    D, cap = Q, 6 * 33
    bufs = {"order": _poisoned(R_ * D, torch.int32, dev), "dt_score": _poisoned(R_ * D, torch.float64, dev), "dt_area": _poisoned(R_ * D, torch.float64, dev),
            "iou": _poisoned(D * cap, torch.float64, dev, guard=0), "gt_area": _poisoned(cap, torch.float64, dev, guard=0),
            "gt_crowd": _poisoned(cap, torch.uint8, dev, guard=0)}
    out = {name: view for name, (_, view) in bufs.items()}
    out["order"] = out["order"].view(R_, D)
    d_scores, d_boxes = torch.zeros(R_, Q, device=dev), torch.zeros(R_, Q, 4, device=dev)
    d_slot = torch.zeros(R_, dtype=torch.int32, device=dev)
    d_iou, d_gt = torch.zeros(R_ + 1, dtype=torch.int64, device=dev), torch.zeros(R_ + 1, dtype=torch.int64, device=dev)
    launch = lambda o: k.coco_boxes(d_scores, d_boxes, MAX_DET, d_slot, st.slot_off, st.gt_xywh, st.gt_area, st.gt_crowd, d_iou, d_gt, D * cap, cap, out=o)
    launch(out)                                                           # (all rows on the empty slot) the module is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(out)
    for n, row_images in enumerate(([ids[0], ids[1], ids[2], ids[3], ids[4], ids[0]], [ids[1], ids[1], ids[4], ids[2], ids[1], ids[3]])):
        scores, boxes = _rows(rng, dataset, row_images, Q)
        row_slot, iou_off, gt_off = C.row_tables(st.slots([(0, i) for i in row_images]), st.slot_sizes, D)
        for dst, src in ((d_scores, scores), (d_boxes, boxes), (d_slot, row_slot), (d_iou, iou_off), (d_gt, gt_off)):
            dst.copy_(torch.from_numpy(src))
        for whole, _ in bufs.values():
            whole.view(torch.uint8).fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {name: t.clone() for name, t in out.items()}
        n_iou, n_gt = int(iou_off[-1]), int(gt_off[-1])
        assert _untouched(replayed["iou"][n_iou:]) and _untouched(replayed["gt_area"][n_gt:]) and _untouched(replayed["gt_crowd"][n_gt:]), n
        assert all(_untouched(whole[view.numel():]) for whole, view in bufs.values()), n
        eager = k.coco_boxes(d_scores, d_boxes, MAX_DET, d_slot, st.slot_off, st.gt_xywh, st.gt_area, st.gt_crowd, d_iou, d_gt, n_iou, n_gt)
        for name in ("order", "dt_score", "dt_area"):
            assert torch.equal(replayed[name].view(torch.uint8), eager[name].view(torch.uint8)), (n, name)
        for name, m in (("iou", n_iou), ("gt_area", n_gt), ("gt_crowd", n_gt)):
            assert _written(replayed[name][:m]) and torch.equal(replayed[name][:m].view(torch.uint8), eager[name].view(torch.uint8)), (n, name)
        assert n_iou > 0 and float(eager["iou"].max()) == 1.0


# ---- end to end: a tiny model's sweep, captured and eager --------------------------------------------------------------------------------
def _model(dev):
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    return toist_amd.build_model(harness.default_args(device="cuda", enc_layers=1, dec_layers=1, num_queries=10))[0].to(dev).eval()


def _inputs(n_images, n_captions, h, w, tokens, seed):
    from toist_amd import harness
    samples, _, _, _ = harness.synthetic_batch(n_images, h, w, tokens=tokens, seed=seed, max_targets=0)
    _, tok, _, _ = harness.synthetic_batch(n_captions, 32, 32, tokens=tokens, seed=seed + 100, max_targets=0)
    return samples, tok


def _ground_truth_from(keyed, names, image_ids):
    """Per task a ground truth cut from the model's own detections, so that there is something to match: the two best boxes of every (image,
    task), the second one shifted; task 0 does not know the last image, task 1 has no annotation on the first."""
    data = {}
    for t, name in enumerate(names):
        known = image_ids[:-1] if t == 0 else image_ids
        anns = []
        for img in known:
            if t == 1 and img == image_ids[0]:
                continue
            r = keyed[(img, name)]
            top = torch.sort(r["scores"].double(), descending=True, stable=True).indices[:2].tolist()
            for j, q in enumerate(top):
                x0, y0, x1, y1 = (float(v) for v in r["boxes"][q])
                w, h = max(x1 - x0, 1.0), max(y1 - y0, 1.0)
                anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "iscrowd": 0, "bbox": [x0 + 3.0 * j, y0, w, h], "area": w * h})
        data[name] = {"images": [{"id": i, "height": 131, "width": 170} for i in known], "annotations": anns}
    return data


def _control(per_batch_keyed, data, names, dev):
    """Per-task evaluators fed by update(), batch by batch, from cloned results."""
    from toist_amd import coco_eval as C
    evs = {n: C.TDODCocoEvaluator(data[n], ["bbox"], device=dev) for n in names}
    for keyed in per_batch_keyed:
        for n in names:
            evs[n].update({img: {k_: v.clone() for k_, v in r.items()} for (img, name), r in keyed.items() if name == n})
    stats = {}
    for n, ev in evs.items():
        ev.synchronize_between_processes()
        ev.accumulate()
        ev.summarize(verbose=False)
        stats[n] = ev.coco_eval["bbox"].stats
    return evs, stats


def _same_as_control(sw, got, evs, stats, names, note):
    for n in names:
        assert sw.evaluators[n].img_ids == evs[n].img_ids, (note, n)
        _same_records(sw.evaluators[n].coco_eval["bbox"].records, evs[n].coco_eval["bbox"].records, (note, n))
        assert np.array_equal(got["tasks"][n], stats[n]) and got["tasks"][n].dtype == stats[n].dtype, (note, n)
    assert got["mAP50"] == float(np.mean([stats[n][1] for n in names])) and got["mAP"] == float(np.mean([stats[n][0] for n in names])), note


def test_scored_sweep_equals_per_task_update_captured_and_eager(dev):
    """Two batches of one bucket through CapturedSweepStep, scored inside the loop by evaluate_sweep(evaluator=) -- the second replay overwrites the
    buffers the first batch's rows were read from --, against per-task evaluators fed by update() from cloned results of each batch: records,
    img_ids and every stat are equal.  The same on the eager path with max_pairs cutting a batch into two pair stages."""
    from toist_amd import coco_eval as C, harness, sweep
    from toist_amd.postprocessors import PostProcess
    model = _model(dev)
    names, tasks = ["a", "b", "c"], [("a", "x"), ("b", "y"), ("c", "z")]
    _, tok = _inputs(2, 3, 128, 160, 16, 40)
    tok = tok.to(dev)
    batches = []
    for n, ids in enumerate(([10, 11], [12, 13])):
        samples, _ = _inputs(2, 3, 128, 160, 16, 41 + n)
        batches.append({"samples": samples.to(dev), "image_ids": ids, "orig_sizes": [(131, 170), (131, 170)]})
    image_ids = [10, 11, 12, 13]
    # captured
    step = harness.CapturedSweepStep(model, batch=2, captions=3, pad_hw=64)
    per_batch = []
    for b in batches:
        results, pi, pc, live = step.step(b["samples"], tok, b["orig_sizes"])
        per_batch.append({key: {k_: v.clone() for k_, v in r.items()} for key, r in sweep.keyed_results(results, b["image_ids"], names, pi, pc, live).items()})
    data = _ground_truth_from({**per_batch[0], **per_batch[1]}, names, image_ids)
    evs, stats = _control(per_batch, data, names, dev)
    sw = C.SweepEvaluator(data, dev)
    replays = step.replays
    got = harness.evaluate_sweep(model, PostProcess(), batches, tasks, dev, captured=step, tokenized=tok, evaluator=sw)
    assert step.replays == replays + 2 and step.captures == 1
    _same_as_control(sw, got, evs, stats, names, "captured")
    assert max(stats[n][1] for n in names) > 0.0                          # the ground truth was matched: the comparison is not of empty tables
    # step() is still step_rows() + the per-row views
    out, pi, pc, live = step.step_rows(batches[0]["samples"], tok, batches[0]["orig_sizes"])
    assert set(out) == {"scores", "boxes"} and tuple(out["scores"].shape) == (6, 10) and live == 6
    assert torch.equal(out["scores"][4], per_batch[0][(10 + int(pi[4]), names[int(pc[4])])]["scores"])
    # eager, two pair stages per batch
    eager = [harness.evaluate_sweep(model, PostProcess(), [b], tasks, dev, max_pairs=4, tokenized=tok) for b in batches]
    eager = [{key: {k_: v.clone() for k_, v in r.items()} for key, r in keyed.items()} for keyed in eager]
    evs, stats = _control(eager, data, names, dev)
    sw = C.SweepEvaluator(data, dev)
    got = harness.evaluate_sweep(model, PostProcess(), batches, tasks, dev, max_pairs=4, tokenized=tok, evaluator=sw)
    _same_as_control(sw, got, evs, stats, names, "eager")
    # without an evaluator nothing changed: the keyed results
    assert sorted(harness.evaluate_sweep(model, PostProcess(), batches[:1], tasks, dev, captured=step, tokenized=tok)) == sorted((i, n) for i in (10, 11) for n in names)
