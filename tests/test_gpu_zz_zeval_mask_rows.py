"""Captured evaluation scored on the device: toist_coco_masks (csrc/evalrows.hip) on synthetic rows of bit planes against dense numpy (bool masks
give the intersections and areas, the double division is written out here) and, as a second check, the per-image kernels.mask_area / mask_iou;
rows the host would have refused, launched unchecked; one launch replayed from a hipGraph after its planes and tables changed;
TDODCocoEvaluator.update_rows(masks=) against update() on the same rows (records equal byte for byte) and against oracle/coco_ref.CocoEvalRef (the 12
"segm" stats, exact); harness.evaluate(score_rows=True) over a captured step of a tiny mask-head model against the score_rows=False loop.
(The file sorts behind every other GPU test file on purpose: DESIGN 8 item 6.  No training step is built here.)"""
import numpy as np
import pytest
import torch

from oracle import coco_ref as R

pytestmark = pytest.mark.gpu

MAX_DET = 100
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = 256


def _words(h):
    return (h + 63) // 64


def _pack_np(dense):
    """bool [n, h, w] -> uint64 [n, w, ceil(h/64)]: bit b of word yw of column x is pixel (64 * yw + b, x) -- written out here, not kernels.mask_pack."""
    n, h, w = dense.shape
    pad = np.zeros((n, _words(h) * 64, w), dtype=np.uint8)
    pad[:, :h] = dense
    cols = np.ascontiguousarray(pad.transpose(0, 2, 1)).reshape(n, w, _words(h), 64)
    return np.packbits(cols, axis=-1, bitorder="little").view("<u8").reshape(n, w, _words(h))


def _dense_iou(dt, gt, crowd):
    """(areas f64 [D], iou f64 [D, G]) of bool [D, h, w] against bool [G, h, w]: the counts from dense sums (0/1 products summed in fp32 are exact below
    2^24 pixels), i / (crowd ? a_d : a_d + a_g - i) in double, 0.0 where i == 0."""
    D, G = dt.shape[0], gt.shape[0]
    assert dt[0].size < 1 << 24
    a = dt.reshape(D, -1).sum(axis=1).astype(np.float64)
    if G == 0:
        return a, np.zeros((D, 0))
    ag = gt.reshape(G, -1).sum(axis=1).astype(np.float64)
    inter = (dt.reshape(D, -1).astype(np.float32) @ gt.reshape(G, -1).astype(np.float32).T).astype(np.float64)
    union = np.where(np.asarray(crowd, dtype=bool)[None], a[:, None] + 0.0 * ag[None], a[:, None] + ag[None] - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        return a, np.where(inter > 0, inter / union, 0.0)


def _poisoned(n, dtype, dev, guard=GUARD):
    """n elements + a guard region, every byte 0xFF (a NaN for doubles) -> (the whole buffer, its first n elements)."""
    buf = torch.full(((n + guard) * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev).view(dtype)
    return buf, buf[:n]


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _written(t):
    """no element is still the poison pattern"""
    width = t.element_size()
    return bool((~(t.contiguous().view(torch.uint8).view(-1, width) == 0xFF).all(dim=1)).all()) if t.numel() else True


class _Batch:
    """R rows of Q random planes each and a hand-staged ground truth (slot 0 empty and shared, then one slot per row with ground truth, in REVERSED row
    order), everything the launch takes as host arrays; the words behind each row's planes and the guard regions around `bits` and `gt_bits` are
    all-ones, so a read beyond a plane changes a count."""

    def __init__(self, rng, shapes, Gs, Q, capacity_words=None):
        self.shapes, self.Gs, self.Q, self.D, self.R = list(shapes), list(Gs), Q, min(Q, MAX_DET), len(shapes)
        need = max(Q * w * _words(h) for h, w in shapes)
        self.cap = need if capacity_words is None else capacity_words
        self.bits = np.full(2 * GUARD + self.R * self.cap, ONES, dtype=np.uint64)
        self.dense, self.gt, self.crowd = [], [], []
        for r, ((h, w), G) in enumerate(zip(shapes, Gs)):
            dense = rng.random((Q, h, w)) < rng.choice([0.05, 0.3, 0.5, 0.9], size=(Q, 1, 1))
            gt = rng.random((G, h, w)) < rng.choice([0.1, 0.5, 0.8], size=(G, 1, 1))
            dense[0] = False                                                # an all-zero plane
            dense[Q - 1] = Q > 1                                            # an all-ones plane
            if G and Q > 2:
                dense[1] = gt[0]                                            # a detection that IS a ground truth: IoU exactly 1.0
            if G > 1 and Q > 3 and w > 1:
                gt[1][:, w // 2:] = False                                   # a disjoint pair
                dense[2][:, :w // 2] = False
            self.dense.append(dense)
            self.gt.append(gt)
            self.crowd.append(np.array([g % 3 == 2 for g in range(G)], dtype=np.uint8))
            planes = _pack_np(dense).reshape(-1)
            self.bits[GUARD + r * self.cap:GUARD + r * self.cap + planes.size] = planes
        self.order = np.stack([rng.permutation(Q)[:self.D] for _ in range(self.R)]).astype(np.int32)
        self.row_hw = np.array(shapes, dtype=np.int64).reshape(self.R, 2)
        with_gt = [r for r in reversed(range(self.R)) if Gs[r]]
        self.row_slot = np.zeros(self.R, dtype=np.int32)
        for s, r in enumerate(with_gt):
            self.row_slot[r] = s + 1
        self.slot_sizes = np.array([0] + [Gs[r] for r in with_gt], dtype=np.int64)
        self.slot_off = np.concatenate([[0], np.cumsum(self.slot_sizes)]).astype(np.int64)
        self.slot_hw = np.array([(0, 0)] + [shapes[r] for r in with_gt], dtype=np.int32)
        n_gt = int(self.slot_off[-1])
        self.gt_crowd = np.concatenate([self.crowd[r] for r in with_gt] + [np.zeros(0, dtype=np.uint8)])
        self.gt_parea = np.concatenate([self.gt[r].reshape(Gs[r], -1).sum(axis=1) for r in with_gt] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
        sizes = np.concatenate([np.full(Gs[r], shapes[r][1] * _words(shapes[r][0]), dtype=np.int64) for r in with_gt] + [np.zeros(0, dtype=np.int64)])
        self.gt_plane_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.gt_bits = np.full(2 * GUARD + int(self.gt_plane_off[-1]), ONES, dtype=np.uint64)
        if n_gt:
            self.gt_bits[GUARD:-GUARD] = np.concatenate([_pack_np(self.gt[r]).reshape(-1) for r in with_gt])
        self.iou_off = np.concatenate([[0], np.cumsum([self.D * G for G in Gs])]).astype(np.int64)

    def upload(self, dev):
        up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
        self.dev = {name: up(getattr(self, name)) for name in ("bits", "order", "row_hw", "row_slot", "slot_off", "slot_hw", "gt_crowd", "gt_parea",
                                                                "gt_plane_off", "gt_bits", "iou_off")}
        return self

    def launch(self, out=None):
        from toist_amd import kernels as k
        d = self.dev
        bits, gt_bits = d["bits"][GUARD:d["bits"].numel() - GUARD], d["gt_bits"][GUARD:d["gt_bits"].numel() - GUARD]
        return k.coco_masks(bits, self.cap, d["row_hw"], self.Q, d["order"], d["row_slot"], d["slot_off"], gt_bits, d["gt_plane_off"], d["slot_hw"],
                            d["gt_parea"], d["gt_crowd"], d["iou_off"], int(self.iou_off[-1]), out=out)

    def outputs(self, dev, n_iou=None):
        n_iou = int(self.iou_off[-1]) if n_iou is None else n_iou
        self.bufs = {"dt_area": _poisoned(self.R * self.D, torch.float64, dev), "iou": _poisoned(n_iou, torch.float64, dev)}
        return {name: view for name, (_, view) in self.bufs.items()}

    def guards_untouched(self):
        return all(_untouched(whole[view.numel():]) for whole, view in self.bufs.values())

    def expected(self, r):
        return _dense_iou(self.dense[r][self.order[r]], self.gt[r], self.crowd[r])

    def check_row(self, got, r, note):
        D, G = self.D, self.Gs[r]
        area, iou = self.expected(r)
        assert np.array_equal(got["dt_area"][r * D:(r + 1) * D], area), (note, r, "dt_area")
        mine = got["iou"][self.iou_off[r]:self.iou_off[r + 1]]
        assert mine.shape == (D * G,) and np.array_equal(mine.reshape(D, G), iou), (note, r, "iou")
        return iou


SHAPES = lambda chunk: [(1, 1), (63, 5), (64, 64), (65, 3), (130, 67), (200, 129), (65, chunk // 2 + 3)]
ROW_G = (1, 5, 33, 0, 33, 5, 5)


@pytest.mark.parametrize("Q", [1, 3, 7, 100, 130])
def test_mixed_rows_in_one_launch_against_dense_numpy(dev, Q):
    """Seven rows from one pixel to a plane that exceeds one LDS chunk by six words, 0 / 1 / 5 / 33 ground truths, D = min(Q, 100) kept detections in
    a random order: every element of every row's extent is written, equals the dense reference exactly, and nothing else is written."""
    from toist_amd import kernels as k
    chunk = k.COCO_MASKS_CHUNK_WORDS
    shapes = SHAPES(chunk)
    assert shapes[-1][1] * _words(shapes[-1][0]) == chunk + 6
    b = _Batch(np.random.default_rng(100 + Q), shapes, ROW_G, Q).upload(dev)
    assert b.cap == Q * max(w * _words(h) for h, w in shapes)
    out = b.outputs(dev)
    b.launch(out)
    torch.cuda.synchronize()
    assert _written(out["dt_area"]) and _written(out["iou"]) and b.guards_untouched()
    got = {name: t.cpu().numpy() for name, t in out.items()}
    seen = []
    for r in range(b.R):
        seen.append(b.check_row(got, r, Q).reshape(-1))
    seen = np.concatenate(seen)
    if Q >= 7:
        assert (seen == 1.0).any() and (seen == 0.0).any() and ((seen > 0) & (seen < 1)).any()
        assert (got["dt_area"] == 0).any() and any((got["dt_area"][r * b.D:(r + 1) * b.D] == h * w).any() for r, (h, w) in enumerate(shapes))
    # the second check: the per-image kernels the batch launch replaces (areas of the kept planes, then mask_iou against the row's ground truth)
    for r, (h, w) in enumerate(shapes):
        planes = torch.from_numpy(_pack_np(b.dense[r][b.order[r]]).view(np.int64)).to(dev)
        area = k.mask_area(planes, h, w)
        assert np.array_equal(area.cpu().numpy().astype(np.float64), got["dt_area"][r * b.D:(r + 1) * b.D]), (Q, r)
        if ROW_G[r]:
            gp = torch.from_numpy(_pack_np(b.gt[r]).view(np.int64)).to(dev)
            want = k.mask_iou(planes, gp, torch.from_numpy(b.crowd[r]).to(dev), area, k.mask_area(gp, h, w), h, w)
            assert np.array_equal(want.cpu().numpy().reshape(-1), got["iou"][b.iou_off[r]:b.iou_off[r + 1]]), (Q, r)


def test_rows_the_host_would_refuse_are_never_an_index(dev):
    """Unchecked tables straight to the launcher: slots outside the staged ground truth, planes of another size than the ground truth's, planes
    beyond the capacity, sizes that are not positive, order entries of -1 and Q, a plane offset outside the arena.  The good rows of the same launch
    stay exact, the bad rows write their areas (0 where a plane could not be read) and no IoU, and the guards stay untouched."""
    Q = 7
    shapes = [(65, 3), (63, 5), (64, 9), (130, 7), (65, 3), (10, 10), (70, 4), (63, 5), (64, 9), (66, 6)]
    Gs = (5, 1, 5, 1, 5, 5, 1, 5, 1, 5)
    b = _Batch(np.random.default_rng(9), shapes, Gs, Q, capacity_words=Q * 8 * _words(130))
    D = b.D
    good = {0, 9}
    b.row_slot[1], b.row_slot[2] = len(b.slot_sizes), -1                     # slots out of range, above and below
    b.row_hw[3] = (130, 8)                                                  # planes of another size than the slot's (G > 0); they fit the capacity
    b.row_hw[4] = (64 * 4096, 4096)                                         # planes far beyond the capacity
    b.row_hw[5] = (0, 10)                                                   # a size that is not positive
    b.order[6, 2], b.order[7, D - 1] = -1, Q                                # order entries outside [0, Q)
    slot8 = int(b.row_slot[8])
    b.gt_plane_off[int(b.slot_off[slot8])] = int(b.gt_plane_off[-1]) - 1    # row 8's plane would end beyond the arena
    assert Q * 8 * _words(130) <= b.cap
    b.upload(dev)
    out = b.outputs(dev)
    b.launch(out)
    torch.cuda.synchronize()
    assert b.guards_untouched()
    got = {name: t.cpu().numpy() for name, t in out.items()}
    for r in sorted(good):
        b.check_row(got, r, "good")
    for r in range(b.R):
        if r not in good:
            assert _untouched(out["iou"][b.iou_off[r]:b.iou_off[r + 1]]), r
    assert _written(out["dt_area"])
    area = lambda r: got["dt_area"][r * D:(r + 1) * D]
    for r in (1, 2, 8):                                                     # the planes themselves were readable
        assert np.array_equal(area(r), b.expected(r)[0]), r
    h, w = 130, 8                                                           # row 3 read its planes with the stride of the size it was given
    flat = b.bits[GUARD + 3 * b.cap:GUARD + 4 * b.cap]
    want = [int(sum(bin(int(v)).count("1") for v in flat[q * w * _words(h):(q + 1) * w * _words(h)])) for q in b.order[3]]
    assert area(3).tolist() == want
    assert (area(4) == 0).all() and (area(5) == 0).all()
    for r, d in ((6, 2), (7, D - 1)):
        dense = b.dense[r][np.clip(b.order[r], 0, Q - 1)]
        want = dense.reshape(D, -1).sum(axis=1).astype(np.float64)
        want[d] = 0.0
        assert np.array_equal(area(r), want), r


def test_one_captured_launch_serves_changed_planes_and_tables(dev):
    """toist_coco_masks reads nothing from the host: one launch captured in a hipGraph, replayed after the planes, order, row_hw and the row tables
    changed in place, gives the new batch's values -- inside fixed-capacity outputs whose tails stay untouched."""
    Q, cap_iou = 7, 7 * 3 * 33
    shape_sets = ([(63, 5), (65, 3), (130, 67)], [(130, 67), (64, 64), (1, 1)], [(65, 3), (63, 5), (64, 64)])
    g_sets = ((5, 0, 33), (1, 33, 5), (0, 0, 1))
    cap = Q * 67 * _words(130)
    batches = [_Batch(np.random.default_rng(20 + n), s, g, Q, capacity_words=cap) for n, (s, g) in enumerate(zip(shape_sets, g_sets))]
    # fixed addresses: the first batch's device tensors, sized for the largest of the three (the staged ground truth changes too: a harder case than
    # an evaluation, whose ground truth stays)
    first = batches[0].upload(dev)
    fixed = {}
    for name in first.dev:
        n = max(getattr(b, name).size for b in batches)
        src = first.dev[name]
        fixed[name] = torch.full((n,), 255 if src.dtype == torch.uint8 else -1, dtype=src.dtype, device=dev)
    out = first.outputs(dev, n_iou=cap_iou)

    def load(b):
        b.upload(dev)
        for name, t in b.dev.items():
            if name in ("gt_bits", "gt_plane_off", "gt_parea", "gt_crowd", "slot_off", "slot_hw"):
                assert t.numel() <= fixed[name].numel()
            fixed[name].fill_(255 if t.dtype == torch.uint8 else -1)
            fixed[name][:t.numel()] = t.reshape(-1)

    from toist_amd import kernels as k

    def launch(b):
        # every table at its fixed address; slot tables are cut to the largest batch's extent (unused slots are never named)
        n_slots = max(x.slot_sizes.size for x in batches)
        n_gt = max(int(x.slot_off[-1]) for x in batches)
        g_words = max(int(x.gt_plane_off[-1]) for x in batches)
        return k.coco_masks(fixed["bits"][GUARD:GUARD + 3 * cap], cap, fixed["row_hw"].view(3, 2), Q, fixed["order"].view(3, Q), fixed["row_slot"],
                            fixed["slot_off"][:n_slots + 1], fixed["gt_bits"][GUARD:GUARD + g_words], fixed["gt_plane_off"][:n_gt + 1],
                            fixed["slot_hw"][:2 * n_slots].view(n_slots, 2), fixed["gt_parea"][:n_gt], fixed["gt_crowd"][:n_gt], fixed["iou_off"], cap_iou,
                            out=out)

    def pad_tables(b):
        """Slot tables of a batch padded to the common extents: unused slots are empty and sit at the end of the staged entries."""
        n_slots = max(x.slot_sizes.size for x in batches)
        n_gt = max(int(x.slot_off[-1]) for x in batches)
        b.slot_off = np.concatenate([b.slot_off, np.full(n_slots + 1 - b.slot_off.size, b.slot_off[-1])]).astype(np.int64)
        b.slot_hw = np.concatenate([b.slot_hw, np.zeros((n_slots - b.slot_hw.shape[0], 2), dtype=np.int32)])
        b.gt_plane_off = np.concatenate([b.gt_plane_off, np.full(n_gt + 1 - b.gt_plane_off.size, b.gt_plane_off[-1])]).astype(np.int64)
        b.gt_parea = np.concatenate([b.gt_parea, np.zeros(n_gt - b.gt_parea.size, dtype=np.int32)])
        b.gt_crowd = np.concatenate([b.gt_crowd, np.zeros(n_gt - b.gt_crowd.size, dtype=np.uint8)])

    for b in batches:
        pad_tables(b)
    load(batches[0])
    launch(batches[0])                                                       # the module is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(batches[0])
    for n in (1, 2, 0):
        b = batches[n]
        load(b)
        for whole, _ in first.bufs.values():
            whole.view(torch.uint8).fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        n_iou = int(b.iou_off[-1])
        assert first.guards_untouched() and _untouched(out["iou"][n_iou:]) and _written(out["iou"][:n_iou]) and _written(out["dt_area"]), n
        got = {name: t.cpu().numpy() for name, t in out.items()}
        for r in range(3):
            b.check_row(got, r, ("replay", n))


# ---- update_rows(masks=) against update() and the oracle ---------------------------------------------------------------------------------
def _mask_dataset(rng, sizes, n_gts, first_id=100):
    """A COCO-format ground truth with dense segmentations: one image per entry of n_gts (None: an image id the ground truth does not know)."""
    images, anns, ids = [], [], []
    for n, (G, (h, w)) in enumerate(zip(n_gts, sizes)):
        img = first_id + n
        ids.append(img)
        if G is None:
            continue
        images.append({"id": img, "height": h, "width": w})
        for g in range(G):
            bw, bh = int(rng.integers(3, max(4, w // 2))), int(rng.integers(3, max(4, h // 2)))
            x, y = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            m = np.zeros((h, w), dtype=bool)
            m[y:y + bh, x:x + bw] = rng.random((bh, bw)) < 0.9
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1 if g != 3 else 2, "iscrowd": int(g == 2),
                         "bbox": [float(x), float(y), float(bw), float(bh)], "area": float(m.sum()) if g % 2 else float(rng.integers(100, 20000)),
                         "segmentation": m})
    return {"images": images, "annotations": anns}, ids


def _mask_rows(rng, dataset, row_images, hw_of, Q):
    """Per row: coarse scores (ties), boxes, and Q dense masks -- jittered copies of the image's objects, an exact copy, false positives, an empty mask."""
    by_img = {}
    for a in dataset["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a)
    scores = np.round(rng.random((len(row_images), Q)), 1).astype(np.float32)
    boxes = np.zeros((len(row_images), Q, 4), dtype=np.float32)
    dense = []
    for r, img in enumerate(row_images):
        h, w = hw_of[img]
        objs = by_img.get(img, [])
        m = np.zeros((Q, h, w), dtype=bool)
        for q in range(Q):
            x, y = rng.integers(0, w - 3), rng.integers(0, h - 3)
            bw, bh = rng.integers(2, w - x), rng.integers(2, h - y)
            if objs and q % 4 != 3:
                a = objs[q % len(objs)]
                dx, dy = (0, 0) if q % 4 == 0 and q < 8 else rng.integers(-4, 5, 2)
                m[q] = np.roll(np.roll(a["segmentation"], dy, 0), dx, 1)
                x, y, bw, bh = a["bbox"][0] + dx, a["bbox"][1] + dy, a["bbox"][2], a["bbox"][3]
            elif q % 8 != 7:
                m[q, y:y + bh, x:x + bw] = True
            boxes[r, q] = (x, y, x + bw + 0.25, y + bh)
        dense.append(m)
    return scores, boxes, dense


def _same_records(got, want, note):
    assert sorted(got, key=str) == sorted(want, key=str), note
    for img in want:
        g, w = got[img], want[img]
        assert list(g) == list(w) and g["image_id"] == w["image_id"], (note, img)
        for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"):
            assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape and np.array_equal(g[key], w[key], equal_nan=True) and \
                g[key].tobytes() == w[key].tobytes(), (note, img, key)


def _row_inputs(scores, boxes, dense, row_images, hw_of, dev):
    """-> (update_rows' out and masks, update()'s predictions: the FIRST row of every image id)."""
    from toist_amd import coco_eval as C, kernels as k
    planes = [k.mask_pack(torch.from_numpy(m).to(dev)) for m in dense]
    out = {"scores": torch.from_numpy(scores).to(dev), "boxes": torch.from_numpy(boxes).to(dev)}
    masks = C.RowMasks.pack(planes, [hw_of[i] for i in row_images])
    pred = {}
    for r, img in enumerate(row_images):
        pred.setdefault(img, {"scores": out["scores"][r], "labels": torch.ones(scores.shape[1], dtype=torch.int64, device=dev), "boxes": out["boxes"][r],
                              "mask_bits": planes[r], "mask_size": hw_of[img]})
    return out, masks, pred


SIZES = [(65, 70), (130, 67), (64, 64), (40, 129), (63, 50), (90, 33)]
N_GTS = (5, 1, 0, None, 12, 3)


@pytest.mark.parametrize("R_", [1, 8])
@pytest.mark.parametrize("types", [["segm"], ["bbox", "segm"], ["bbox"]])
def test_update_rows_with_masks_files_the_records_of_update(dev, types, R_):
    """update_rows(masks=) on a batch (an image id twice in it, an image the ground truth does not know, an image without annotations, a padding
    row behind `live`) and a second batch that names an image of the first again, against update() on the same rows as dicts: the records of every
    iou type, img_ids and the summaries are equal."""
    from toist_amd import coco_eval as C
    rng = np.random.default_rng(31 * R_ + len(types))
    dataset, ids = _mask_dataset(rng, SIZES, N_GTS)
    hw_of = dict(zip(ids, SIZES))
    Q = 12
    if R_ == 1:
        plans = [([ids[0]], 1), ([ids[3]], 1), ([ids[0]], 1), ([ids[2]], 1)]
    else:
        plans = [([ids[0], ids[1], ids[2], ids[3], ids[4], ids[0], ids[1], ids[5]], 7), ([ids[5], ids[1], ids[4], ids[3], ids[2], ids[0], ids[5], ids[5]], 8)]
    ev, ctl = C.TDODCocoEvaluator(dataset, types, device=dev), C.TDODCocoEvaluator(dataset, types, device=dev)
    for row_images, live in plans:
        scores, boxes, dense = _mask_rows(rng, dataset, row_images, hw_of, Q)
        out, masks, _ = _row_inputs(scores, boxes, dense, row_images, hw_of, dev)
        _, _, pred = _row_inputs(scores[:live], boxes[:live], dense[:live], row_images[:live], hw_of, dev)
        ev.update_rows(out, row_images, live=live, masks=masks)
        ctl.update(pred)
    assert ev.img_ids == ctl.img_ids
    for t in types:
        _same_records(ev.coco_eval[t].records, ctl.coco_eval[t].records, (types, R_, t))
    assert len(ev._scorer.mail) == 0 and ev._scorer.staged.has_planes == ("segm" in types)
    for e in (ev, ctl):
        e.accumulate()
        e.summarize(verbose=False)
    for t in types:
        assert np.array_equal(ev.coco_eval[t].stats, ctl.coco_eval[t].stats), (t, ev.coco_eval[t].stats, ctl.coco_eval[t].stats)
    if "segm" in types and R_ == 8:
        assert ev.coco_eval["segm"].stats[1] > 0.0
        # a row whose planes are of another size than its ground truth's is refused before anything is launched, in update()'s words
        scores, boxes, dense = _mask_rows(rng, {"annotations": []}, [ids[0]], {ids[0]: (64, 64)}, Q)
        out, masks, _ = _row_inputs(scores, boxes, dense, [ids[0]], {ids[0]: (64, 64)}, dev)
        with pytest.raises(ValueError, match="predicted masks are 64x64, the ground truth is 65x70"):
            ev.update_rows(out, [ids[0]], masks=masks)


def test_segm_stats_of_update_rows_match_the_oracle_exactly(dev):
    """Eight images in two batches of four rows through update_rows(masks=): the precision table and the 12 "segm" stats equal
    oracle/coco_ref.CocoEvalRef(iou_type="segm"), exact (as tests/test_gpu_coco.py holds update())."""
    from toist_amd import coco_eval as C
    rng = np.random.default_rng(17)
    sizes = [(90, 120), (65, 70), (130, 67), (64, 64), (100, 129), (63, 50), (90, 33), (77, 77)]
    dataset, ids = _mask_dataset(rng, sizes, (5, 1, 0, 7, 12, 3, 2, 4))
    hw_of = dict(zip(ids, sizes))
    Q = 16
    ev = C.TDODCocoEvaluator(dataset, ["segm"], device=dev)
    res = {}
    for lo in (0, 4):
        row_images = ids[lo:lo + 4]
        scores, boxes, dense = _mask_rows(rng, dataset, row_images, hw_of, Q)
        out, masks, _ = _row_inputs(scores, boxes, dense, row_images, hw_of, dev)
        ev.update_rows(out, row_images, masks=masks)
        for r, img in enumerate(row_images):
            res[img] = {"scores": scores[r], "labels": np.ones(Q, dtype=np.int64), "boxes": boxes[r], "masks": dense[r][:, None]}
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize(verbose=False)
    gts = [dict(a, counts=R.rle_encode(a["segmentation"])) for a in dataset["annotations"]]
    ref = R.CocoEvalRef(gts, R.detections_from_results(res, "segm"), ids, "segm")
    ref.evaluate()
    ref.accumulate()
    want = ref.summarize()
    got = ev.coco_eval["segm"]
    assert sorted(got.records) == ids
    assert np.array_equal(got.eval["precision"][:, :, 0], ref.precision[:, :, 0])
    assert np.array_equal(got.stats, want), (got.stats, want)
    assert 0.0 < want[0] < 1.0


# ---- end to end: a tiny mask-head model through the captured step ----------------------------------------------------------------------------
def test_evaluation_loop_scores_the_captured_rows_on_the_device(dev):
    """harness.evaluate(captured=, criterion=None, score_rows=True) on three batches of two 128 x 192 images of a tiny mask-head model returns the box
    and mask summaries of the score_rows=False loop on the same batches, the evaluators' records are equal, and a second, different batch replayed
    right behind update_rows does not change what the first batch filed."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess, PostProcessSegm
    torch.manual_seed(0)
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", enc_layers=1, dec_layers=1, num_queries=20)
    model, _, _, weight_dict = toist_amd.build_model(args)
    model.to(dev)
    batches = []
    for b in range(3):
        samples, tok, targets, pmap = harness.synthetic_batch(2, 128, 192, tokens=12, seed=20 + b, device=dev, max_targets=4, with_masks=True)
        for i, t in enumerate(targets):
            t["image_id"] = torch.tensor([100 + 2 * b + i], device=dev)
            t["orig_size"], t["size"] = torch.tensor([128, 192], device=dev), torch.tensor([128, 192], device=dev)
        batches.append({"samples": samples, "tokenized": tok, "targets": targets, "positive_map": pmap})
    gt = harness.synthetic_ground_truth([b["targets"] for b in batches])
    post = {"bbox": PostProcess(), "segm": PostProcessSegm(packed=True)}
    step = harness.CapturedEvalStep(model, batch=2, max_orig_hw=(128, 192), pad_hw=64)
    ev = toist_amd.TDODCocoEvaluator(gt, ["bbox", "segm"], device=dev)
    keyed = harness.evaluate(model, None, None, post, weight_dict, batches, [ev], dev, args, captured=step)
    ev2 = toist_amd.TDODCocoEvaluator(gt, ["bbox", "segm"], device=dev)
    rows = harness.evaluate(model, None, None, post, weight_dict, batches, [ev2], dev, args, captured=step, score_rows=True)
    assert step.captures == 1 and step.replays == 5
    assert sorted(ev2.img_ids) == [100, 101, 102, 103, 104, 105] == sorted(ev.img_ids)
    for name in ("coco_eval_bbox", "coco_eval_masks"):
        assert len(rows[name]) == 12 and rows[name] == keyed[name], (name, rows[name], keyed[name])
    assert set(rows) == set(keyed)
    for t in ("bbox", "segm"):
        _same_records(ev2.coco_eval[t].records, ev.coco_eval[t].records, t)
    # the views of a bucket live until its next step: what update_rows launched has read them before the next replay overwrites them
    sizes = [(128, 192)] * 2
    ev3 = toist_amd.TDODCocoEvaluator(gt, ["bbox", "segm"], device=dev)
    out, masks = step.step_rows(batches[0]["samples"], batches[0]["tokenized"], sizes, sizes)
    assert masks.capacity_words == step.capacity_words and masks.hw_host == sizes and tuple(masks.hw_dev.shape) == (2, 2)
    ev3.update_rows(out, [100, 101], masks=masks)
    step.step_rows(batches[2]["samples"], batches[2]["tokenized"], sizes, sizes)
    for t in ("bbox", "segm"):
        _same_records(ev3.coco_eval[t].records, {i: ev.coco_eval[t].records[i] for i in (100, 101)}, ("overwritten", t))
    with pytest.raises(ValueError, match="dense_masks=False"):
        harness.CapturedEvalStep(model, batch=2, max_orig_hw=(128, 192), pad_hw=64, dense_masks=True).step_rows(
            batches[0]["samples"], batches[0]["tokenized"], sizes, sizes)
