"""COCO evaluation of the detection / segmentation outputs (reference: /root/reference/datasets/coco_eval.py:167-404,
TDODCocoEvaluator, driven by engine.py:307-342).

The reference hands every batch to pycocotools on the host: Q dense masks per image are copied off the GPU, run-length
encoded, intersected run by run, then matched in pure-Python loops.  Here the per-batch work stays on the MI355X
(csrc/evalmask.hip): masks are column-major bit planes (from PostProcessSegm(packed=True), or packed from dense masks),
areas and intersections are popcounts, IoUs are formed in double exactly as maskApi's rleIou / bbIou do, and
COCOeval.evaluateImg's greedy matching runs as one thread per (image, area range, IoU threshold).  Only the per-image match
tables travel to the host; accumulate() / summarize() (once per evaluation, a few thousand numbers) are numpy.

pycocotools is a third-party package that is absent from /root/reference and from this image (requirements.txt:56 pins
cocoapi @ 8c9bcc3); its published algorithm is restated in oracle/coco_ref.py, which tests/ hold this module against.
There is no CPU path: without the HIP library, or with host tensors, the kernels raise."""
import numpy as np
import torch

from . import dist as tdist
from . import kernels as k

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LBL = ("all", "small", "medium", "large")


# ---- RLE text form (maskApi.c rleToString / rleFrString) -------------------------------------------------------
def counts_to_string(counts):
    c = np.asarray(counts, dtype=np.int64)
    x = c.copy()
    x[3:] -= c[1:-2]                                        # from the 4th count on: difference to the count two back
    out = bytearray()
    for v in x.tolist():
        while True:
            ch = v & 0x1F
            v >>= 5
            more = (v != -1) if (ch & 0x10) else (v != 0)
            out.append((ch | 0x20 if more else ch) + 48)
            if not more:
                break
    return out.decode("ascii")


def string_to_counts(s):
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, shift = 0, 0
        while True:
            ch = ord(s[p]) - 48
            p += 1
            x |= (ch & 0x1F) << shift
            shift += 5
            if not ch & 0x20:
                if ch & 0x10:
                    x |= -1 << shift
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def counts_to_mask(counts, h, w):
    """dense bool [h, w] of a column-major run-length list (zeros first)."""
    c = np.asarray(counts, dtype=np.int64)
    if int(c.sum()) != h * w:
        raise ValueError(f"run lengths sum to {int(c.sum())}, the mask has {h * w} pixels")
    vals = np.zeros(len(c), dtype=bool)
    vals[1::2] = True
    return np.repeat(vals, c).reshape(w, h).T


def polygon_to_mask(xy, h, w):
    """maskApi.c rleFrPoly restated: polygon edges are traced on a 5x finer integer grid, the crossings of pixel-column
    boundaries become run boundaries of the column-major mask.  (Host-side ground-truth preparation, once per annotation.)"""
    scale = 5.0
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    x = [int(scale * px + .5) for px in pts[:, 0]]
    y = [int(scale * py + .5) for py in pts[:, 1]]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(len(pts)):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    bx, by = [], []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / scale - .5
        if np.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / scale - .5
        yd = min(max(yd, 0.0), float(h))
        bx.append(int(xd))
        by.append(int(np.ceil(yd)))
    a = np.sort(np.array([px * h + py for px, py in zip(bx, by)] + [h * w], dtype=np.int64))
    runs = np.diff(np.concatenate([[0], a]))
    counts, j = [int(runs[0])], 1
    while j < len(runs):                                      # zero-length runs glue their neighbours together
        if runs[j] > 0:
            counts.append(int(runs[j]))
            j += 1
        else:
            j += 1
            if j < len(runs):
                counts[-1] += int(runs[j])
                j += 1
    return counts_to_mask(counts, h, w)


DEVICE_TRACE_STEPS = 1 << 22       # trace steps one device call of convert_coco_poly_to_mask accepts: 5 per pixel of perimeter, i.e. 840 k pixels
_RASTERISERS = {}                  # device -> DevicePolygonMasks, regrown when a call needs more


def _device_poly_masks(segmentations, height, width, device):
    """bool [n, height, width] on `device` from csrc/poly.hip: one launch for all objects."""
    from .preprocess import DevicePolygonMasks, polygon_tables
    device = torch.device(device)
    segmentations = [list(polygons) for polygons in segmentations]
    sizes = [(height, width)] * len(segmentations)
    verts, polys, desc, steps = polygon_tables(segmentations, sizes)              # every check before a buffer is made
    if steps > DEVICE_TRACE_STEPS:
        raise ValueError(f"convert_coco_poly_to_mask: {steps} trace steps exceed coco_eval.DEVICE_TRACE_STEPS = {DEVICE_TRACE_STEPS}: rasterise these on the host")
    need = (desc.shape[0], max(polys.shape[0], 1), max(verts.shape[0], 1), height, width)
    r = _RASTERISERS.get(device)
    have = (0,) * 5 if r is None else (r.max_objects, r.max_polygons, r.max_vertices, *r.max_hw)
    if any(n > c for n, c in zip(need, have)):
        cap = [max(n, c) for n, c in zip(need, have)]
        r = _RASTERISERS[device] = DevicePolygonMasks(device, cap[0], cap[1], cap[2], (cap[3], cap[4]), DEVICE_TRACE_STEPS)
    with torch.cuda.device(device):
        return torch.stack(r.dense(r.pack(segmentations, sizes)), dim=0)


def convert_coco_poly_to_mask(segmentations, height, width, device=None):
    """datasets/tdod.py:133-147 (and datasets/coco.py:66-80): one bool mask per object, the union of its polygons
    (coco_mask.frPyObjects + decode + any(dim=2) in the reference).  device = a GPU: the same masks as a bool device tensor, rasterised there
    (csrc/poly.hip through preprocess.DevicePolygonMasks; at most kernels.POLYGON_MAX_ROWS rows and DEVICE_TRACE_STEPS trace steps per call)."""
    if device is not None:
        if not segmentations:
            return torch.zeros((0, height, width), dtype=torch.uint8, device=device)
        return _device_poly_masks(segmentations, height, width, device)
    masks = []
    for polygons in segmentations:
        m = np.zeros((height, width), dtype=bool)
        for poly in polygons:
            m |= polygon_to_mask(poly, height, width)
        masks.append(torch.from_numpy(m))
    return torch.stack(masks, dim=0) if masks else torch.zeros((0, height, width), dtype=torch.uint8)


def polygon_vertices(poly):
    """One polygon of a "segmentation" (a flat x0, y0, x1, y1, ...) checked before it is rasterised: -> (float64 [n, 2] vertices, trace steps).  The
    trace steps are the sum over the closed path's edges of max(|dx|, |dy|) on rleFrPoly's 5x grid, int(5 * c + .5): the iterations polygon_to_mask
    spends on the polygon (its cost, about 5x the perimeter in pixels).  Raises ValueError for an empty or odd-length list, a non-finite coordinate
    and a coordinate whose grid value leaves int32 (maskApi.c holds the grid in int)."""
    try:
        xy = np.asarray(poly, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError(f"a polygon is a flat list of numbers x0, y0, x1, y1, ... ({e})") from None
    if xy.size == 0 or xy.size % 2:
        raise ValueError(f"a polygon is a non-empty flat list x0, y0, x1, y1, ... of even length (got {xy.size} numbers)")
    if not np.isfinite(xy).all():
        raise ValueError("a polygon holds a non-finite coordinate")
    grid = 5.0 * xy + .5
    if (np.abs(grid) >= 2.0 ** 31).any():
        raise ValueError("a polygon holds a coordinate whose 5x grid value does not fit int32")
    g = np.trunc(grid).astype(np.int64).reshape(-1, 2)
    d = np.abs(np.roll(g, -1, axis=0) - g)
    return xy.reshape(-1, 2), int(d.max(axis=1).sum())


# ---- ground truth ----------------------------------------------------------------------------------------------
class CocoGroundTruth:
    """The slice of pycocotools.coco.COCO the evaluator reads: a COCO-format dict {"images": [{"id","height","width"}],
    "annotations": [{"id","image_id","category_id","bbox" [x,y,w,h],"area","iscrowd","segmentation"}]}.
    A segmentation is a list of polygons, an RLE dict {"size": [h, w], "counts": list | str} or a dense [h, w] array.
    polygons_on_device: planes() rasterises an image's polygon annotations on the device (convert_coco_poly_to_mask(device=)), the same bits; RLE and
    dense segmentations keep the host path."""

    def __init__(self, dataset, polygons_on_device=False):
        self.dataset = dataset
        self.polygons_on_device = bool(polygons_on_device)
        self.imgs = {im["id"]: im for im in dataset.get("images", [])}
        self.img_anns = {i: [] for i in self.imgs}
        for ann in dataset.get("annotations", []):
            if ann["id"] == 0:
                raise ValueError("annotation ids must be non-zero: COCOeval stores the matched id and reads 0 as 'unmatched'")
            self.img_anns.setdefault(ann["image_id"], []).append(ann)
        self._planes = {}

    def annotations(self, img_id, cat_ids):
        return [a for a in self.img_anns.get(img_id, []) if cat_ids is None or a["category_id"] in cat_ids]

    def dense_mask(self, ann):
        """COCO.annToMask: polygons are merged by union."""
        im = self.imgs[ann["image_id"]]
        h, w = im["height"], im["width"]
        seg = ann["segmentation"]
        if isinstance(seg, dict):
            counts = string_to_counts(seg["counts"]) if isinstance(seg["counts"], (str, bytes)) else seg["counts"]
            return counts_to_mask(counts, seg["size"][0], seg["size"][1])
        if isinstance(seg, (list, tuple)):
            out = np.zeros((h, w), dtype=bool)
            for poly in seg:
                out |= polygon_to_mask(poly, h, w)
            return out
        return np.asarray(seg).astype(bool)

    def _dense_on_device(self, anns, device):
        """bool [n, h, w] on the device: the polygon annotations in one rasterise launch, every other kind through dense_mask."""
        im = self.imgs[anns[0]["image_id"]]
        poly = [i for i, a in enumerate(anns) if isinstance(a["segmentation"], (list, tuple))]
        dense = torch.zeros((len(anns), im["height"], im["width"]), dtype=torch.bool, device=device)
        if poly:
            dense[poly] = convert_coco_poly_to_mask([anns[i]["segmentation"] for i in poly], im["height"], im["width"], device=device)
        for i, a in enumerate(anns):
            if i not in poly:
                dense[i] = torch.from_numpy(np.ascontiguousarray(self.dense_mask(a))).to(device)
        return dense

    def planes(self, img_id, cat_ids, device):
        """Bit planes of an image's ground-truth masks (packed once, kept on the device)."""
        key = (img_id, None if cat_ids is None else tuple(cat_ids))
        if key not in self._planes:
            anns = self.annotations(img_id, cat_ids)
            if anns and self.polygons_on_device:
                self._planes[key] = k.mask_pack(self._dense_on_device(anns, device))
                return self._planes[key]
            dense = np.stack([self.dense_mask(a) for a in anns]) if anns else None
            self._planes[key] = None if dense is None else k.mask_pack(torch.from_numpy(dense).to(device))
        return self._planes[key]


# ---- the evaluator -----------------------------------------------------------------------------------------------
class IouTypeEval:
    """What the reference reads from a pycocotools COCOeval: .eval (precision / recall tables) and .stats."""

    def __init__(self, iou_type):
        self.iouType = iou_type
        self._records = {}                # image id -> per-image match tables
        self.drain = None                 # set by a row scorer (update_rows): files the match tables that are still on their way
        self.eval, self.stats = None, None

    @property
    def records(self):
        """image id -> per-image match tables.  Every read first files what update_rows has in flight, so a reader sees what update() would have left."""
        if self.drain is not None:
            self.drain()
        return self._records

    @records.setter
    def records(self, value):
        self._records = value

    def accumulate(self):
        T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
        precision, recall, scores = -np.ones((T, R, 1, A, M)), -np.ones((T, 1, A, M)), -np.ones((T, R, 1, A, M))
        recs = [self.records[i] for i in sorted(self.records)]
        recs = [r for r in recs if r["scores"].size or r["gt_ignore"].shape[1]]           # images with neither are skipped
        for a in range(A):
            if not recs:
                continue
            npig = int(sum((~r["gt_ignore"][a]).sum() for r in recs))
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sc = np.concatenate([r["scores"][:max_det] for r in recs])
                order = np.argsort(-sc, kind="mergesort")
                sc = sc[order]
                matched = np.concatenate([r["dt_match"][a][:, :max_det] >= 0 for r in recs], axis=1)[:, order]
                ignored = np.concatenate([r["dt_ignore"][a][:, :max_det] for r in recs], axis=1)[:, order]
                tp = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                fp = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                nd = tp.shape[1]
                if nd == 0:
                    recall[:, 0, a, m], precision[:, :, 0, a, m], scores[:, :, 0, a, m] = 0, 0, 0
                    continue
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]                 # monotone precision envelope
                recall[:, 0, a, m] = rc[:, -1]
                for t in range(T):
                    at = np.searchsorted(rc[t], REC_THRS, side="left")
                    ok = at < nd
                    precision[t, :, 0, a, m] = np.where(ok, pr[t][np.minimum(at, nd - 1)], 0.0)
                    scores[t, :, 0, a, m] = np.where(ok, sc[np.minimum(at, nd - 1)], 0.0)
        self.eval = {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, 1, A, M]}

    def summarize(self, verbose=True):
        if self.eval is None:
            raise RuntimeError("Please run accumulate() first")

        def one(ap, iou_thr=None, area="all", max_dets=100):
            a, m = AREA_LBL.index(area), MAX_DETS.index(max_dets)
            s = self.eval["precision"][:, :, :, a, m] if ap else self.eval["recall"][:, :, a, m]
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            val = -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
            if verbose:
                rng = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
                print(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
                    "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", rng, area, max_dets, val))
            return val
        self.stats = np.array([one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"),
                               one(0, max_dets=1), one(0, max_dets=10), one(0), one(0, area="small"), one(0, area="medium"),
                               one(0, area="large")])
        return self.stats


class TDODCocoEvaluator:
    """Same surface as the reference class (coco_eval.py:167-345): update(res), synchronize_between_processes(), accumulate(),
    summarize(), .coco_eval[iou_type].stats.  `coco_gt` is a CocoGroundTruth (or the COCO-format dict itself).  The reference
    evaluates category 1 only (coco_eval.py:203: params.catIds = 1, and PostProcess labels every query 1)."""

    def __init__(self, coco_gt, iou_types, useCats=True, device="cuda"):
        assert isinstance(iou_types, (list, tuple))
        self.coco_gt = coco_gt if isinstance(coco_gt, CocoGroundTruth) else CocoGroundTruth(coco_gt)
        self.iou_types, self.useCats = list(iou_types), useCats
        self.cat_ids = (1,) if useCats else None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TDODCocoEvaluator runs its IoU and matching kernels on the GPU; there is no CPU path")
        self.coco_eval = {t: IouTypeEval(t) for t in iou_types}
        self.img_ids = []
        self._scorer, self._staged_index = None, 0           # update_rows' device state, made at its first call (or attached by a SweepEvaluator)
        self._thr = torch.from_numpy(IOU_THRS).to(self.device)
        self._rng = torch.from_numpy(AREA_RNG).to(self.device)

    # -- per batch ---------------------------------------------------------------------------------------------------
    def _detections(self, pred):
        """score-descending (stable) order of the detections of the evaluated category, cut to maxDets[-1]."""
        scores = pred["scores"].to(self.device)
        keep = torch.arange(scores.numel(), device=self.device)
        if self.cat_ids is not None:
            labels = pred["labels"].to(self.device)
            keep = keep[(labels[:, None] == torch.tensor(self.cat_ids, device=self.device)[None]).any(1)]
        order = torch.sort(scores[keep].double(), descending=True, stable=True).indices[:MAX_DETS[-1]]
        return keep[order]

    def update(self, predictions):
        img_ids = sorted(set(predictions.keys()))
        self.img_ids.extend(img_ids)
        for iou_type in self.iou_types:
            if iou_type not in ("bbox", "segm"):
                raise ValueError("Unknown iou type {}".format(iou_type))
            self._evaluate(iou_type, img_ids, predictions)

    def update_rows(self, out, image_ids, live=None, masks=None):
        """update() for a whole batch of PostProcess rows in two launches (toist_coco_boxes, toist_coco_match) and without a host synchronisation:
        out = kernels.postprocess's dict (scores f32 [rows, Q], boxes f32 [rows, Q, 4], read in place), row i belongs to image_ids[i], the first
        `live` rows are scored (default: one per image id).  The records it files are the ones update() files for the same rows -- same keys,
        dtypes, shapes and bytes; the first evaluation of an image id wins, also inside one batch.  The match tables travel through a
        staging.Mailbox and become records when they have arrived, oldest first; accumulate(), synchronize_between_processes() and any read of
        .records drain everything.  The ground truth is staged on the device at the first call (StagedGroundTruth).
        masks=None: only iou_types == ["bbox"].  masks = a RowMasks over the rows' bit planes (CapturedEvalStep.step_rows hands one out; RowMasks.pack
        builds one): any iou_types within ("bbox", "segm") -- "segm" adds toist_coco_masks (the IoU block and the popcount areas of the whole batch in
        one launch, against ground-truth planes staged once) and a second toist_coco_match.  Everything is launched on the current stream, behind
        whatever wrote `out` and the planes there, so a replay issued afterwards on that stream overwrites them only when they have been read."""
        if masks is None:
            if self.iou_types != ["bbox"]:
                raise ValueError(f"update_rows without masks serves iou_types == ['bbox'] (this evaluator has {self.iou_types}): pass masks=RowMasks, "
                                 "or send masks through update()")
        elif not self.iou_types or any(t not in ("bbox", "segm") for t in self.iou_types):
            raise ValueError(f"update_rows serves iou_types within ('bbox', 'segm') (this evaluator has {self.iou_types})")
        elif not isinstance(masks, RowMasks):
            raise TypeError(f"update_rows: masks is a coco_eval.RowMasks (got {type(masks).__name__})")
        ids = [int(i) if torch.is_tensor(i) else i for i in image_ids]
        live = len(ids) if live is None else int(live)
        if not 0 <= live <= len(ids):
            raise ValueError(f"update_rows: {live} live rows but {len(ids)} image ids")
        ids = ids[:live]
        scorer, t = self._row_scorer()
        if masks is None:
            ev = self.coco_eval["bbox"]
            scorer.score(out, scorer.staged.slots([(t, i) for i in ids]), [(ev, i) for i in ids])
        else:
            scorer.score(out, scorer.staged.slots([(t, i) for i in ids]), [(self.coco_eval, i) for i in ids], masks=masks, types=tuple(self.iou_types))
        self.img_ids.extend(sorted(set(ids)))

    def _row_scorer(self):
        """(the _RowScorer that serves update_rows, this evaluator's index in its staged ground truth): its own, made at the first call, unless a
        SweepEvaluator attached the one its evaluators share."""
        if getattr(self, "_scorer", None) is None:
            staged = StagedGroundTruth([self.coco_gt], self.device, self.cat_ids, planes="segm" in self.iou_types)
            self._attach(_RowScorer(staged, self.device), 0)
        return self._scorer, self._staged_index

    def _attach(self, scorer, index):
        self._scorer, self._staged_index = scorer, index
        for ev in self.coco_eval.values():
            ev.drain = scorer.drain

    def _evaluate(self, iou_type, img_ids, predictions):
        dev = self.device
        ious, dt_area, gt_area, gt_crowd, scores, n_dt, n_gt = [], [], [], [], [], [], []
        for img in img_ids:
            pred = predictions[img]
            anns = self.coco_gt.annotations(img, self.cat_ids)
            crowd = torch.tensor([int(a.get("iscrowd", 0)) for a in anns], dtype=torch.uint8, device=dev)
            sel = self._detections(pred) if len(pred) else torch.zeros(0, dtype=torch.int64, device=dev)
            D, G = int(sel.numel()), len(anns)
            if iou_type == "bbox":
                b = pred["boxes"].to(dev)[sel].float() if D else torch.zeros(0, 4, device=dev)
                xywh = torch.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), dim=1).double()   # convert_to_xywh in fp32
                area = xywh[:, 2] * xywh[:, 3]
                g = torch.tensor([a["bbox"] for a in anns], dtype=torch.float64, device=dev).view(-1, 4)
                iou = _box_iou(xywh, g, crowd)
            else:
                if D and "mask_bits" in pred:
                    h, w = pred["mask_size"]
                    planes = pred["mask_bits"].to(dev)[sel]
                elif D:
                    dense = pred["masks"].to(dev)
                    h, w = dense.shape[-2:]
                    planes = k.mask_pack((dense[sel, 0] > 0.5) if dense.dtype != torch.bool else dense[sel, 0])
                if D:
                    area_i = k.mask_area(planes, h, w)
                    area = area_i.double()
                else:
                    area = torch.zeros(0, dtype=torch.float64, device=dev)
                iou = torch.zeros(D, G, dtype=torch.float64, device=dev)
                if D and G:
                    gp = self.coco_gt.planes(img, self.cat_ids, dev)
                    im = self.coco_gt.imgs[img]
                    if (im["height"], im["width"]) != (h, w):
                        raise ValueError(f"image {img}: predicted masks are {h}x{w}, the ground truth is {im['height']}x{im['width']}")
                    iou = k.mask_iou(planes, gp, crowd, area_i, k.mask_area(gp, h, w), h, w)
            ious.append(iou.reshape(-1))
            dt_area.append(area)
            gt_area.append(torch.tensor([float(a["area"]) for a in anns], dtype=torch.float64, device=dev))
            gt_crowd.append(crowd)
            scores.append(pred["scores"].to(dev)[sel].double() if D else torch.zeros(0, dtype=torch.float64, device=dev))
            n_dt.append(D)
            n_gt.append(G)
        offs = lambda sizes: torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
        A, T = len(AREA_RNG), len(IOU_THRS)
        crowd_all = torch.cat(gt_crowd) if gt_crowd else torch.zeros(0, dtype=torch.uint8, device=dev)
        dt_match, dt_ignore, gt_flag = k.coco_match(torch.cat(ious), offs([d * g for d, g in zip(n_dt, n_gt)]), torch.cat(dt_area), offs(n_dt),
                                                    torch.cat(gt_area), crowd_all, crowd_all, offs(n_gt), self._rng, self._thr)
        dt_match, dt_ignore, gt_flag = dt_match.cpu().numpy(), dt_ignore.cpu().numpy().astype(bool), gt_flag.cpu().numpy().astype(bool)
        scores_h = torch.cat(scores).cpu().numpy()
        d0 = g0 = 0
        for img, D, G in zip(img_ids, n_dt, n_gt):
            rec = {"image_id": img, "scores": scores_h[d0:d0 + D],
                   "dt_match": dt_match[A * T * d0:A * T * (d0 + D)].reshape(A, T, D),
                   "dt_ignore": dt_ignore[A * T * d0:A * T * (d0 + D)].reshape(A, T, D),
                   "gt_ignore": gt_flag[A * g0:A * (g0 + G)].reshape(A, G)}
            self.coco_eval[iou_type].records.setdefault(img, rec)                         # first evaluation of an image wins (merge: np.unique)
            d0, g0 = d0 + D, g0 + G

    # -- whole evaluation --------------------------------------------------------------------------------------------
    def synchronize_between_processes(self):
        """coco_eval.py:345-373: gather every rank's per-image tables, keep one entry per image id."""
        if not tdist.is_dist_avail_and_initialized() or tdist.get_world_size() == 1:
            return
        import torch.distributed as td
        for ev in self.coco_eval.values():
            gathered = [None] * tdist.get_world_size()
            td.all_gather_object(gathered, ev.records)
            merged = {}
            for part in gathered:
                for img, rec in part.items():
                    merged.setdefault(img, rec)
            ev.records = merged
        self.img_ids = sorted(set(i for ev in self.coco_eval.values() for i in ev.records))

    def accumulate(self):
        for ev in self.coco_eval.values():
            ev.accumulate()

    def summarize(self, verbose=True):
        for iou_type, ev in self.coco_eval.items():
            if verbose:
                print("IoU metric: {}".format(iou_type))
            ev.summarize(verbose)

    # -- result export (prepare_for_coco_segmentation, coco_eval.py:307-332) -------------------------------------------
    def segmentation_results(self, predictions):
        """[{"image_id","category_id","segmentation": {"size","counts" (compressed string)},"score"}] with the run lengths
        produced on the device."""
        out = []
        for img, pred in predictions.items():
            if len(pred) == 0:
                continue
            if "mask_bits" in pred:
                (h, w), planes = pred["mask_size"], pred["mask_bits"].to(self.device)
            else:
                dense = pred["masks"].to(self.device)
                h, w = dense.shape[-2:]
                planes = k.mask_pack(dense[:, 0] > 0.5 if dense.dtype != torch.bool else dense[:, 0])
            counts, first = k.mask_rle(planes, h, w)
            counts, first = counts.cpu().numpy(), first.cpu().numpy()
            scores, labels = pred["scores"].tolist(), pred["labels"].tolist()
            for q in range(planes.shape[0]):
                rle = {"size": [h, w], "counts": counts_to_string(counts[first[q]:first[q + 1]])}
                out.append({"image_id": img, "category_id": labels[q], "segmentation": rle, "score": scores[q]})
        return out


def _box_iou(dt, gt, crowd):
    """maskApi.c bbIou on [x, y, w, h] float64 boxes: [D, G]; crowd ground truth: union = detection area."""
    if dt.shape[0] == 0 or gt.shape[0] == 0:
        return torch.zeros(dt.shape[0], gt.shape[0], dtype=torch.float64, device=dt.device)
    da, ga = dt[:, 2] * dt[:, 3], gt[:, 2] * gt[:, 3]
    w = torch.minimum((dt[:, 2] + dt[:, 0])[:, None], (gt[:, 2] + gt[:, 0])[None]) - torch.maximum(dt[:, 0][:, None], gt[:, 0][None])
    h = torch.minimum((dt[:, 3] + dt[:, 1])[:, None], (gt[:, 3] + gt[:, 1])[None]) - torch.maximum(dt[:, 1][:, None], gt[:, 1][None])
    inter = w * h
    union = torch.where(crowd.bool()[None], da[:, None].expand_as(inter), da[:, None] + ga[None] - inter)
    return torch.where((w > 0) & (h > 0), inter / union, torch.zeros_like(inter))


# ---- a batch of PostProcess rows scored on the device (csrc/evalbox.hip) -------------------------------------------------------------
class StagedGroundTruth:
    """The device image of what COCOeval.evaluateImg reads of one or several CocoGroundTruth (a sweep has one per task), built once and uploaded
    once (staging.Staging): per annotation of the evaluated categories its bbox [x, y, w, h], its area and its crowd flag (which is also its ignore
    flag, as _evaluate passes it), grouped into SLOTS.  Slot 0 is empty and shared by every image a ground truth does not know -- update() gives such
    an image a record without ground truth --; then, ground truth by ground truth, one slot per image id in the order of CocoGroundTruth.img_anns,
    holding CocoGroundTruth.annotations(image, cat_ids) in that order (an image without annotations owns an empty slot).
      slot_off int64 [slots + 1], gt_xywh f64 [N, 4], gt_area f64 [N], gt_crowd uint8 [N] on `device` (N at least 1: a padding entry no slot names)
      slot_sizes: numpy int64 [slots], on the host; n_gt: the annotations staged
      slots(keys): keys = (ground-truth index, image id) pairs -> numpy int64 slot per key
    planes=True (what "segm" rows need: toist_coco_masks) also stages every annotation's mask, once: CocoGroundTruth.planes of every slot packed into
    ONE int64 arena, with
      gt_bits int64 [words], gt_plane_off int64 [N + 1] (word offset per annotation), slot_hw int32 [slots, 2] (the (h, w) of CocoGroundTruth.imgs; slot 0
      and a slot without annotations of a size-less image: (0, 0)), gt_parea int32 [N] (the popcount of each plane: one kernels.mask_area per slot)
      slot_hw_host: numpy int32 [slots, 2]; plane_bytes: the arena's size
    The arena's size is known from the image sizes alone: above max_plane_bytes (default 8 GiB -- a guard, not a measurement: a 480 x 640 plane is
    40 KB, so it holds about 200 000 annotations) the constructor raises ValueError naming both numbers before anything is allocated."""

    def __init__(self, ground_truths, device, cat_ids=(1,), planes=False, max_plane_bytes=8 << 30):
        from . import staging
        if isinstance(ground_truths, (CocoGroundTruth, dict)):
            ground_truths = [ground_truths]
        self.ground_truths = [g if isinstance(g, CocoGroundTruth) else CocoGroundTruth(g) for g in ground_truths]
        self.device, self.cat_ids = torch.device(device), None if cat_ids is None else tuple(cat_ids)
        self._slot, sizes, anns, owners = {}, [0], [], [None]
        for t, gt in enumerate(self.ground_truths):
            for img in gt.img_anns:
                mine = gt.annotations(img, self.cat_ids)
                self._slot[(t, img)] = len(sizes)
                sizes.append(len(mine))
                owners.append((gt, img))
                anns.extend(mine)
        self.slot_sizes, self.n_gt = np.asarray(sizes, dtype=np.int64), len(anns)
        S, N = len(sizes), max(len(anns), 1)
        self.has_planes, self.plane_bytes = bool(planes), 0
        segments = [(torch.int64, (S + 1,)), (torch.float64, (N, 4)), (torch.float64, (N,)), (torch.uint8, (N,))]
        if self.has_planes:
            hw, plane_off = self._plane_layout(owners, N)
            self.plane_bytes = 8 * int(plane_off[-1])
            if self.plane_bytes > int(max_plane_bytes):
                raise ValueError(f"StagedGroundTruth: the ground-truth planes of {len(anns)} annotations take {self.plane_bytes} bytes, above "
                                 f"max_plane_bytes = {int(max_plane_bytes)}")
            segments += [(torch.int64, (N + 1,)), (torch.int32, (S, 2))]
        views, total = staging.typed_views(segments)
        stage = staging.Staging(torch.zeros(total, dtype=torch.uint8), self.device)
        slot_off, xywh, area, crowd = views(stage.open())[:4]
        slot_off[1:] = torch.from_numpy(np.cumsum(self.slot_sizes))
        if anns:
            xywh[:len(anns)] = torch.tensor([a["bbox"] for a in anns], dtype=torch.float64).view(-1, 4)
            area[:len(anns)] = torch.tensor([float(a["area"]) for a in anns], dtype=torch.float64)
            crowd[:len(anns)] = torch.tensor([int(a.get("iscrowd", 0)) for a in anns], dtype=torch.uint8)
        if self.has_planes:
            h_off, h_hw = views(stage.host)[4:]
            h_off.copy_(torch.from_numpy(plane_off))
            h_hw.copy_(torch.from_numpy(hw))
            self.slot_hw_host = hw
        self._arena = torch.empty(total, dtype=torch.uint8, device=self.device)
        stage.upload((self._arena, stage.host))
        self._stage = stage                                   # (keeps the pinned buffer until the copy has left it)
        self.slot_off, self.gt_xywh, self.gt_area, self.gt_crowd = views(self._arena)[:4]
        if self.has_planes:
            self.gt_plane_off, self.slot_hw = views(self._arena)[4:]
            self._pack_planes(owners, hw, plane_off, N)

    def _plane_layout(self, owners, N):
        """(slot_hw int32 [slots, 2], plane_off int64 [N + 1]) from the image sizes alone: nothing is allocated on the device."""
        hw, plane_off, n = np.zeros((len(owners), 2), dtype=np.int32), np.zeros(N + 1, dtype=np.int64), 0
        for s, (owner, G) in enumerate(zip(owners, self.slot_sizes.tolist())):
            im = None if owner is None else owner[0].imgs.get(owner[1])
            if im is not None:
                hw[s] = (int(im["height"]), int(im["width"]))
            if G:
                if im is None or hw[s, 0] <= 0 or hw[s, 1] <= 0:
                    raise ValueError(f"StagedGroundTruth: image {owner[1]} has annotations but no positive height and width: its planes have no size")
                words = int(hw[s, 1]) * ((int(hw[s, 0]) + 63) // 64)
                plane_off[n + 1:n + G + 1] = plane_off[n] + words * np.arange(1, G + 1, dtype=np.int64)
                n += G
        plane_off[n + 1:] = plane_off[n]
        return hw, plane_off

    def _pack_planes(self, owners, hw, plane_off, N):
        self.gt_bits = torch.empty(int(plane_off[-1]), dtype=torch.int64, device=self.device)
        self.gt_parea = torch.zeros(N, dtype=torch.int32, device=self.device)
        n = 0
        for s, (owner, G) in enumerate(zip(owners, self.slot_sizes.tolist())):
            if not G:
                continue
            h, w = int(hw[s, 0]), int(hw[s, 1])
            planes = owner[0].planes(owner[1], self.cat_ids, self.device)
            if tuple(planes.shape) != (G, w, (h + 63) // 64):
                raise ValueError(f"image {owner[1]}: ground-truth planes of shape {tuple(planes.shape)}, the image is {h}x{w} with {G} annotations")
            self.gt_bits[int(plane_off[n]):int(plane_off[n + G])] = planes.reshape(-1)
            self.gt_parea[n:n + G] = k.mask_area(planes, h, w)
            n += G

    def slots(self, keys):
        get = self._slot.get
        return np.fromiter((get(key, 0) for key in keys), dtype=np.int64)


def row_tables(slots, slot_sizes, D):
    """The host-built tables of one batch of rows for toist_coco_boxes / toist_coco_match: slots = each row's slot, slot_sizes = the staged ground
    truth's, D = the detections kept per row -> (row_slot int32 [R], iou_off int64 [R + 1], gt_off int64 [R + 1]) as numpy arrays: exclusive prefix
    sums of D * G_r and of G_r.  ValueError for a slot outside the staged ground truth: the check the launch relies on."""
    slots, sizes = np.asarray(slots, dtype=np.int64).reshape(-1), np.asarray(slot_sizes, dtype=np.int64)
    bad = np.flatnonzero((slots < 0) | (slots >= sizes.size))
    if bad.size:
        raise ValueError(f"row {int(bad[0])}: slot {int(slots[bad[0]])} is outside the staged ground truth's {sizes.size} slots")
    G = sizes[slots]
    iou_off, gt_off = np.zeros(slots.size + 1, dtype=np.int64), np.zeros(slots.size + 1, dtype=np.int64)
    np.cumsum(G * int(D), out=iou_off[1:])
    np.cumsum(G, out=gt_off[1:])
    return slots.astype(np.int32), iou_off, gt_off


def mask_row_tables(slots, slot_sizes, slot_hw, row_hw, Q, capacity_words, D=None):
    """The host check of one batch of rows for toist_coco_masks, and its tables: slots = each row's slot, slot_sizes / slot_hw = the staged ground
    truth's (StagedGroundTruth.slot_sizes, .slot_hw_host), row_hw = each row's (h, w), Q = the planes per row, capacity_words = the words between two
    rows' planes, D = the detections kept per row (default min(Q, MAX_DETS[-1])) -> (row_slot int32 [R], iou_off int64 [R + 1], row_hw int64 [R, 2]) as
    numpy arrays.  ValueError for everything the launch relies on: a slot outside the staged ground truth, fewer planes than kept detections, a size
    that is not positive (or with 2^32 pixels or more: the counts are 32-bit), planes that overflow the capacity, and a row WITH ground truth whose
    planes are of another size than the ground truth's (a row without may be of any size, as in update())."""
    Q, capacity_words = int(Q), int(capacity_words)
    D = min(Q, MAX_DETS[-1]) if D is None else int(D)
    if Q < 0 or D < 0 or Q < D:
        raise ValueError(f"mask rows: {D} kept detections of {Q} planes per row")
    row_slot, iou_off, _ = row_tables(slots, slot_sizes, D)
    hw = np.asarray(row_hw, dtype=np.int64).reshape(-1, 2)
    slot_hw = np.asarray(slot_hw, dtype=np.int64).reshape(-1, 2)
    sizes = np.asarray(slot_sizes, dtype=np.int64)
    if hw.shape[0] != row_slot.size or slot_hw.shape[0] != sizes.size:
        raise ValueError(f"mask rows: {row_slot.size} slots for {hw.shape[0]} row sizes, {slot_hw.shape[0]} slot sizes for {sizes.size} slots")
    for r in range(hw.shape[0]):
        h, w = int(hw[r, 0]), int(hw[r, 1])
        if h <= 0 or w <= 0 or h * w >= 1 << 32:
            raise ValueError(f"row {r}: predicted masks of size {h}x{w}")
        if Q * w * ((h + 63) // 64) > capacity_words:
            raise ValueError(f"row {r}: {Q} planes of {h}x{w} take {Q * w * ((h + 63) // 64)} words, the capacity is {capacity_words}")
        s = int(row_slot[r])
        if sizes[s] > 0 and (int(slot_hw[s, 0]), int(slot_hw[s, 1])) != (h, w):
            raise ValueError(f"row {r}: predicted masks are {h}x{w}, the ground truth is {int(slot_hw[s, 0])}x{int(slot_hw[s, 1])}")
    return row_slot, iou_off, hw


class RowMasks:
    """The bit planes of a batch of rows where toist_coco_masks reads them: bits int64 [>= rows * capacity_words] on the device, row r's Q planes
    [Q, w_r, ceil(h_r/64)] from word r * capacity_words; hw_dev int64 [rows, 2] = (h, w) per row on the device; hw_host = the same as a list of int
    pairs.  CapturedEvalStep.step_rows hands out views of its bucket; pack() builds one from per-row planes."""

    def __init__(self, bits, capacity_words, hw_dev, hw_host):
        self.bits, self.capacity_words, self.hw_dev = bits, int(capacity_words), hw_dev
        self.hw_host = [(int(h), int(w)) for h, w in hw_host]

    @classmethod
    def pack(cls, planes_list, sizes, capacity_words=None):
        """planes_list: per row an int64 [Q, w, ceil(h/64)] device tensor (kernels.mask_pack, PostProcessSegm(packed=True)), sizes: per row (h, w)."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        if not planes_list or len(planes_list) != len(sizes):
            raise ValueError(f"RowMasks.pack: {len(planes_list)} rows of planes, {len(sizes)} sizes")
        for p, (h, w) in zip(planes_list, sizes):
            if p.dim() != 3 or tuple(p.shape[1:]) != (w, (h + 63) // 64) or p.dtype != torch.int64:
                raise ValueError(f"RowMasks.pack: planes of shape {tuple(p.shape)} ({p.dtype}) for a row of size {h}x{w}")
        need = max(int(p.numel()) for p in planes_list)
        cap = need if capacity_words is None else int(capacity_words)
        if cap < need:
            raise ValueError(f"RowMasks.pack: a row of {need} words, the capacity is {cap}")
        dev = planes_list[0].device
        bits = torch.zeros(len(sizes) * cap, dtype=torch.int64, device=dev)
        for r, p in enumerate(planes_list):
            bits[r * cap:r * cap + p.numel()] = p.reshape(-1)
        return cls(bits, cap, torch.tensor(sizes, dtype=torch.int64).to(dev), sizes)


class _RowScorer:
    """What update_rows runs per batch, for one evaluator or for all of a SweepEvaluator's: the per-batch tables through one staging.Staging, the two
    launches, and the match tables on their way to the host in a staging.Mailbox with the bookkeeping that turns them into records.  All state
    hangs off the evaluator that owns the scorer: no process-wide cache, nothing keyed by table contents."""

    def __init__(self, staged, device):
        from . import staging
        self.staged, self.device = staged, torch.device(device)
        self.mail = staging.Mailbox()
        self._meta = []                   # one entry per posted batch, oldest first: (D, [(IouTypeEval, image id, G) per row])
        self._rows, self._stage, self._tables, self._views = 0, None, None, None
        self._thr = torch.from_numpy(IOU_THRS).to(self.device)
        self._rng = torch.from_numpy(AREA_RNG).to(self.device)

    def _grow(self, R):
        from . import staging
        if R > self._rows:
            self._views, total = staging.typed_views([(torch.int32, (R,)), (torch.int64, (R + 1,)), (torch.int64, (R + 1,)), (torch.int64, (R + 1,))])
            self._stage = staging.Staging(torch.zeros(total, dtype=torch.uint8), self.device)
            self._tables = torch.empty(total, dtype=torch.uint8, device=self.device)
            self._rows = R

    def score(self, out, slots, targets, masks=None, types=("bbox",)):
        """Score the first len(targets) rows of `out`: slots = each row's slot (numpy), targets = each row's (IouTypeEval, image id) -- or, for several
        `types`, ({iou type: IouTypeEval}, image id).  "segm" needs masks = the rows' RowMasks and a ground truth staged with planes=True."""
        scores, boxes = out["scores"], out["boxes"]
        R = len(targets)
        if scores.dim() != 2 or R > scores.shape[0] or len(slots) != R:
            raise ValueError(f"update_rows: {R} rows to score, {len(slots)} slots, scores of shape {tuple(scores.shape)}")
        Q = int(scores.shape[1])
        D = min(Q, MAX_DETS[-1])
        row_slot, iou_off, gt_off = row_tables(slots, self.staged.slot_sizes, D)              # ValueError before anything is launched
        segm = "segm" in types
        if segm:
            st = self.staged
            if masks is None or not getattr(st, "has_planes", False):
                raise ValueError("update_rows: 'segm' rows need masks=RowMasks and a ground truth staged with its planes (StagedGroundTruth(planes=True))")
            if len(masks.hw_host) < R or masks.hw_dev.dim() != 2 or masks.hw_dev.shape[0] < R:
                raise ValueError(f"update_rows: {R} rows to score, masks of {len(masks.hw_host)} rows")
            mask_row_tables(slots, st.slot_sizes, st.slot_hw_host, masks.hw_host[:R], Q, masks.capacity_words, D)
        self.drain(wait=False)
        if R == 0:
            return
        if not scores.is_cuda:
            raise RuntimeError("update_rows scores its rows on the GPU (toist_coco_boxes, toist_coco_match); there is no CPU path")
        self._grow(R)
        h_slot, h_iou, h_gt, h_dt = self._views(self._stage.open())
        h_slot[:R], h_iou[:R + 1], h_gt[:R + 1] = torch.from_numpy(row_slot), torch.from_numpy(iou_off), torch.from_numpy(gt_off)
        h_dt[:R + 1] = torch.arange(R + 1, dtype=torch.int64) * D
        self._stage.upload((self._tables, self._stage.host))
        d_slot, d_iou, d_gt, d_dt = (v[:n] for v, n in zip(self._views(self._tables), (R, R + 1, R + 1, R + 1)))
        st = self.staged
        got = k.coco_boxes(scores[:R], boxes[:R], MAX_DETS[-1], d_slot, st.slot_off, st.gt_xywh, st.gt_area, st.gt_crowd, d_iou, d_gt,
                           int(iou_off[-1]), int(gt_off[-1]))
        G = (gt_off[1:] - gt_off[:-1]).tolist()
        pick = lambda ev, t: ev[t] if isinstance(ev, dict) else ev
        for t in types:
            if t == "bbox":
                iou, dt_area = got["iou"], got["dt_area"]
            elif t == "segm":
                mk = k.coco_masks(masks.bits, masks.capacity_words, masks.hw_dev[:R], Q, got["order"], d_slot, st.slot_off, st.gt_bits, st.gt_plane_off,
                                  st.slot_hw, st.gt_parea, st.gt_crowd, d_iou, int(iou_off[-1]))
                iou, dt_area = mk["iou"], mk["dt_area"]
            else:
                raise ValueError("Unknown iou type {}".format(t))
            dt_match, dt_ignore, gt_flag = k.coco_match(iou, d_iou, dt_area, d_dt, got["gt_area"], got["gt_crowd"], got["gt_crowd"], d_gt, self._rng,
                                                        self._thr)
            packed = torch.cat([got["dt_score"].view(torch.uint8), dt_match.view(torch.uint8), dt_ignore, gt_flag])
            self.post(packed, (D, [(pick(ev, t), img, g) for (ev, img), g in zip(targets, G)]))

    def post(self, packed, meta):
        """Queue one batch's tables (uint8: dt_score f64 [R * D], dt_match int32 [A * T * R * D], dt_ignore [A * T * R * D], gt_flag [A * sum G]) with what
        files them."""
        queued = len(self.mail)
        self.mail.post(packed)
        if len(self.mail) != queued + 1:
            raise RuntimeError("update_rows: the match tables could not be queued for the host (a host tensor, or a stream that is capturing)")
        self._meta.append(meta)

    def drain(self, wait=True):
        """File the batches whose tables have arrived, oldest first (wait=True: all of them)."""
        for host in self.mail.drain(wait=wait, ordered=True):
            self._file(host.numpy().copy(), *self._meta.pop(0))              # (a copy: the records do not hold on to pinned memory)

    @staticmethod
    def _file(buf, D, rows):
        A, T, R = len(AREA_RNG), len(IOU_THRS), len(rows)
        n_dt, n_gt = R * D, sum(g for _, _, g in rows)
        cut = np.cumsum([0, 8 * n_dt, 4 * A * T * n_dt, A * T * n_dt, A * n_gt])
        if buf.size != cut[-1]:
            raise RuntimeError(f"update_rows: {buf.size} bytes arrived for a batch whose tables hold {int(cut[-1])}")
        scores, dt_match = buf[cut[0]:cut[1]].view(np.float64), buf[cut[1]:cut[2]].view(np.int32)
        dt_ignore, gt_flag = buf[cut[2]:cut[3]].astype(bool), buf[cut[3]:cut[4]].astype(bool)
        g0 = 0
        for r, (ev, img, G) in enumerate(rows):
            d0 = r * D
            rec = {"image_id": img, "scores": scores[d0:d0 + D],
                   "dt_match": dt_match[A * T * d0:A * T * (d0 + D)].reshape(A, T, D),
                   "dt_ignore": dt_ignore[A * T * d0:A * T * (d0 + D)].reshape(A, T, D),
                   "gt_ignore": gt_flag[A * g0:A * (g0 + G)].reshape(A, G)}
            ev._records.setdefault(img, rec)                                  # first evaluation of an image wins, also inside a batch
            g0 += G


class SweepEvaluator:
    """A task sweep scored on the device: one TDODCocoEvaluator(gt, iou_types) per task over ONE StagedGroundTruth, all rows of a batch in two launches
    per iou type (+ toist_coco_masks for "segm").
    ground_truths = {task name: CocoGroundTruth or COCO-format dict}.  iou_types: ("bbox",) -- the default, a detection model's sweep: update_rows
    takes no masks and the ground truth is staged without planes -- or any of ("bbox", "segm"): with "segm" the ground truth is staged with its planes
    (StagedGroundTruth(planes=True)) and update_rows needs masks = the RowMasks of the rows (CapturedMaskSweepStep.step_rows hands one out,
    RowMasks.pack builds one from PostProcessSegm(packed=True)'s planes).  COCO-Tasks' number is mAP@0.5 per task and its mean over the tasks:
    summarize() -> {"tasks": {name: the 12 box stats}, "mAP50": mean over the tasks of stats[1], "mAP": mean of stats[0]} (plain means over every
    task, a task without ground truth counts with pycocotools' -1) and, with "segm", "segm": {"tasks", "mAP50", "mAP"} of the mask stats beside them
    (iou_types == ("segm",): the top-level numbers are the mask numbers too)."""

    def __init__(self, ground_truths, device="cuda", iou_types=("bbox",)):
        self.device = torch.device(device)
        if isinstance(iou_types, str) or not isinstance(iou_types, (list, tuple)):
            raise ValueError(f"SweepEvaluator: iou_types is a tuple within ('bbox', 'segm') (got {iou_types!r})")
        self.iou_types = tuple(iou_types)
        if not self.iou_types or any(t not in ("bbox", "segm") for t in self.iou_types) or len(set(self.iou_types)) != len(self.iou_types):
            raise ValueError(f"SweepEvaluator: iou_types is a non-empty tuple of distinct types within ('bbox', 'segm') (got {iou_types!r})")
        gts = {name: g if isinstance(g, CocoGroundTruth) else CocoGroundTruth(g) for name, g in ground_truths.items()}
        if not gts:
            raise ValueError("SweepEvaluator needs at least one task")
        self.evaluators = {name: TDODCocoEvaluator(g, list(self.iou_types), device=self.device) for name, g in gts.items()}
        self.staged = StagedGroundTruth(list(gts.values()), self.device, planes="segm" in self.iou_types)
        self._scorer = _RowScorer(self.staged, self.device)
        self._index = {name: t for t, name in enumerate(gts)}
        for name, t in self._index.items():
            self.evaluators[name]._attach(self._scorer, t)

    def update_rows(self, out, image_ids, task_names, pair_image, pair_caption, live=None, masks=None):
        """Score the first `live` rows of out = kernels.postprocess's dict: row p is caption task_names[pair_caption[p]] on image
        image_ids[pair_image[p]] (the tables of sweep.pair_tables / CapturedSweepStep.step_rows).  Every task named by a live row must be one of
        this evaluator's.  masks: the rows' RowMasks, needed by (and only read for) "segm".  No host synchronisation: see
        TDODCocoEvaluator.update_rows."""
        from .sweep import _index_list
        if "segm" in self.iou_types:
            if masks is None:
                raise ValueError("SweepEvaluator(iou_types with 'segm').update_rows needs masks = the rows' coco_eval.RowMasks")
            if not isinstance(masks, RowMasks):
                raise TypeError(f"update_rows: masks is a coco_eval.RowMasks (got {type(masks).__name__})")
        pi, pc = _index_list(pair_image, "pair_image"), _index_list(pair_caption, "pair_caption")
        live = len(pi) if live is None else int(live)
        if len(pc) != len(pi) or not 0 <= live <= len(pi):
            raise ValueError(f"update_rows: tables of {len(pi)} and {len(pc)} pairs, {live} of them live")
        ids = [int(i) if torch.is_tensor(i) else i for i in image_ids]
        keys, targets, seen = [], [], {}
        boxes_only = self.iou_types == ("bbox",)
        for p in range(live):
            name = task_names[pc[p]]
            if name not in self._index:
                raise ValueError(f"update_rows: pair {p} names task {name!r}, which this SweepEvaluator has no ground truth for")
            img = ids[pi[p]]
            keys.append((self._index[name], img))
            evs = self.evaluators[name].coco_eval
            targets.append((evs["bbox"] if boxes_only else evs, img))
            seen.setdefault(name, set()).add(img)
        if boxes_only:
            self._scorer.score(out, self.staged.slots(keys), targets)
        else:
            self._scorer.score(out, self.staged.slots(keys), targets, masks=masks if "segm" in self.iou_types else None, types=self.iou_types)
        for name, imgs in seen.items():
            self.evaluators[name].img_ids.extend(sorted(imgs))

    def synchronize_between_processes(self):
        self._scorer.drain()
        for ev in self.evaluators.values():
            ev.synchronize_between_processes()

    def accumulate(self):
        self._scorer.drain()
        for ev in self.evaluators.values():
            ev.accumulate()

    def summarize(self, verbose=False):
        for name, ev in self.evaluators.items():
            if verbose:
                print(f"task {name}")
            ev.summarize(verbose)

        def numbers(iou_type):
            tasks = {name: ev.coco_eval[iou_type].stats for name, ev in self.evaluators.items()}
            return {"tasks": tasks, "mAP50": float(np.mean([s[1] for s in tasks.values()])), "mAP": float(np.mean([s[0] for s in tasks.values()]))}

        iou_types = getattr(self, "iou_types", ("bbox",))
        out = numbers("bbox" if "bbox" in iou_types else "segm")
        if "segm" in iou_types:
            out["segm"] = numbers("segm")
        return out
