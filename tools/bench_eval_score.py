"""Scoring a captured evaluation on one MI355X: batches of B = 8 images at 640 x 640 (originals 480 x 640) through a CapturedEvalStep with the mask
head, Q = 100 queries, a seeded ground truth of 0-10 objects (box + mask) per image, TDODCocoEvaluator(["bbox", "segm"]).  The legs alternate batch by
batch inside one process, each figure the median over `--batches` batches:
  a  update_ms            the evaluator as it was: update() on step()'s 8 per-image dicts (it reads its tables back, so it ends synchronised)
  b  update_rows_ms       update_rows(out, ids, masks=masks) on step_rows()' views of the same batch: toist_coco_boxes, toist_coco_masks and two
                          toist_coco_match, then a device synchronise and the drain of the Mailbox (the whole latency of a batch;
                          update_rows_issue_ms is the host time of the call alone, which is what a loop pays)
  c  replay_ms            the CapturedEvalStep replay alone (step_rows: upload, graph launch, status read), synchronised
  d  scored_images_per_s  the scored loop, step_rows + update_rows per batch over a region of `--batches` batches ending in a synchronise and the drain,
                          beside unscored_images_per_s: the same region without update_rows
and the toist_coco_masks launch alone (HIP events around a hipGraph of 20 launches on the same rows, per launch, median of 30) against its traffic
floor: the R * D detection planes read once plus each row's G ground-truth planes once, over the HBM rate measured on this part (6.3 TB/s).  The ground truth is cut from seeded rectangles, so
most detections match nothing -- the cost of the path does not depend on it.  Every timed step is held to `--step-limit` seconds (the tool stops at
the first that takes longer; a hang is the caller's time limit to end).  Prints ONE JSON line and writes it to profiles/eval_score.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_MEASURED = 6.3e12      # bytes/s
LAUNCHES = 20              # toist_coco_masks launches per timed graph replay


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def rectangle_rle(x, y, bw, bh, h, w):
    """Column-major run lengths (zeros first) of the rectangle [y, y + bh) x [x, x + bw) in an h x w mask."""
    counts = [x * h + y]
    for _ in range(bw - 1):
        counts += [bh, h - bh]
    return counts + [bh, h * w - ((x + bw - 1) * h + y + bh)]


def ground_truth(image_ids, hw, seed):
    """COCO-format dict: 0-10 objects per image, seeded; boxes and RLE segmentations of the same rectangles."""
    rng = np.random.default_rng(seed)
    h, w = hw
    anns = []
    for img in image_ids:
        for _ in range(int(rng.integers(0, 11))):
            bw, bh = int(rng.integers(8, w // 2)), int(rng.integers(8, h // 2))
            x, y = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "iscrowd": int(rng.random() < 0.05), "bbox": [float(x), float(y), float(bw), float(bh)],
                         "area": float(bw * bh), "segmentation": {"size": [h, w], "counts": rectangle_rle(x, y, bw, bh, h, w)}})
    return {"images": [{"id": i, "height": h, "width": w} for i in image_ids], "annotations": anns}


def run(a):
    import toist_amd
    from toist_amd import coco_eval as C, harness, kernels as k
    dev = torch.device("cuda:0")
    B, L, N = a.batch, 16, a.batches
    orig_hw = (480, 640)
    orig, sizes = [orig_hw] * B, [(a.size, a.size)] * B
    torch.manual_seed(0)
    args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", contrastive_align_loss=False)
    model = toist_amd.build_model(args)[0].to(dev).eval()
    batches = [harness.synthetic_batch(B, a.size, a.size, tokens=L, seed=500 + i, device=dev, max_targets=0)[:2] for i in range(N)]
    ids = [[n * B + i for i in range(B)] for n in range(N)]
    data = C.CocoGroundTruth(ground_truth([i for b in ids for i in b], orig_hw, seed=5))
    step = harness.CapturedEvalStep(model, batch=B, max_orig_hw=orig_hw, pad_hw=64)
    Q = step.num_queries
    types = ["bbox", "segm"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if ms > a.step_limit * 1e3:
            raise SystemExit(f"bench_eval_score: a step took {ms:.0f} ms, above --step-limit {a.step_limit} s")
        return ms, r

    def leg_a(ev, n):
        results = step.step(*batches[n], orig, sizes)                  # (the same replay: the dicts are views of the rows leg b read)
        torch.cuda.synchronize()
        return timed(lambda: ev.update(dict(zip(ids[n], results))))[0]

    def leg_b(ev, n, out, masks):
        def body():
            t0 = time.perf_counter()
            ev.update_rows(out, ids[n], masks=masks)
            issue = time.perf_counter() - t0
            torch.cuda.synchronize()
            ev._scorer.drain()
            return issue
        return timed(body)

    fresh = lambda: C.TDODCocoEvaluator(data, types, device=dev)
    ms = {"a": [], "b": [], "b_issue": [], "c": []}
    with torch.no_grad():
        ev_a, ev_b = fresh(), fresh()
        t_stage, _ = timed(lambda: ev_b._row_scorer())                 # the ground-truth planes, staged once per evaluation
        for n in range(min(a.warmup, N)):                              # every leg once on every shape it uses, before any clock starts
            out, masks = step.step_rows(*batches[n], orig, sizes)
            leg_b(ev_b, n, out, masks)
            leg_a(ev_a, n)
        staged = ev_b._scorer.staged
        ev_a, ev_b = fresh(), fresh()
        ev_b._attach(C._RowScorer(staged, dev), 0)                     # (the staged planes are the evaluation's, not the timed call's)
        for n in range(N):                                             # alternated batch by batch
            t_c, (out, masks) = timed(lambda: step.step_rows(*batches[n], orig, sizes))
            ms["c"].append(t_c)
            t_b, issue = leg_b(ev_b, n, out, masks)
            ms["b"].append(t_b)
            ms["b_issue"].append(issue * 1e3)
            ms["a"].append(leg_a(ev_a, n))
        same = all(np.array_equal(ev_b.coco_eval[t].records[i][key], ev_a.coco_eval[t].records[i][key])
                   for t in types for i in ev_a.coco_eval[t].records for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"))
        same = same and all(sorted(ev_b.coco_eval[t].records) == sorted(ev_a.coco_eval[t].records) for t in types)

        def region(scored):
            ev = fresh() if scored else None
            if scored:
                ev._attach(C._RowScorer(staged, dev), 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(N):
                out, masks = step.step_rows(*batches[n], orig, sizes)
                if scored:
                    ev.update_rows(out, ids[n], masks=masks)
            torch.cuda.synchronize()
            if scored:
                ev._scorer.drain()
            return N * B / (time.perf_counter() - t0)
        rates = {"scored": [], "unscored": []}
        for _ in range(a.repeats):
            for kind in ("unscored", "scored"):
                rates[kind].append(region(kind == "scored"))

        # the toist_coco_masks launch alone, on the last batch's rows
        out, masks = step.step_rows(*batches[N - 1], orig, sizes)
        slots = staged.slots([(0, i) for i in ids[N - 1]])
        D = min(Q, C.MAX_DETS[-1])
        row_slot, iou_off, gt_off = C.row_tables(slots, staged.slot_sizes, D)
        C.mask_row_tables(slots, staged.slot_sizes, staged.slot_hw_host, masks.hw_host, Q, masks.capacity_words, D)
        d_slot, d_iou, d_gt = (torch.from_numpy(t).to(dev) for t in (row_slot, iou_off, gt_off))
        got = k.coco_boxes(out["scores"], out["boxes"], C.MAX_DETS[-1], d_slot, staged.slot_off, staged.gt_xywh, staged.gt_area, staged.gt_crowd, d_iou, d_gt,
                           int(iou_off[-1]), int(gt_off[-1]))
        buf = {"dt_area": torch.empty(B * D, dtype=torch.float64, device=dev), "iou": torch.empty(int(iou_off[-1]), dtype=torch.float64, device=dev)}
        launch = lambda: k.coco_masks(masks.bits, masks.capacity_words, masks.hw_dev, Q, got["order"], d_slot, staged.slot_off, staged.gt_bits,
                                      staged.gt_plane_off, staged.slot_hw, staged.gt_parea, staged.gt_crowd, d_iou, int(iou_off[-1]), out=buf)
        launch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()                                  # LAUNCHES launches in one graph: device time, not the host's launch gap
        with torch.cuda.graph(graph):
            for _ in range(LAUNCHES):
                launch()
        graph.replay()
        kernel_ms = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            kernel_ms.append(e0.elapsed_time(e1) / LAUNCHES)
        plane = 8 * orig_hw[1] * ((orig_hw[0] + 63) // 64)
        floor_bytes = B * D * plane + int(gt_off[-1]) * plane
        for e in (ev_a,):
            e.accumulate()
            e.summarize(verbose=False)
    a_ms, b_ms, c_ms, k_ms = _median(ms["a"]), _median(ms["b"]), _median(ms["c"]), _median(kernel_ms)
    return {"tool": "tools/bench_eval_score.py", "device": "MI355X",
            "workload": {"images_per_batch": B, "queries": Q, "image_hw": [a.size, a.size], "orig_hw": list(orig_hw), "batches": N, "iou_types": types,
                         "ground_truth_objects": len(data.dataset["annotations"]), "ground_truth_plane_bytes": staged.plane_bytes, "region_repeats": a.repeats},
            "a_update_ms": a_ms, "b_update_rows_ms": b_ms, "b_update_rows_issue_ms": _median(ms["b_issue"]), "c_replay_ms": c_ms,
            "d_scored_images_per_s": _median(rates["scored"]), "unscored_images_per_s": _median(rates["unscored"]),
            "a_over_b": a_ms / b_ms, "b_below_a": b_ms < a_ms, "b_below_c": b_ms < c_ms, "stage_ground_truth_once_ms": t_stage,
            "coco_masks_launch_ms": k_ms, "coco_masks_traffic_floor_ms": floor_bytes / HBM_MEASURED * 1e3, "coco_masks_floor_bytes": floor_bytes,
            "coco_masks_floor_fraction": floor_bytes / HBM_MEASURED * 1e3 / k_ms, "coco_masks_rows_ground_truth": int(gt_off[-1]),
            "all_ms": ms, "all_images_per_s": rates, "records_equal": bool(same),
            "segm_mAP50": float(ev_a.coco_eval["segm"].stats[1]), "bbox_mAP50": float(ev_a.coco_eval["bbox"].stats[1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=24, help="batches per leg (the median is over them) and per region of the loop; at least 20")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=60.0, help="seconds one timed step may take before the tool stops")
    ap.add_argument("--out", default=os.path.join("profiles", "eval_score.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_score: no GPU; nothing is measured without one")

    def rnd(v):
        if isinstance(v, float):
            return round(v, 3) if abs(v) >= 1 else float(f"{v:.3g}")
        if isinstance(v, list):
            return [rnd(x) for x in v]
        if isinstance(v, dict):
            return {k_: rnd(x) for k_, x in v.items()}
        return v

    out = rnd(run(a))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
