"""Scoring a task sweep on one MI355X: B = 8 images x T = 14 task captions = 112 PostProcess rows of Q = 100 queries per batch, a seeded ground truth of
0-10 boxes per (image, task).  Four figures, the legs alternating batch by batch inside one process, each the median over `--batches` batches:
  a  update_per_task_ms   the evaluator as it was: one TDODCocoEvaluator per task, update() on that task's 8 keyed results (14 calls per batch; the
                          call reads its tables back, so it ends synchronised)
  b  update_rows_ms       SweepEvaluator.update_rows on the same 112 rows: two launches, then a device synchronise and the drain of the Mailbox (the
                          whole latency of a batch; update_rows_issue_ms is the host time of the call alone, which is what a loop pays)
  c  replay_ms            the CapturedSweepStep replay alone (step_rows: upload, graph launch, status read), synchronised
  d  scored_pairs_per_s   the scored loop, step_rows + update_rows per batch over a region of `--batches` batches ending in a synchronise and the drain,
                          beside unscored_pairs_per_s: the same region without update_rows
The rows of (a) and (b) are the captured sweep's own outputs for that batch, cloned; the ground truth is cut from seeded boxes, so most detections
match nothing -- the cost of the path does not depend on it.  Prints ONE JSON line and writes it to profiles/sweep_score.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def ground_truth(names, image_ids, hw, seed):
    """{task: COCO-format dict}: 0-10 boxes per (image, task), seeded."""
    rng = np.random.default_rng(seed)
    h, w = hw
    out = {}
    for name in names:
        anns = []
        for img in image_ids:
            for _ in range(int(rng.integers(0, 11))):
                bw, bh = float(rng.integers(8, w // 2)), float(rng.integers(8, h // 2))
                x, y = float(rng.integers(0, w - int(bw))), float(rng.integers(0, h - int(bh)))
                anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "iscrowd": int(rng.random() < 0.05), "bbox": [x, y, bw, bh], "area": bw * bh})
        out[name] = {"images": [{"id": i, "height": h, "width": w} for i in image_ids], "annotations": anns}
    return out


def run(a):
    import toist_amd
    from toist_amd import coco_eval as C, harness, sweep
    dev = torch.device("cuda:0")
    B, T, L, N = a.batch, a.captions, 16, a.batches
    orig = [(480, 640)] * B
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cuda"))[0].to(dev).eval()
    Q = model.query_embed.weight.shape[0]
    _, captions, _, _ = harness.synthetic_batch(T, 32, 32, tokens=L, seed=77, device=dev, max_targets=0)
    batches = [harness.synthetic_batch(B, a.size, a.size, tokens=L, seed=900 + i, device=dev, max_targets=0)[0] for i in range(N)]
    ids = [[n * B + i for i in range(B)] for n in range(N)]
    names = [f"task_{t + 1}" for t in range(T)]
    data = ground_truth(names, [i for b in ids for i in b], orig[0], seed=5)
    step = harness.CapturedSweepStep(model, batch=B, captions=T, pad_hw=64)
    labels = torch.ones(Q, dtype=torch.int64, device=dev)

    def rows_of(n):
        out, pi, pc, live = step.step_rows(batches[n], captions, orig)
        return {k_: v.clone() for k_, v in out.items()}, pi, pc, live

    def fresh():
        return {n: C.TDODCocoEvaluator(data[n], ["bbox"], device=dev) for n in names}, C.SweepEvaluator(data, dev)

    def leg_a(per_task, n, rows, pi, pc, live):
        keyed = sweep.keyed_results([{"scores": rows["scores"][p], "labels": labels, "boxes": rows["boxes"][p]} for p in range(live)], ids[n], names, pi, pc, live)
        for name in names:
            per_task[name].update({img: r for (img, task), r in keyed.items() if task == name})

    def leg_b(sw, n, rows, pi, pc, live):
        t0 = time.perf_counter()
        sw.update_rows(rows, ids[n], names, pi, pc, live)
        issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        sw._scorer.drain()
        return issue

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    ms = {"a": [], "b": [], "b_issue": [], "c": []}
    with torch.no_grad():
        per_task, sw = fresh()
        for n in range(min(a.warmup, N)):                              # every leg once on every shape it uses, before any clock starts
            rows, pi, pc, live = rows_of(n)
            leg_a(per_task, n, rows, pi, pc, live)
            leg_b(sw, n, rows, pi, pc, live)
        per_task, sw = fresh()
        for n in range(N):                                             # alternated batch by batch
            t_c, (rows, pi, pc, live) = timed(lambda: rows_of(n))
            ms["c"].append(t_c)
            ms["a"].append(timed(lambda: leg_a(per_task, n, rows, pi, pc, live))[0])
            t_b, issue = timed(lambda: leg_b(sw, n, rows, pi, pc, live))
            ms["b"].append(t_b)
            ms["b_issue"].append(issue * 1e3)
        # the two evaluators saw the same rows: the same records
        same = all(np.array_equal(sw.evaluators[n].coco_eval["bbox"].records[i][key], per_task[n].coco_eval["bbox"].records[i][key])
                   for n in names for i in per_task[n].coco_eval["bbox"].records for key in ("scores", "dt_match", "dt_ignore", "gt_ignore"))

        def region(scored):
            sw = C.SweepEvaluator(data, dev) if scored else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(N):
                out, pi, pc, live = step.step_rows(batches[n], captions, orig)
                if scored:
                    sw.update_rows(out, ids[n], names, pi, pc, live)
            torch.cuda.synchronize()
            if scored:
                sw._scorer.drain()
            return N * B * T / (time.perf_counter() - t0)
        rates = {"scored": [], "unscored": []}
        for _ in range(a.repeats):
            for kind in ("unscored", "scored"):
                rates[kind].append(region(kind == "scored"))
        sw.synchronize_between_processes()
        sw.accumulate()
        summary = sw.summarize()
    return {"tool": "tools/bench_sweep_score.py", "device": "MI355X",
            "workload": {"images_per_batch": B, "captions": T, "rows_per_batch": B * T, "queries": Q, "image_hw": [a.size, a.size], "batches": N,
                         "ground_truth_boxes": sum(len(d["annotations"]) for d in data.values()), "region_repeats": a.repeats},
            "a_update_per_task_ms": _median(ms["a"]), "b_update_rows_ms": _median(ms["b"]), "b_update_rows_issue_ms": _median(ms["b_issue"]),
            "c_replay_ms": _median(ms["c"]), "d_scored_pairs_per_s": _median(rates["scored"]), "unscored_pairs_per_s": _median(rates["unscored"]),
            "a_over_b": _median(ms["a"]) / _median(ms["b"]), "b_under_c": _median(ms["b"]) < _median(ms["c"]),
            "all_ms": ms, "all_pairs_per_s": rates, "records_equal": bool(same), "mAP50": summary["mAP50"], "mAP": summary["mAP"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--captions", type=int, default=14)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", type=int, default=24, help="batches per leg (the median is over them) and per region of the loop")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "sweep_score.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep_score: no GPU; nothing is measured without one")

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
