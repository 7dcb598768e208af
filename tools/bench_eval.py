"""Evaluation throughput on one MI355X: the eager evaluation body of harness.evaluate against harness.CapturedEvalStep (one hipGraph per shape bucket).

Default run: a synthetic stream of batches of 8 images of 640 x 640 with 16-token captions (a different batch every step), under the default
detection recipe and under --masks (segmentation head, 800 x 160 x 160 mask logits per batch, 480 x 640 originals); per recipe three timed regions
of N batches each, repeated and alternated:
  eager      encode -> decode -> PostProcess (-> PostProcessSegm(packed=True)) -> status check, launched op by op (the loop body of harness.evaluate)
  captured   CapturedEvalStep.step: one upload + one graph launch + status check
  postproc   the two post-processing kernels alone (toist_postprocess, toist_mask_resize_pack_batch) against the torch ops / per-image launches
Every recipe runs in a child process of its own under a time limit; a child that fails ends the run.  Prints ONE JSON line (images/s per region, the
ratio captured / eager) and writes the same to profiles/eval_captured.json.  Timings are host clocks around regions that end in a device
synchronisation; the postproc region uses HIP events.

--micro: the evaluation-path microbenchmark at BASELINE size (fused PostProcessSegm kernel against the reference's arithmetic as device torch ops,
device RLE encode, popcount IoU, the batched matching kernel, one whole TDODCocoEvaluator.update); prints one JSON object.
"""
import json
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from toist_amd import coco_eval as C, kernels as k          # noqa: E402
from toist_amd.postprocessors import PostProcessSegm        # noqa: E402


def timed(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def micro():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Q, h0, H, W, PAD = 8, 100, 160, 480, 640, 640
    pred = torch.randn(B, Q, 1, h0, h0, device=dev) * 2 - 1
    sizes, origs = torch.tensor([[PAD, PAD]] * B, device=dev), torch.tensor([[H, W]] * B, device=dev)
    out = {}

    def fused():
        return PostProcessSegm(packed=True)([{} for _ in range(B)], {"pred_masks": pred}, origs, sizes)

    def torch_path(to_host):
        m = F.interpolate(pred.squeeze(2), size=(PAD, PAD), mode="bilinear", align_corners=False)
        m = F.interpolate(m, size=(H, W), mode="bilinear").sigmoid() > 0.5
        return m.cpu() if to_host else m
    t_f = timed(fused)
    out["postprocess_fused_ms"] = t_f
    out["postprocess_torch_device_only_ms"] = timed(lambda: torch_path(False), iters=5)
    out["postprocess_torch_with_dense_d2h_ms"] = timed(lambda: torch_path(True), iters=3, warm=1)
    alg = B * Q * (h0 * h0 * 4 + W * ((H + 63) // 64) * 8)
    out["postprocess_fused_algorithmic_bytes"] = alg
    out["postprocess_fused_GBps"] = alg / t_f / 1e6
    out["postprocess_fused_Gpixel_per_s"] = B * Q * H * W / t_f / 1e6
    res = fused()
    bits = torch.cat([r["mask_bits"] for r in res])                      # [800, W, 8]
    plane_bytes = bits.numel() * 8
    t = timed(lambda: k.mask_area(bits, H, W))
    out["area_ms"], out["area_GBps"] = t, plane_bytes / t / 1e6
    t = timed(lambda: k.mask_rle(bits, H, W), iters=5)
    counts, first = k.mask_rle(bits, H, W)
    out["rle_encode_800_masks_ms"], out["rle_runs"] = t, int(counts.numel())
    gt = bits[:10]
    area = k.mask_area(bits, H, W)
    crowd = torch.zeros(10, dtype=torch.uint8, device=dev)
    t = timed(lambda: k.mask_iou(bits[:100], gt, crowd, area[:100], area[:10], H, W))
    out["iou_100x10_ms"], out["iou_100x10_GBps_L2"] = t, 100 * 10 * 2 * (plane_bytes / 800) / t / 1e6
    # whole evaluator step: 8 images x 100 packed detections, 5 ground-truth masks each
    images = [{"id": i + 1, "height": H, "width": W} for i in range(B)]
    anns = []
    for i in range(B):
        dense = k.mask_unpack(res[i]["mask_bits"][:5], H, W).cpu().numpy()
        for q in range(5):
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": 1, "iscrowd": 0, "area": float(dense[q].sum()),
                         "bbox": [0.0, 0.0, float(W), float(H)], "segmentation": dense[q]})
        res[i]["scores"], res[i]["labels"] = torch.rand(Q, device=dev), torch.ones(Q, dtype=torch.int64, device=dev)
        res[i]["boxes"] = torch.rand(Q, 4, device=dev) * 100
    ev = C.TDODCocoEvaluator({"images": images, "annotations": anns}, ["bbox", "segm"], device=dev)
    ev.update({i + 1: res[i] for i in range(B)})                          # packs the ground truth once
    t0 = time.perf_counter()
    for _ in range(5):
        ev.update({i + 1: res[i] for i in range(B)})
    torch.cuda.synchronize()
    out["evaluator_update_bbox_and_segm_ms"] = (time.perf_counter() - t0) / 5 * 1e3
    # CPU baseline: the oracle's encode + run-merging IoU (pure Python, as a port) on a bounded sample
    from oracle import coco_ref as R
    dense = k.mask_unpack(bits[:4], H, W).cpu().numpy()
    t0 = time.perf_counter()
    rles = [R.rle_encode(m) for m in dense]
    R.rle_iou(rles, rles[:2], [0, 0])
    out["cpu_oracle_encode4_iou4x2_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in out.items()}))


# ---- eager evaluation body against the captured step ----------------------------------------------------------------------------------
def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def leg(masks, steps, warmup, repeats):
    """One recipe in this process -> dict of figures."""
    import toist_amd
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess
    dev = torch.device("cuda:0")
    B, H, W, L = 8, 640, 640, 16
    orig_hw = (480, 640)
    args = harness.default_args(device="cuda", masks=masks, mask_model="smallconv" if masks else "none", contrastive_align_loss=not masks)
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    model.to(dev).eval()
    batches = []
    for i in range(steps):
        samples, tok, _, _ = harness.synthetic_batch(B, H, W, tokens=L, seed=500 + i, device=dev, max_targets=0)
        batches.append((samples, tok))
    orig, sizes = [orig_hw] * B, [(H, W)] * B
    orig_dev, sizes_dev = torch.tensor(orig, device=dev), torch.tensor(sizes, device=dev)
    post, segm = PostProcess(), PostProcessSegm(packed=True)
    step = harness.CapturedEvalStep(model, batch=B, max_orig_hw=orig_hw if masks else None, pad_hw=64)

    def eager_body(samples, tok):
        mc = model(samples, tok, encode_and_save=True)
        outputs = model(samples, tok, encode_and_save=False, memory_cache=mc)
        results = post(outputs, orig_dev)
        if masks:
            results = segm(results, outputs, orig_dev, sizes_dev)
        k.xdec_check()
        return results, outputs

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for samples, tok in batches:
            fn(samples, tok)
        torch.cuda.synchronize()
        return steps * B / (time.perf_counter() - t0)

    with torch.no_grad():
        for samples, tok in batches[:warmup]:
            eager_body(samples, tok)
            step.step(samples, tok, orig, sizes)
        eager, captured = [], []
        for _ in range(repeats):                       # alternated: the two paths share whatever else the host is doing
            eager.append(region(lambda s_, t_: eager_body(s_, t_)))
            captured.append(region(lambda s_, t_: step.step(s_, t_, orig, sizes)))
        # same results on the same batch (the captured step pads nothing here: 640 is a multiple of 64)
        want, outputs = eager_body(*batches[0])
        got = step.step(*batches[0], orig, sizes)
        same = all(torch.allclose(g["boxes"], w["boxes"], rtol=1e-5, atol=1e-3) and torch.allclose(g["scores"], w["scores"], rtol=1e-5, atol=1e-6) and
                   (not masks or torch.equal(g["mask_bits"], w["mask_bits"])) for g, w in zip(got, want))
        diff = {"max_score_diff": max(float((g["scores"] - w["scores"]).abs().max()) for g, w in zip(got, want)),
                "max_box_diff": max(float((g["boxes"] - w["boxes"]).abs().max()) for g, w in zip(got, want))}
        if masks:
            diff["mask_words_differing"] = sum(int((g["mask_bits"] != w["mask_bits"]).sum()) for g, w in zip(got, want))
            diff["mask_words"] = sum(g["mask_bits"].numel() for g in got)
        # the post-processing alone, on the outputs of one forward
        table = torch.tensor([list(s_) + list(o_) for s_, o_ in zip(sizes, orig)], dtype=torch.int64, device=dev)

        def torch_post():
            r = post(outputs, orig_dev)
            return segm(r, outputs, orig_dev, sizes_dev) if masks else r

        out_pp, bits = None, None
        if masks:
            cap_words = outputs["pred_logits"].shape[1] * orig_hw[1] * k.mask_words(orig_hw[0])
            bits = torch.empty(B * cap_words, dtype=torch.int64, device=dev)
            logits = outputs["pred_masks"].squeeze(2).float().contiguous()

        def kernel_post():
            nonlocal out_pp
            out_pp = k.postprocess(outputs["pred_logits"], outputs["pred_boxes"], orig_dev, None, out=out_pp)
            if masks:
                k.mask_resize_pack_batch(logits, (H, W), table, orig_hw, cap_words, bits)

        t_torch, t_kernel = timed(torch_post, iters=steps, warm=warmup), timed(kernel_post, iters=steps, warm=warmup)
    e, c = _median(eager), _median(captured)
    return {"batch": B, "image_hw": [H, W], "tokens": L, "orig_hw": list(orig_hw), "steps_per_region": steps, "repeats": repeats,
            "eager_images_per_s": e, "captured_images_per_s": c, "captured_over_eager": c / e, "eager_all": eager, "captured_all": captured,
            "captures": step.captures, "replays": step.replays, "xdec_in_graph": bool(next(iter(step._buckets.values()))["xdec"]),
            "results_equal_eager": bool(same), "difference_to_eager": diff, "postproc_torch_ms": t_torch, "postproc_kernels_ms": t_kernel,
            "postproc_torch_images_per_s": B / t_torch * 1e3, "postproc_kernels_images_per_s": B / t_kernel * 1e3}


def main():
    import argparse
    import os
    import subprocess
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--micro", action="store_true", help="the evaluation-path kernel microbenchmark instead")
    ap.add_argument("--masks", action="store_true", help="only the segmentation recipe (default: detection, then segmentation)")
    ap.add_argument("--steps", type=int, default=16, help="batches per timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", choices=["detection", "masks"], help=argparse.SUPPRESS)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds one recipe's child process may take")
    ap.add_argument("--out", default=os.path.join("profiles", "eval_captured.json"))
    a = ap.parse_args()
    if a.micro:
        return micro()
    def rnd(v):
        if isinstance(v, float):
            return round(v, 3) if abs(v) >= 1 else float(f"{v:.3g}")
        if isinstance(v, list):
            return [rnd(x) for x in v]
        if isinstance(v, dict):
            return {k_: rnd(x) for k_, x in v.items()}
        return v

    if a.leg:
        print("LEG " + json.dumps(rnd(leg(a.leg == "masks", a.steps, a.warmup, a.repeats))))
        return
    out = {"tool": "tools/bench_eval.py", "device": "MI355X"}
    for name in (["masks"] if a.masks else ["detection", "masks"]):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_eval: the {name} leg ran into its time limit; nothing more is started")
        line = next((ln for ln in done.stdout.splitlines() if ln.startswith("LEG ")), None)
        if done.returncode != 0 or line is None:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"bench_eval: the {name} leg failed (exit {done.returncode}); nothing more is started")
        out[name] = json.loads(line[4:])
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
