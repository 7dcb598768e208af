"""Shared-image training WITH THE MASK HEAD on one MI355X: P = 8 (image, caption) training samples per step from B images and T captions, against
the per-sample step on the expanded batch.  configs[2] settings: 640 x 640 images, 16-token captions, DETRsegm with the mask losses, 0..10 targets
per sample with their ground-truth masks, FusedClipAdamWEMA, a different batch every step -- everything trainable (5 aux layers) and the
reference's frozen-detector recipe (no aux layers; the mask head and bbox_attention train alone).  Legs, in ms per step:
  control_8[_frozen]        CapturedTrainStep(batch=8) with masks on harness.expand_pairs of the batch: the ResNet runs 8 times forward and backward
  shared_B_T[_frozen]       CapturedMaskPairTrainStep at (B, T) = (8, 8) identity, (2, 4), (1, 8), each with P = 8: all 800 maps live, B backbone passes
The (8, 8) identity leg runs the arithmetic of the control: its time against the control's is what the pair tables cost by themselves.
Every leg is warmed (its eager first step and the capture included) before any clock starts; a timed region is `--steps` steps on a host clock and
ends in a device synchronise; the legs alternate inside one process and a leg's figure is the median of its `--repeats` regions.  Both kinds of leg
pack their targets and ground-truth masks on the host inside the step.  Also measured: the two launches of the mask program's backward over pairs
alone (HIP events) at the step's shapes against their traffic floors at 8 TB/s, and the allocator peak of each leg (eager first step, capture
and the graph's pool) above what was allocated before the leg was built.
Prints ONE JSON line and writes it to profiles/pair_masks.json.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, spec
BF16 = torch.bfloat16


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _timed(fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def launches_alone(dev, B, P, Q, size, matched):
    """toist_sum_maps_by_image and toist_resize_add_rows_pairs at the shapes of the step's last stage (adapter3 / lay5: 160 x 160 at 640 x 640, 32
    channels in; `matched` maps carry a gradient), and the dense sum over all P * Q maps: mean of 50 back-to-back launches, against the bytes moved."""
    from toist_amd import kernels as k
    side, C = size // 4, 32
    per = side * side * C
    table = torch.tensor([p * B // P for p in range(P)], dtype=torch.int32, device=dev)
    rows = torch.sort(torch.randperm(P * Q, generator=torch.Generator().manual_seed(0))[:matched]).values.to(dev)
    seg = torch.tensor([int((rows < p * Q).sum()) for p in range(P + 1)], dtype=torch.int32, device=dev)
    out = {}
    g = torch.randn(matched, side, side, C, device=dev).to(BF16)
    sums = torch.empty(B, per, dtype=BF16, device=dev)
    ms = _timed(lambda: k.sum_maps_by_image(g, seg, table, Q, B, per, sums))
    traffic = (matched + B) * per * 2
    out["sum_maps_by_image_matched"] = {"maps": matched, "images": B, "per": per, "launch_ms": ms, "bytes": traffic, "traffic_floor_ms": traffic / HBM_PEAK * 1e3}
    dense = torch.randn(P * Q, side // 2, side // 2, C, device=dev).to(BF16)       # the dense backward at the stage below (80 x 80): 800 maps
    per2 = (side // 2) ** 2 * C
    sums2 = torch.empty(B, per2, dtype=BF16, device=dev)
    ms = _timed(lambda: k.sum_maps_by_image(dense, None, table, Q, B, per2, sums2))
    traffic = (P * Q + B) * per2 * 2
    out["sum_maps_by_image_dense"] = {"maps": P * Q, "images": B, "per": per2, "launch_ms": ms, "bytes": traffic, "traffic_floor_ms": traffic / HBM_PEAK * 1e3}
    x = torch.randn(matched, side // 2, side // 2, C, device=dev).to(BF16)
    fpn = torch.randn(B, side, side, C, device=dev).to(BF16)
    up = torch.empty(matched, side, side, C, dtype=BF16, device=dev)
    ms = _timed(lambda: k.resize_add_rows_pairs(x, fpn, rows, table, matched, Q, side // 2, side // 2, side, side, C, up))
    traffic = (matched * (side // 2) ** 2 * C + B * per + matched * per) * 2              # every image term read once (the rest from cache), every map written
    out["resize_add_rows_pairs"] = {"maps": matched, "images": B, "from": [side // 2, side // 2], "to": [side, side], "C": C, "launch_ms": ms, "bytes": traffic,
                                    "traffic_floor_ms": traffic / HBM_PEAK * 1e3}
    assert k.sweep_check(raise_on_failure=False) == 0
    for v in out.values():
        v["includes"] = "launch overhead of back-to-back launches on one stream; HIP events, not a kernel trace"
    return out


def run(a):
    import toist_amd
    from toist_amd import harness, kernels as k
    from toist_amd.optim import FusedClipAdamWEMA
    dev = torch.device("cuda:0")
    H = W = a.size
    L, P = 16, 8
    k.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    legs, peaks = {}, {}

    def recipe(frozen):
        args = harness.default_args(device="cuda", masks=True, mask_model="smallconv", frozen_weights="detector_checkpoint.pth" if frozen else None,
                                    aux_loss=not frozen)
        torch.manual_seed(0)
        model, criterion, _, weight_dict = toist_amd.build_model(args)
        model.to(dev).train()
        criterion.train()
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        groups = [g for g in ({"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
                              {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
                              {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}) if g["params"]]
        src = [v for v in model.state_dict().values() if v.is_floating_point()]
        opt = FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm,
                                ema=list(zip(src, [v.detach().clone() for v in src])), ema_decay=0.9998)
        return model, criterion, weight_dict, opt

    def pair_pool(B, T):
        return [harness.synthetic_pair_batch(B, T, P, height=H, width=W, tokens=L, seed=1000 + 7919 * i, max_targets=10, device=dev, with_masks=True)
                for i in range(a.steps)]

    def on_host(batch):            # targets, masks and the positive map stay on the host, as a loader delivers them; images and tokens are on the device
        s, tok, pi, pc, targets, pmap = batch
        return s, tok, pi, pc, [{k_: (v.cpu() if torch.is_tensor(v) else v) for k_, v in t.items()} for t in targets], pmap.cpu()

    def build(name, make, pool, call):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        step = make()
        for i in range(max(a.warmup, 2)):          # the eager first step + the capture, then a replay
            call(step, pool[i % len(pool)])
        torch.cuda.synchronize()
        peaks[name] = {"peak_above_start_GiB": (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30,
                       "kept_after_warmup_GiB": (torch.cuda.memory_allocated(dev) - base) / 2 ** 30}
        legs[name] = (step, pool, call)
        sys.stderr.write(f"bench_pair_masks: built {name}\n")
        sys.stderr.flush()

    for frozen in (False, True):
        model, criterion, weight_dict, opt = recipe(frozen)
        tag = "_frozen" if frozen else ""
        pool = [on_host(b) for b in pair_pool(P, P)]               # P images, P captions, identity pairs: the expanded batch itself
        expanded = [harness.expand_pairs(*b) for b in pool]
        build("control_8" + tag, lambda: harness.CapturedTrainStep(model, criterion, opt, weight_dict, batch=P, max_targets_per_image=10, pad_hw=64),
              expanded, lambda step, b: step.step(b[0], b[1], b[2], b[3]))
        for B, T in ((8, 8), (2, 4), (1, 8)):
            pool = [on_host(b) for b in pair_pool(B, T)]
            build(f"shared_{B}_{T}" + tag, lambda B=B, T=T: harness.CapturedMaskPairTrainStep(model, criterion, opt, weight_dict, batch=B, captions=T, pairs=P,
                                                                                             max_targets_per_image=10, pad_hw=64),
                  pool, lambda step, b: step.step(*b))

    def region(name):
        step, pool, call = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in pool:
            last = call(step, b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(pool), float(last.detach())

    times, final = {name: [] for name in legs}, {}
    for _ in range(a.repeats):                     # alternated: the legs share whatever else the host is doing
        for name in legs:
            dt, final[name] = region(name)
            times[name].append(dt)
            sys.stderr.write(f"bench_pair_masks: {name} {1e3 * dt:.3f} ms/step\n")
            sys.stderr.flush()
    assert k.sweep_check(raise_on_failure=False) == 0
    ms = {name: 1e3 * _median(v) for name, v in times.items()}
    control_of = lambda name: "control_8_frozen" if name.endswith("_frozen") else "control_8"
    return {"tool": "tools/bench_pair_masks.py", "device": "MI355X",
            "workload": {"image_hw": [H, W], "tokens": L, "queries": 100, "pairs": P,
                         "recipe": "configs[2]: detection + mask losses, 5 aux layers, dropout 0.1; _frozen: the frozen-detector recipe, no aux layers",
                         "optimizer": "FusedClipAdamWEMA", "steps_per_region": a.steps, "repeats": a.repeats, "a_different_batch_every_step": True,
                         "targets": "0..10 per pair with their masks at 640 x 640, packed on the host inside the step (both kinds of leg)"},
            "ms_per_step": ms, "samples_per_s": {name: P / (v * 1e-3) for name, v in ms.items()},
            "ms_per_step_all": {name: [1e3 * x for x in v] for name, v in times.items()},
            "over_control": {name: ms[control_of(name)] / v for name, v in ms.items() if name.startswith("shared")},
            "final_loss": final, "allocator": peaks,
            "captures": {name: legs[name][0].captures for name in legs}, "replays": {name: legs[name][0].replays for name in legs},
            "xdec_failed": bool(k.XDEC_FAILED),
            "launches_alone": {"B2_P8": launches_alone(dev, 2, P, 100, a.size, 40), "B1_P8": launches_alone(dev, 1, P, 100, a.size, 40)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "pair_masks.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_masks: no GPU; nothing is measured without one")

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
