#!/usr/bin/env python
"""The distillation step (configs[4], batch 4 pairs) on a stream a real loader could deliver: the batches cycle through the three image sizes of
`bench.py --mixed-sizes` (read from bench.py) and the noun and the pronoun caption have different token counts that change from batch to batch.

  (a) list       harness.distillation_step on the collate batch (the list-of-dicts step): all that could run on such a stream before the buckets
  (b) bucketed   harness.CapturedDistillStep without image_hw / tokens: one hipGraph per bucket (Hp, Wp, Lp), timed after every bucket is captured
  (c) fixed      for context: harness.CapturedDistillStep(image_hw=(640, 640), tokens=16) on 640 x 640 batches of 16-token captions

(a) and (b) run the same stream on the same models, alternated region by region in one process; every figure is the median of --repeats regions of
--steps steps (host clock around a region that ends in a device synchronise), with the smallest and the largest region beside it.  Also recorded: the
buckets used, captures and replays, the device memory each bucket took (torch's allocated / reserved bytes around its first step: static inputs,
target and caption tables, the graph's private pool) and what a first step costs (the eager pass plus the capture).
Writes profiles/distill_buckets.json (--out) and prints it.

    python tools/bench_distill_buckets.py --steps 12 --repeats 5
"""
import argparse
import ast
import copy
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (noun tokens, pronoun tokens) of the six batches of the pool; pad_tokens = 8 makes Lp = 16 of all but the fourth (24): with the three image sizes,
# four buckets -- the default max_graphs
CAPTIONS = ((16, 13), (12, 15), (14, 11), (20, 17), (10, 12), (13, 16))


def mixed_sizes():
    """The image sizes `bench.py --mixed-sizes` alternates, read from its source."""
    with open(os.path.join(ROOT, "bench.py")) as f:
        m = re.search(r"^\s*sizes = (\(\(.*\)\))\s*$", f.read(), flags=re.M)
    if m is None:
        raise SystemExit("bench.py: the sizes of --mixed-sizes were not found")
    return [tuple(int(v) for v in hw) for hw in ast.literal_eval(m.group(1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12, help="steps of one timed region (two passes over the pool)")
    ap.add_argument("--repeats", type=int, default=5, help="timed regions per leg")
    ap.add_argument("--warmup", type=int, default=6, help="steps of every leg before its first timed region")
    ap.add_argument("--no-contrastive", action="store_true", help="leave loss_contrastive_align out (bench.py --distill runs without it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_buckets.json"))
    a = ap.parse_args()

    import torch
    import toist_amd
    from toist_amd import engine, harness, kernels
    from toist_amd.matcher import check_lsap_pending
    from toist_amd.optim import FusedClipAdamWEMA
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill_buckets needs the GPU")
    dev = torch.device("cuda:0")
    sizes = mixed_sizes()
    args = harness.default_args(device="cuda", distillation=True, cluster=True, nsthl2_loss=True, softkd_loss=True, train_batch_size=a.batch,
                                contrastive_align_loss=not a.no_contrastive)
    torch.manual_seed(0)
    model, criterion, cc0, weight_dict = toist_amd.build_model(args)
    model_noun, _, _, _ = toist_amd.build_model(args)
    for m in (model, model_noun):
        m.to(dev).train()
    cc0.to(dev)
    cc0.full_label.fill_(1)                     # steady state, as bench.py --distill: banks full, k-means from the stored centres
    cc0.sync_host_state()
    engine.REUSE_GRAD_BUFFERS = True
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)

    def tail(m):
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        groups = [{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
                  {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
                  {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}]
        return FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm)

    opts = [tail(model), tail(model_noun)]

    def make_batch(j, hw, tokens):
        b_j = harness.synthetic_distill_batch(a.batch, *hw, tokens=tokens[0], tokens_pronoun=tokens[1], seed=2000 + 7919 * j, device=dev)
        for side_t in b_j["targets"]:
            for i, t in enumerate(side_t):
                t["dataset_name"] = f"task_{1 + (i * (j + 1) + 3 * j) % 14}_train.json"
        return b_j

    pool = [make_batch(j, sizes[j % len(sizes)], CAPTIONS[j]) for j in range(len(CAPTIONS))]
    fixed_pool = [make_batch(10 + j, (640, 640), (16, 16)) for j in range(4)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.set_stream(side)

    def region(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            out = fn(i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loss = float(out.detach())
        if loss != loss:
            raise SystemExit("bench_distill_buckets: a non-finite loss")
        return a.batch * n / dt

    def summary(rates):
        return {"pairs_per_s": round(statistics.median(rates), 2), "min": round(min(rates), 2), "max": round(max(rates), 2),
                "ms_per_step": round(1e3 * a.batch / statistics.median(rates), 3), "regions": [round(r, 2) for r in rates]}

    # ---- (a) the list-of-dicts step
    cc_list = copy.deepcopy(cc0)
    cc_list.sync_host_state()

    def list_step(i):
        kernels.SEED_DEV.add_(1000003)
        for o in opts:
            o.zero_grad(set_to_none=True)
        total, _ = harness.distillation_step(model, model_noun, criterion, cc_list, weight_dict, pool[i % len(pool)])
        total.backward()
        for o in opts:
            o.step()
        return total

    region(list_step, a.warmup)

    # ---- (b) the bucketed captured step: first steps (eager + capture) one by one, with the memory each bucket takes
    cc_cap = copy.deepcopy(cc0)
    cc_cap.sync_host_state()
    cap = harness.CapturedDistillStep(model, model_noun, criterion, cc_cap, opts, weight_dict, batch=a.batch, max_targets_per_image=10, stream=side)
    packed = [cap.pack(b) for b in pool]
    first = {}
    for pk in packed:
        key = pk[0]["key"]
        if key in first:
            continue
        torch.cuda.synchronize()
        alloc0, res0, t0 = torch.cuda.memory_allocated(), torch.cuda.memory_reserved(), time.perf_counter()
        cap.step(packed=pk)
        torch.cuda.synchronize()
        first[key] = {"first_step_ms": round(1e3 * (time.perf_counter() - t0), 1), "allocated_MiB": round((torch.cuda.memory_allocated() - alloc0) / 2 ** 20, 1),
                      "reserved_MiB": round((torch.cuda.memory_reserved() - res0) / 2 ** 20, 1)}
    captures_after_first_pass = cap.captures

    def cap_step(i):
        return cap.step(packed=packed[i % len(packed)])

    region(cap_step, a.warmup)
    listed, bucketed = [], []
    for _ in range(a.repeats):                  # alternated: both legs see the same neighbours on the machine
        listed.append(region(list_step, a.steps))
        bucketed.append(region(cap_step, a.steps))
    check_lsap_pending()
    kernels.xdec_check()
    assert cap.captures == captures_after_first_pass == len(first), (cap.captures, captures_after_first_pass, len(first))

    # ---- (c) the fixed-shape captured step, for context
    cc_fix = copy.deepcopy(cc0)
    cc_fix.sync_host_state()
    fix = harness.CapturedDistillStep(model, model_noun, criterion, cc_fix, opts, weight_dict, batch=a.batch, image_hw=(640, 640), tokens=16,
                                      max_targets_per_image=10, stream=side)
    fixed_packed = [fix.pack(b) for b in fixed_pool]

    def fix_step(i):
        return fix.step(packed=fixed_packed[i % len(fixed_packed)])

    region(fix_step, a.warmup)
    fixed = [region(fix_step, a.steps) for _ in range(a.repeats)]
    check_lsap_pending()
    kernels.xdec_check()

    pixels = [hw[0] * hw[1] for hw in sizes]
    padded = [k_[0] * k_[1] for pk in packed for k_ in [pk[0]["key"]]]
    real = [b["samples"][0].tensors.shape[-2] * b["samples"][0].tensors.shape[-1] for b in pool]
    med = lambda v: statistics.median(v)
    out = {"tool": "bench_distill_buckets", "device": torch.cuda.get_device_name(0), "batch_pairs": a.batch, "steps_per_region": a.steps, "regions": a.repeats,
           "warmup_steps": a.warmup, "contrastive_align_loss": not a.no_contrastive,
           "stream": {"image_sizes_from_bench_py": sizes, "captions_noun_pronoun_tokens": list(CAPTIONS), "pad_hw": cap.pad_hw, "pad_tokens": cap.pad_tokens,
                      "buckets_per_batch": [list(pk[0]["key"]) for pk in packed], "padded_over_real_pixels": round(sum(padded) / sum(real), 4),
                      "pixels_over_640x640": round(sum(pixels) / len(pixels) / (640 * 640), 4)},
           "a_list_of_dicts_step": summary(listed), "b_bucketed_captured_step": summary(bucketed), "c_fixed_shape_captured_step_640x640": summary(fixed),
           "b_over_a": round(med(bucketed) / med(listed), 3), "b_over_c": round(med(bucketed) / med(fixed), 3),
           "bucketed": {"buckets": len(first), "max_graphs": cap.max_graphs, "captures": cap.captures, "replays": cap.replays,
                        "per_bucket": {"x".join(str(v) for v in k_): v for k_, v in first.items()},
                        "note": "around each bucket's first step: allocated = the tensors the bucket keeps (static inputs, target and caption tables, outputs); reserved = "
                                "what the caching allocator took from the device for it, mostly the graph's private pool of activations.  The first bucket's figures "
                                "also hold what the captured path allocates once for all buckets (constant index tables, scratch of its stream), and its pool found "
                                "blocks the list step's warm-up had left in the allocator's cache"}}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
