"""Task-sweep inference WITH THE MASK HEAD on one MI355X: T = 14 captions over batches of B = 8 synthetic 640 x 640 images (P = 112 (image, caption)
pairs per image batch, 16-token captions, DETRsegm with Q = 100 queries, masks packed for 480 x 640 originals), in ms per image batch and pairs/s:
  control         what a user does without the sweep: 14 CapturedEvalStep(masks) replays per image batch (one per caption: the ResNet, the adapters and
                  the per-image convolutions of the mask head run 14 times), the results of every replay copied out of the bucket's buffers
  sweep_ppp_N     CapturedMaskSweepStep(batch=8, captions=14, pairs_per_pass=N), N in --passes (4, 8, 16): one upload + one graph launch + the
                  status reads per image batch
Same weights, same images, same captions.  Every leg is warmed (its eager first pass and its capture included) before any clock starts; a timed
region is `--steps` image batches (a different batch every step) on a host clock and ends in a device synchronise; the legs alternate inside one
process and the figure of a leg is the median of its `--repeats` regions.  Also reported per leg: the peak of allocated bytes while it was built and
warmed, and the bytes the caching allocator reserved for it (the bucket's buffers + its graph pool).  How far the sweep's scores, boxes and mask bits
are from the control's is measured on one batch after the timings.
Prints ONE JSON line and writes it to profiles/mask_sweep.json; --parity FILE merges the oracle errors the test suite wrote out
(mask_sweep_model_parity.json of tests/test_gpu_zz_zzzz_mask_sweep_model.py) into it.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run(a):
    import toist_amd
    from toist_amd import harness, kernels as k
    from toist_amd.transformer import TokenizedText
    dev = torch.device("cuda:0")
    B, T, H, W, L = a.batch, a.captions, a.size, a.size, 16
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cuda", masks=True, mask_model="smallconv"))[0].to(dev).eval()
    Q = model.detr.query_embed.weight.shape[0]
    _, captions, _, _ = harness.synthetic_batch(T, 32, 32, tokens=L, seed=77, device=dev, max_targets=0)
    per_caption = [TokenizedText({"input_ids": captions["input_ids"][t:t + 1].expand(B, L).contiguous(),
                                  "attention_mask": captions["attention_mask"][t:t + 1].expand(B, L).contiguous()}) for t in range(T)]
    batches = [harness.synthetic_batch(B, H, W, tokens=L, seed=900 + i, device=dev, max_targets=0)[0] for i in range(a.steps)]
    orig, crop, cap_hw = [(480, 640)] * B, [(H, W)] * B, (480, 640)

    def built(make, first):
        """make() a step and run first(step) -- its eager pass and its capture -- -> (step, peak allocated bytes meanwhile, bytes reserved for it)"""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base_alloc, base_res = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
        step = make()
        with torch.no_grad():
            for _ in range(a.warmup):
                first(step)
        torch.cuda.synchronize()
        return step, {"peak_allocated_bytes": torch.cuda.max_memory_allocated(), "allocated_before_bytes": base_alloc,
                      "reserved_for_the_leg_bytes": torch.cuda.memory_reserved() - base_res, "allocated_held_bytes": torch.cuda.memory_allocated() - base_alloc}

    def control_batch(step, samples):
        kept = []
        for t in range(T):
            r = step.step(samples, per_caption[t], orig, crop)
            kept.append((torch.stack([x["scores"] for x in r]), torch.stack([x["boxes"] for x in r]),
                         torch.stack([x["mask_bits"] for x in r])))             # the next replay overwrites the bucket's buffers
        return kept

    legs, memory = {}, {}
    ctl, memory["control"] = built(lambda: harness.CapturedEvalStep(model, batch=B, masks=True, max_orig_hw=cap_hw, pad_hw=64), lambda s: control_batch(s, batches[0]))
    legs["control"] = lambda samples: control_batch(ctl, samples)
    sweeps = {}
    for n in a.passes:
        name = f"sweep_ppp_{n}"
        sweeps[n], memory[name] = built(lambda n=n: harness.CapturedMaskSweepStep(model, batch=B, captions=T, max_orig_hw=cap_hw, pairs_per_pass=n, pad_hw=64),
                                        lambda s: s.step(batches[0], captions, orig, crop))
        legs[name] = lambda samples, n=n: sweeps[n].step(samples, captions, orig, crop)

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in batches:
            fn(s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(batches) * 1e3

    ms = {name: [] for name in legs}
    with torch.no_grad():
        for _ in range(a.repeats):                                # alternated: the legs share whatever else the host is doing
            for name, fn in legs.items():
                ms[name].append(region(fn))
                sys.stderr.write(f"bench_mask_sweep: {name} {ms[name][-1]:.2f} ms per image batch\n")
                sys.stderr.flush()
        # the same answers: per (image, task), the sweep against the control on one batch
        want = control_batch(ctl, batches[0])
        diff = {}
        for n, step in sweeps.items():
            res, pi, pc, live = step.step(batches[0], captions, orig, crop)
            d = {"scores": 0.0, "boxes": 0.0, "mask_bits_differing_fraction": 0.0}
            for p in range(live):
                i, t = int(pi[p]), int(pc[p])
                d["scores"] = max(d["scores"], float((res[p]["scores"] - want[t][0][i]).abs().max()))
                d["boxes"] = max(d["boxes"], float((res[p]["boxes"] - want[t][1][i]).abs().max()))
                x = res[p]["mask_bits"] ^ want[t][2][i]
                flipped = sum(int(((x >> s) & 1).sum()) for s in range(64))
                d["mask_bits_differing_fraction"] = max(d["mask_bits_differing_fraction"], flipped / (Q * cap_hw[0] * cap_hw[1]))
            diff[f"sweep_ppp_{n}"] = d
    med = {name: _median(v) for name, v in ms.items()}
    return {"tool": "tools/bench_mask_sweep.py", "device": "MI355X",
            "workload": {"images_per_batch": B, "captions": T, "pairs_per_image_batch": B * T, "image_hw": [H, W], "tokens": L, "queries": Q,
                         "original_hw": list(cap_hw), "image_batches_per_region": a.steps, "repeats": a.repeats, "warmup_passes": a.warmup},
            "ms_per_image_batch": med, "ms_per_image_batch_all": ms, "pairs_per_s": {name: B * T / v * 1e3 for name, v in med.items()},
            "sweep_over_control": {name: med["control"] / v for name, v in med.items() if name != "control"},
            "memory": memory, "plane_buffer_bytes": {"control": B * ctl.capacity_words * 8, "sweep": B * T * next(iter(sweeps.values())).capacity_words * 8},
            "memory_note": "peak_allocated_bytes includes what was allocated before the leg (the model, the inputs, earlier legs: allocated_before_bytes); "
                           "reserved_for_the_leg_bytes is the caching allocator's growth over the leg's eager pass and capture: its buffers and graph pool",
            "xdec_in_graph": {"control": bool(next(iter(ctl._buckets.values()))["xdec"]),
                              **{f"sweep_ppp_{n}": bool(next(iter(s._buckets.values()))["xdec"]) for n, s in sweeps.items()}},
            "xdec_failed": bool(k.XDEC_FAILED), "captures": {"control": ctl.captures, **{f"sweep_ppp_{n}": s.captures for n, s in sweeps.items()}},
            "max_difference_to_control": diff,
            "difference_units": "scores: probability; boxes: pixels of the 480 x 640 originals; mask bits: the largest fraction of a pair's Q planes that differs"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--captions", type=int, default=14)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=10, help="image batches per timed region")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, nargs="+", default=[4, 8, 16], help="pairs_per_pass values of the sweep legs")
    ap.add_argument("--parity", default=None, help="mask_sweep_model_parity.json as the test suite wrote it: merged into the output")
    ap.add_argument("--out", default=os.path.join("profiles", "mask_sweep.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_sweep: no GPU; nothing is measured without one")

    def rnd(v):
        if isinstance(v, float):
            return round(v, 3) if abs(v) >= 1 else float(f"{v:.3g}")
        if isinstance(v, list):
            return [rnd(x) for x in v]
        if isinstance(v, dict):
            return {k_: rnd(x) for k_, x in v.items()}
        return v

    out = rnd(run(a))
    if a.parity and os.path.exists(a.parity):
        with open(a.parity) as f:
            out["oracle_parity"] = json.load(f)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
