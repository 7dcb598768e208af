"""Shared-image training on one MI355X: P (image, caption) training samples per step from B images and T captions, against the per-sample step on
the expanded batch.  configs[1] settings: 640 x 640 images, 16-token captions, the default detection recipe with loss_contrastive_align,
FusedClipAdamWEMA, a different batch every step.  Legs, in (image, caption) pairs per second and ms per step:
  control_8            CapturedTrainStep(batch=8) on harness.expand_pairs of the batch: the per-sample path (ResNet and RoBERTa run 8 times)
  shared_B_T           CapturedPairTrainStep at (B, T) = (8, 8) identity, (4, 2), (2, 4), (1, 8), each with P = 8
  control_16 / shared_2_8_16   the larger step: (B, T, P) = (2, 8, 16) against CapturedTrainStep(batch=16)
The (8, 8) identity leg runs the arithmetic of the control: its time against the control's is what the new path costs by itself.
Every leg is warmed (its eager first step and the capture included) before any clock starts; a timed region is `--steps` steps on a host clock and
ends in a device synchronise; the legs alternate inside one process and a leg's figure is the median of its `--repeats` regions.  Both kinds of leg
pack their targets on the host inside the step.  Also measured: the toist_sweep_assemble_bwd launch alone (HIP events) against its traffic floor
(P*S + B*HW + T*L) * D * 2 bytes at 8 TB/s, and the allocator peak of each leg (eager first step, capture and the graph's pool), above what was
allocated before the leg was built.
Prints ONE JSON line and writes it to profiles/pair_train.json; --parity FILE merges the gradient-parity figures the test suite wrote out
(pair_train_grad_parity.json of tests/test_gpu_zz_pair_train.py) into it.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, spec


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def assemble_bwd_alone(dev, B, T, P, HW, L, D, iters=50):
    """The backward launch at the workload's shape: the mean of `iters` launches between two HIP events, against the bytes it must move."""
    from toist_amd import kernels as k
    g = torch.Generator().manual_seed(0)
    d_seq = torch.randn(P, HW + L, D, generator=g).to(torch.bfloat16).to(dev)
    pi = torch.tensor([p * B // P for p in range(P)], dtype=torch.int32, device=dev)
    pc = torch.tensor([p % T for p in range(P)], dtype=torch.int32, device=dev)
    out = k.sweep_assemble_bwd(d_seq, pi, pc, B, HW, T, L)
    for _ in range(5):
        k.sweep_assemble_bwd(d_seq, pi, pc, B, HW, T, L, out=out)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        k.sweep_assemble_bwd(d_seq, pi, pc, B, HW, T, L, out=out)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / iters
    traffic = (P * (HW + L) + B * HW + T * L) * D * 2
    return {"shape": {"B": B, "T": T, "P": P, "HW": HW, "L": L, "D": D}, "launch_ms": ms, "bytes": traffic, "traffic_floor_ms": traffic / HBM_PEAK * 1e3,
            "includes": "launch overhead of back-to-back launches on one stream; HIP events, not a kernel trace"}


def run(a):
    import toist_amd
    from toist_amd import harness, kernels as k
    from toist_amd.optim import FusedClipAdamWEMA
    dev = torch.device("cuda:0")
    H = W = a.size
    L = 16
    args = harness.default_args(device="cuda", contrastive_align_loss=True)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    criterion.train()
    k.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
              {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
              {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}]
    src = [v for v in model.state_dict().values() if v.is_floating_point()]
    opt = FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm,
                            ema=list(zip(src, [v.detach().clone() for v in src])), ema_decay=0.9998)

    def pair_pool(B, T, P):
        return [harness.synthetic_pair_batch(B, T, P, height=H, width=W, tokens=L, seed=1000 + 7919 * i, max_targets=10, device=dev) for i in range(a.steps)]

    def on_host(batch):            # the targets and the positive map stay on the host, as a loader delivers them; images and tokens are on the device
        s, tok, pi, pc, targets, pmap = batch
        return s, tok, pi, pc, [{k_: (v.cpu() if torch.is_tensor(v) else v) for k_, v in t.items()} for t in targets], pmap.cpu()

    legs, peaks = {}, {}

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

    def control(P):
        pool = [on_host(b) for b in pair_pool(P, P, P)]            # P images, P captions, identity pairs: the expanded batch itself
        expanded = [harness.expand_pairs(*b) for b in pool]
        build(f"control_{P}", lambda: harness.CapturedTrainStep(model, criterion, opt, weight_dict, batch=P, max_targets_per_image=10, pad_hw=64),
              expanded, lambda step, b: step.step(b[0], b[1], b[2], b[3]))

    def shared(B, T, P, name):
        pool = [on_host(b) for b in pair_pool(B, T, P)]
        build(name, lambda: harness.CapturedPairTrainStep(model, criterion, opt, weight_dict, batch=B, captions=T, pairs=P, max_targets_per_image=10,
                                                          pad_hw=64), pool, lambda step, b: step.step(*b))

    control(8)
    for B, T in ((8, 8), (4, 2), (2, 4), (1, 8)):
        shared(B, T, 8, f"shared_{B}_{T}")
    control(16)
    shared(2, 8, 16, "shared_2_8_16")

    def region(name):
        step, pool, call = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in pool:
            last = call(step, b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(pool), float(last)

    times, final = {name: [] for name in legs}, {}
    for _ in range(a.repeats):                     # alternated: the legs share whatever else the host is doing
        for name in legs:
            dt, final[name] = region(name)
            times[name].append(dt)
            sys.stderr.write(f"bench_pair_train: {name} {1e3 * dt:.3f} ms/step\n")
            sys.stderr.flush()
    pairs_of = lambda name: 16 if name.endswith("16") else 8
    ms = {name: 1e3 * _median(v) for name, v in times.items()}
    HW = (H // 32) * (W // 32)
    return {"tool": "tools/bench_pair_train.py", "device": "MI355X",
            "workload": {"image_hw": [H, W], "tokens": L, "queries": 100, "recipe": "detection + loss_contrastive_align, 5 aux layers, dropout 0.1",
                         "optimizer": "FusedClipAdamWEMA", "steps_per_region": a.steps, "repeats": a.repeats, "a_different_batch_every_step": True,
                         "targets": "0..10 per pair, packed on the host inside the step (both kinds of leg)"},
            "ms_per_step": ms, "pairs_per_s": {name: pairs_of(name) / (v * 1e-3) for name, v in ms.items()},
            "ms_per_step_all": {name: [1e3 * x for x in v] for name, v in times.items()},
            "over_control": {name: ms["control_16" if name.endswith("16") else "control_8"] / v for name, v in ms.items() if name.startswith("shared")},
            "final_loss": final, "allocator": peaks,
            "captures": {name: legs[name][0].captures for name in legs}, "replays": {name: legs[name][0].replays for name in legs},
            "xdec_failed": bool(k.XDEC_FAILED),
            "assemble_bwd": [assemble_bwd_alone(dev, 2, 4, 8, HW, L, 256), assemble_bwd_alone(dev, 2, 8, 16, HW, L, 256)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parity", default=None, help="pair_train_grad_parity.json as the test suite wrote it: its worst cases are merged into the output")
    ap.add_argument("--out", default=os.path.join("profiles", "pair_train.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_train: no GPU; nothing is measured without one")

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
            parity = json.load(f)
        out["gradient_parity"] = {"source": "tests/test_gpu_zz_pair_train.py::test_shared_pairs_against_the_oracle_and_the_expanded_batch",
                                  "pairs": parity.get("pairs"), "total": parity.get("total"), "worst": parity.get("worst")}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
