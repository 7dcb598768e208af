"""The prototype choice inside the captured task sweep on one MI355X: T = 14 pronoun captions ('something') over batches of B = 8 synthetic
640 x 640 images (P = 112 (image, caption) pairs per batch, 16-token captions, detection model with cluster=True, 14 memory banks of 1024 rows,
all full), in (image, task) pairs per second:
  a  eager_loop_with_choice    what served the distilled model before: harness.evaluate_sweep's eager loop with the ClusterCriterion
                               (ClusterCriterion.infer_choice per pair stage: fp32 memory, clone, torch.where, decode from the fp32 copy)
  b  captured_with_choice      CapturedSweepStep(model, criterion): the toist_sweep_prototypes launch inside the graph, decode from bf16 memory_mod
  c  captured_without_choice   CapturedSweepStep(model) on the same model with args.cluster off, as context: what the stage adds to a replay
  d  the toist_sweep_prototypes launch alone at the workload's shape, in microseconds (HIP events around back-to-back launches; the centres
     persist from launch to launch, as they do from replay to replay, so a pair costs one Lloyd iteration -- the first launch, from the stored
     centres, is timed by itself)
Every leg is warmed on every shape it uses; a timed region is `--steps` image batches (a different batch every step) on a host clock and ends in a
device synchronise; the legs alternate inside one process and the figure of a leg is the median of its `--repeats` regions.  Each leg has its own
copy of the criterion (every step moves the centres).  Prints ONE JSON line and writes it to profiles/sweep_choice.json."""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _blob_banks(cc, seed=0):
    """banks of three well separated blobs per task (noun features cluster; k-means on white noise would measure nothing of interest), centres near
    the blob means, every bank marked full"""
    g = torch.Generator().manual_seed(seed)
    T, N, D, K = cc.task_count, cc.memory_size, cc.feature_dim, cc.cluster_num
    means = torch.randn(T, K, D, generator=g) * 2.0
    cc.feature_bank.copy_(means[:, torch.arange(N) % K, :] + 0.25 * torch.randn(T, N, D, generator=g))
    cc.cluster_centers.copy_(means + 0.5 * torch.randn(T, K, D, generator=g))
    cc.full_label.fill_(1)
    cc.update_count.fill_(N + 1)
    cc.sync_host_state()


def launch_alone(dev, cc, P, T, HW, L, iters=50):
    """toist_sweep_prototypes at the workload's shape on synthetic rows: the first launch from the stored centres, then the mean of `iters` launches"""
    from toist_amd import kernels as k
    from toist_amd.distill import SweepChoiceTables
    from toist_amd.harness import SyntheticCaptions
    g = torch.Generator().manual_seed(1)
    D = cc.feature_dim
    memory = torch.randn(P, HW + L, D, generator=g).to(torch.bfloat16).to(dev)
    mod = memory.clone()
    ids = torch.zeros(T, L, dtype=torch.int64)
    tables = SweepChoiceTables(T, L, dev)
    tables.load(SyntheticCaptions({"input_ids": ids, "attention_mask": torch.ones_like(ids)}), [f"use something for task {t}" for t in range(T)],
                [f"task_{t + 1}_train.json" for t in range(T)], P)
    pc = (torch.arange(P, dtype=torch.int32) % T).to(dev)
    banks, centers = cc.feature_bank.clone(), cc.cluster_centers.clone()
    iters_out = torch.zeros(P, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    k.sweep_prototypes(memory, mod, pc, tables, banks, centers, HW, iters=iters_out)
    b.record()
    torch.cuda.synchronize()
    first_us, first_iters = a.elapsed_time(b) * 1e3, iters_out.tolist()
    for _ in range(5):
        k.sweep_prototypes(memory, mod, pc, tables, banks, centers, HW, iters=iters_out)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        k.sweep_prototypes(memory, mod, pc, tables, banks, centers, HW, iters=iters_out)
    b.record()
    torch.cuda.synchronize()
    k.sweep_check()
    return {"shape": {"P": P, "T": T, "HW": HW, "L": L, "D": D, "K": cc.cluster_num, "N": cc.memory_size, "workgroups": T},
            "launch_us": a.elapsed_time(b) * 1e3 / iters, "lloyd_iterations_per_pair": sorted(set(iters_out.tolist())),
            "first_launch_us": first_us, "first_launch_lloyd_iterations": [min(first_iters), max(first_iters)],
            "includes": "launch overhead of back-to-back launches on one stream; HIP events, not a kernel trace"}


def run(a):
    import toist_amd
    from toist_amd import harness, kernels as k
    from toist_amd.postprocessors import PostProcess
    dev = torch.device("cuda:0")
    B, T, H, W, L = a.batch, a.captions, a.size, a.size, 16
    torch.manual_seed(0)
    model, _, cc, _ = toist_amd.build_model(harness.default_args(device="cuda", distillation=True, cluster=True, cluster_memory_size=a.bank))
    model.to(dev).eval()
    if T > cc.task_count:
        raise SystemExit(f"bench_sweep_choice: {T} captions for a criterion of {cc.task_count} tasks")
    cc.to(dev)
    _blob_banks(cc)
    cc_a, cc_b = copy.deepcopy(cc), copy.deepcopy(cc)
    for c in (cc_a, cc_b):
        c.sync_host_state()
    post = PostProcess()
    _, tok, _, _ = harness.synthetic_batch(T, 32, 32, tokens=L, seed=77, max_targets=0)
    tok["attention_mask"][:] = 1
    captions = harness.SyntheticCaptions(dict(tok)).to(dev)
    strings = [f"use something for task {t}" for t in range(T)]          # 'something' = tokens 2 .. 4
    names = [f"task_{t + 1}_train.json" for t in range(T)]
    tasks = [(f"task_{t + 1}", strings[t], names[t]) for t in range(T)]
    batches = [harness.synthetic_batch(B, H, W, tokens=L, seed=900 + i, device=dev, max_targets=0)[0] for i in range(a.steps)]
    orig = [(480, 640)] * B
    as_batch = lambda s: {"samples": s, "image_ids": list(range(B)), "orig_sizes": orig}
    step_b = harness.CapturedSweepStep(model, cc_b, batch=B, captions=T, pad_hw=64)
    step_c = harness.CapturedSweepStep(model, batch=B, captions=T, pad_hw=64)

    def leg_a(samples_list):
        return harness.evaluate_sweep(model, post, [as_batch(s) for s in samples_list], tasks, dev, cluster_criterion=cc_a, tokenized=captions)

    def leg_b(samples):
        return step_b.step(samples, captions, orig, dataset_names=names, captions=strings)

    def leg_c(samples):
        model.args.cluster = False                                 # decode reads it when the bucket's first batch runs and is captured; a replay does not
        try:
            return step_c.step(samples, captions, orig)
        finally:
            model.args.cluster = True

    def region(fn, whole):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if whole:
            fn(batches)
        else:
            for s in batches:
                fn(s)
        torch.cuda.synchronize()
        return len(batches) * B * T / (time.perf_counter() - t0)

    legs = {"a_eager_loop_with_choice": (leg_a, True), "b_captured_with_choice": (leg_b, False), "c_captured_without_choice": (leg_c, False)}
    rates = {name: [] for name in legs}
    with torch.no_grad():
        for name, (fn, whole) in legs.items():
            for _ in range(a.warmup):
                fn(batches[:1]) if whole else fn(batches[0])
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for name, (fn, whole) in legs.items():
                rates[name].append(region(fn, whole))
                sys.stderr.write(f"bench_sweep_choice: {name} {rates[name][-1]:.1f} pairs/s\n")
                sys.stderr.flush()
        # the same answers: (a) and (b) from one state of the centres on one batch
        cc_b.cluster_centers.copy_(cc_a.cluster_centers)
        want = leg_a(batches[:1])
        res, pi, pc, live = leg_b(batches[0])
        diff = {"scores": 0.0, "boxes": 0.0}
        for p in range(live):
            r = want[(int(pi[p]), tasks[int(pc[p])][0])]
            for k_ in diff:
                diff[k_] = max(diff[k_], float((res[p][k_] - r[k_]).abs().max()))
        centres = float((cc_a.cluster_centers - cc_b.cluster_centers).abs().max())
    med = {name: _median(v) for name, v in rates.items()}
    P = B * T
    ms = {name: P / v * 1e3 for name, v in med.items()}
    alone = launch_alone(dev, cc, P, T, (H // 32) * (W // 32), L)
    return {"tool": "tools/bench_sweep_choice.py", "device": "MI355X",
            "workload": {"images_per_batch": B, "captions": T, "pairs_per_image_batch": P, "image_hw": [H, W], "tokens": L, "queries": 100, "bank_rows": a.bank,
                         "image_batches_per_region": a.steps, "repeats": a.repeats, "warmup_passes": a.warmup},
            "pairs_per_s": med, "pairs_per_s_all": rates, "ms_per_image_batch": ms, "b_over_a": med["b_captured_with_choice"] / med["a_eager_loop_with_choice"],
            "choice_stage_ms_per_replay": ms["b_captured_with_choice"] - ms["c_captured_without_choice"],
            "sweep_prototypes_alone": alone, "launch_share_of_b": alone["launch_us"] * 1e-3 / ms["b_captured_with_choice"],
            "max_abs_difference_b_to_a": diff, "cluster_centers_max_abs_difference_b_to_a": centres,
            "difference_units": "scores: probability; boxes: pixels of the 480 x 640 originals",
            "captures": {"b": step_b.captures, "c": step_c.captures}, "replays": {"b": step_b.replays, "c": step_c.replays}, "xdec_failed": bool(k.XDEC_FAILED)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--captions", type=int, default=14)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--bank", type=int, default=1024, help="rows of every memory bank")
    ap.add_argument("--steps", type=int, default=20, help="image batches per timed region")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "sweep_choice.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep_choice: no GPU; nothing is measured without one")

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
