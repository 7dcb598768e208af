#!/usr/bin/env python
"""The fill phase of a distillation run at configs[4] size (batch 4 pairs, 640 x 640, 14 fresh banks of 1024 x 256, every full_label 0): what a real
run does for its first several thousand steps, measured on both paths over the same batch stream and the same np.random seed.

  captured   harness.CapturedDistillStep from step 0: one hipGraph; toist_bank_fifo pushes the rows and keeps update_count / full_label, toist_kmeans_init
             starts every sample's k-means from the bank rows ClusterCriterion.plan_fill drew
  list       harness.distillation_step on the collate_fn batch: FIFO by torch.cat, per-sample host k-means with one host read per Lloyd iteration

plus, with device events (median of --repeats), the FIFO launch alone (4 groups, each shifting its 1 MB bank) and one random-start k-means launch on
the banks as the timed steps left them (4 samples in 4 tasks; its Lloyd iteration counts are reported, and the stored-centre start beside it).
`--steady-parent` / `--steady-branch` take the `value` of three `bench.py --distill --batch 4` runs each (same machine, same session), so the file
also records that the steady state does not pay for the fill phase.  Writes profiles/distill_fill.json (--out) and prints it.

    python tools/bench_distill_fill.py --steps 20 --warmup 3
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steady-parent", type=float, nargs="*", default=None)
    ap.add_argument("--steady-branch", type=float, nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_fill.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import toist_amd
    from toist_amd import engine, harness, kernels
    from toist_amd.matcher import check_lsap_pending
    from toist_amd.optim import FusedClipAdamWEMA
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill_fill needs the GPU")
    dev = torch.device("cuda:0")
    args = harness.default_args(device="cuda", distillation=True, cluster=True, nsthl2_loss=True, softkd_loss=True, train_batch_size=a.batch)
    torch.manual_seed(0)
    model, criterion, cc0, weight_dict = toist_amd.build_model(args)
    model_noun, _, _, _ = toist_amd.build_model(args)
    for m in (model, model_noun):
        m.to(dev).train()
    cc0.to(dev)                                 # fresh: update_count = full_label = 0, banks and centres as the reference initialises them
    engine.REUSE_GRAD_BUFFERS = True
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)

    def tail(m):
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        groups = [{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
                  {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
                  {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}]
        return FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm)

    opts = [tail(model), tail(model_noun)]
    pool = []
    for j in range(4):                          # the batch stream of bench.py --distill: other images, captions, target counts and tasks every step
        b_j = harness.synthetic_distill_batch(a.batch, a.size, a.size, tokens=16, seed=2000 + 7919 * j, device=dev)
        for side_t in b_j["targets"]:
            for i, t in enumerate(side_t):
                t["dataset_name"] = f"task_{1 + (i * (j + 1) + 3 * j) % 14}_train.json"
        pool.append(b_j)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.set_stream(side)

    def timed(fn):
        np.random.seed(a.seed)
        for i in range(a.warmup):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            out = fn(a.warmup + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"pairs_per_s": round(a.batch * a.steps / dt, 2), "ms_per_step": round(1e3 * dt / a.steps, 3), "final_loss": round(float(out.detach()), 4)}

    # ---- captured, from step 0
    cc_cap = copy.deepcopy(cc0)
    cc_cap.sync_host_state()
    cap = harness.CapturedDistillStep(model, model_noun, criterion, cc_cap, opts, weight_dict, batch=a.batch, image_hw=(a.size, a.size), tokens=16,
                                      max_targets_per_image=10, stream=side)
    packed = [cap.pack(b) for b in pool]
    captured = timed(lambda i: cap.step(packed=packed[i % len(packed)]))
    check_lsap_pending()
    cc_cap.check_start_status(defer=False)
    kernels.xdec_check()
    assert cap.captures == 1 and cap.replays == a.warmup + a.steps - 1 and float(cc_cap.full_label.sum()) == 0

    # ---- list of dicts, same stream of batches, same draws
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
    listed = timed(list_step)
    assert torch.equal(cc_list.update_count, cc_cap.update_count)

    # ---- the two launches alone, on the banks the captured run left
    from toist_amd import kernels as k

    def events(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        return {"median_us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}

    B = a.batch
    tb = cap.sides[1]["targets"].distill
    host = torch.zeros(tb.nbytes, dtype=torch.uint8)
    views = [v.numpy() for v in tb._views(host)]
    tb._pack_groups(list(range(B)), views[4], views[5], views[6], views[7])          # B samples in B filling tasks
    tb.load_packed(host)
    rows = torch.randn(B, cc_cap.feature_dim, device=dev)
    lsap_rows = torch.zeros(B, dtype=torch.int32, device=dev)
    fifo = events(lambda: k.bank_fifo(cc_cap.feature_bank, cc_cap.update_count, cc_cap.full_label, tb.group_task, tb.group_off, tb.members, rows, False, lsap_rows))
    pick, chosen = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, cc_cap.feature_dim, device=dev)
    iters, status = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rs = np.random.RandomState(a.seed)
    drawn = torch.tensor(np.stack([rs.choice(cc_cap.memory_size, cc_cap.cluster_num, replace=False) for _ in range(B)]), dtype=torch.int32, device=dev)
    none = torch.full_like(drawn, -1)
    full = torch.ones_like(cc_cap.full_label)

    def km(label, init):
        k.kmeans_init(cc_cap.feature_bank, cc_cap.cluster_centers, tb.group_task, tb.group_off, tb.members, rows, 1e-4, 10000, pick, chosen, label, init, status, iters=iters)
    random_start = events(lambda: km(cc_cap.full_label, drawn))
    random_start["lloyd_iterations"] = iters.tolist()
    stored_start = events(lambda: km(full, none))          # (restarts from converged centres after the first call: the steady state's launch)
    stored_start["lloyd_iterations"] = iters.tolist()
    assert int(status) == 0

    out = {"tool": "bench_distill_fill", "device": torch.cuda.get_device_name(0), "batch_pairs": a.batch, "image": [a.size, a.size], "steps": a.steps, "warmup": a.warmup,
           "memory": "14 banks of %d x %d, fresh (every full_label 0)" % (cc0.memory_size, cc0.feature_dim),
           "fill_phase": {"captured_step": captured, "list_of_dicts_step": listed,
                          "speedup": round(captured["pairs_per_s"] / listed["pairs_per_s"], 3)},
           "launches": {"bank_fifo_%d_groups" % B: fifo, "kmeans_random_start_%d_samples" % B: random_start, "kmeans_stored_start_%d_samples" % B: stored_start}}
    if a.steady_parent and a.steady_branch:
        p_, b_ = statistics.median(a.steady_parent), statistics.median(a.steady_branch)
        out["steady_state_bench_distill_batch4"] = {"parent_pairs_per_s": a.steady_parent, "branch_pairs_per_s": a.steady_branch, "parent_median": p_, "branch_median": b_,
                                                    "branch_over_parent": round(b_ / p_, 4), "allowed_minimum": 0.98}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
