#!/usr/bin/env python
"""Headline benchmark: train images/s (640x640 synthetic images + 16-token captions, batch 8 per GPU)
for the MI355X-native TOIST/MDETR hot path (BASELINE.json: metric / configs[1]).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

One step = zero_grad -> encode -> decode -> SetCriterion (labels, boxes, cardinality, 5 aux layers) ->
backward (+ flat-buffer RCCL gradient all-reduce when N > 1) -> clip_grad_norm_(0.1) -> AdamW -> EMA,
in train mode (dropout 0.1 on).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps once and prints the line.  Everything else is measured
only with --full: the K-step region repeated (--repeats, `value` = the median region), `roofline` (the
GEMM kernel families timed launch by launch, toist_amd/csrc/gemm.hip, plus rocprofv3 passes of their
own), `cpu_baseline` (the fp32 oracle, a port of the reference's CPU path, on the host cores at N = 1)
with the matcher index bit-match, the `secondary` configurations, and at N > 1 the parameter identity
across ranks and the per-segment collectives.

--dump-outputs DIR writes what the timed path computed in its last step as DIR/<name>.npy (float32):
the loss, the predictions of every decoder layer and a fixed, seeded sample of the updated parameters.
With the same arguments the inputs are the same in every run, and so are the default (configs[1]) step's dumped
predictions and parameters (the loss to its last bits): three gradient reductions of that step that added with float atomics in completion order
(split-K bias column sums, the text embedding tables, the contrastive token gradient) now fold in a fixed order
(tests/test_gpu_determinism.py).  Float atomics remain elsewhere, e.g. the per-term loss sums (no gradient
reads them) and the mask head of --masks, so those paths are not claimed to repeat bit for bit.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E ~8 TB/s
PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
GFLOP_PER_IMG_TRAIN = 397.7  # detection train step, stem + layer1 frozen
GFLOP_PER_IMG_TRAIN_MASKS_DENSE = 839.9   # with the mask head, everything trainable (3 x 288.5 - 25.6), every map's backward multiplied through
GFLOP_MASK_HEAD_FWD = 147.5               # attention map + mask head forward of one image (100 maps)
MASK_SLOTS_PER_IMAGE, QUERIES = 10, 100   # StaticTargets capacity of the bench batches: the mask head's backward runs on the matched-pair slots (the other maps' gradients are exactly zero)
# executed flops: the dense count minus the backward of the maps that carry no gradient
GFLOP_PER_IMG_TRAIN_MASKS = round(GFLOP_PER_IMG_TRAIN_MASKS_DENSE - 2 * GFLOP_MASK_HEAD_FWD * (1 - MASK_SLOTS_PER_IMAGE / QUERIES), 1)
GFLOP_PER_IMG_TRAIN_MASKS_FROZEN = round(288.5 + 2 * GFLOP_MASK_HEAD_FWD * MASK_SLOTS_PER_IMAGE / QUERIES, 1)   # frozen-detector recipe: full forward + that backward only


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--profile-all", action="store_true", help="time every GEMM launch (diagnostic; adds host overhead)")
    ap.add_argument("--distill", action="store_true", help="config 5 on this GPU: teacher + student forward, cluster criterion, paired criterion "
                    "(eager launch: the k-means loop reads the device); use with --batch 4")
    ap.add_argument("--masks", action="store_true", help="config 3: add the segmentation head and the mask losses")
    ap.add_argument("--frozen", action="store_true", help="with --masks: the reference's segmentation recipe (scripts/train_seg.sh:5-12): --frozen_weights (detector frozen, "
                    "models/segmentation.py:22-24), --no_aux_loss, --no_contrastive_align_loss -- only bbox_attention.* / mask_head.* train")
    ap.add_argument("--mixed-sizes", action="store_true", help="configs[1] on a stream of batches of three padded image sizes (640x640, 576x704, 512x768) through "
                    "toist_amd.harness.CapturedTrainStep: one cached hipGraph per shape bucket, the library's replayed step with variable-size inputs")
    ap.add_argument("--no-secondary", action="store_true", help="do not run the short configs[2] / configs[2]-frozen / configs[4] legs (child processes) that the default N = 1 run appends as `secondary`")
    ap.add_argument("--repeats", type=int, default=None, help="hipGraph replay: the K-step timed region is run this many times (value = the MEDIAN region; first / min reported "
                    "beside it); default 3 with --full, else 1")
    ap.add_argument("--full", action="store_true", help="also measure and check what the headline figure does not need: repeated timed regions, roofline (with "
                    "rocprofv3 passes), cpu_baseline + matcher bit-match, the secondary configurations, at N > 1 parameter identity and collectives")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32, "
                    "large arrays as a fixed, seeded sample)")
    ap.add_argument("--allow-eager-fallback", action="store_true", help="N > 1: if hipGraph capture fails, run eager instead of aborting (a different launch protocol: labelled in config.launch)")
    ap.add_argument("--no-overlap", action="store_true", help="keep the text branch on the main stream (no parallel graph branch)")
    ap.add_argument("--torch-optimizer", action="store_true", help="diagnostic: torch clip_grad_norm_ + fused AdamW + foreach EMA instead of the HIP tail")
    ap.add_argument("--defer-ema", action="store_true", help="diagnostic: run the EMA update beside the next forward pass instead of inside the optimizer tail "
                                                             "(measured slower: 504 vs 514 images/s, the forward pass is HBM-sensitive)")
    ap.add_argument("--late-text-tail", action="store_true", help="diagnostic: the text encoder's share of the clip + AdamW + EMA tail is issued at the head of the "
                    "next step's text branch, beside the ResNet forward (measured slower: profiles/r04_late_tail_ab.txt)")
    ap.add_argument("--no-contrastive", action="store_true", help="drop loss_contrastive_align (the round-1 configuration; the reference's detection recipe has it on, "
                    "main.py:179-184)")
    ap.add_argument("--bf16-grads", action="store_true", help="N > 1: gradients cross the xGMI links as bfloat16 (half the bytes; the reference reduces in fp32)")
    ap.add_argument("--static-batch", action="store_true", help="replay the step on ONE fixed batch (the round-1 headline); default: every step sees a different "
                    "batch (images, captions, number of targets per image) through fixed-address input buffers, the same captured graph")
    ap.add_argument("--no-pmc", action="store_true", help="do not run the two rocprofv3 PMC passes that measure the roofline kernel's HBM traffic (the committed passes are quoted instead)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel from Python instead of replaying a captured hipGraph")
    ap.add_argument("--dump-graph", default=None, help="diagnostic: write the captured step's hipGraph (nodes + dependency edges) as a DOT file to this path")
    ap.add_argument("--glue-report", action="store_true", help="diagnostic: one EAGER step under torch.profiler; prints (stderr) every source line of toist_amd / bench.py that "
                    "launches torch (non-toist) device kernels, with the number of kernels and their device time, then exits")
    ap.add_argument("--no-early-norm", action="store_true", help="A/B: sum the squares of the text encoder's gradients inside the optimizer tail instead of at the end of "
                    "the text branch's backward pass (beside the ResNet backward)")
    ap.add_argument("--stamps", action="store_true", help="diagnostic: one-thread clock kernels at the fork / join points of the step (captured into the graph); prints (stderr) "
                    "when each branch of the LAST replayed step started and ended, in microseconds from the step's first kernel, no profiler attached")
    ap.add_argument("--host-times", action="store_true", help="diagnostic: print (stderr) the host microseconds spent inside each run_step() call of the first timed region")
    ap.add_argument("--split-graph", action="store_true", help="force the multi-GPU structure (graph: fwd+bwd | eager all-reduce | graph: clip+AdamW+EMA) on one GPU")
    a = ap.parse_args()
    if a.repeats is None:
        a.repeats = 3 if a.full else 1
    if not a.full:      # a plain run does only what the headline figure needs (--profile-all asks for its launch-by-launch timing explicitly)
        a.no_cpu_baseline = a.no_secondary = a.no_pmc = True
        a.no_roofline = a.no_roofline or not a.profile_all
    return a


SETTLE_REPLAYS = 30             # a plain run's minimum number of untimed replays before its one timed region
DUMP_SAMPLE = 1 << 22           # --dump-outputs: an array of more elements is written as this many of them (seeded indices)
DUMP_PARAMS_PER_TENSOR = 2048   # --dump-outputs: sampled elements of each trainable parameter


def param_sample(params, seed=0):
    """A fixed, seeded sample of the parameters, the same indices in every run: up to DUMP_PARAMS_PER_TENSOR elements of each tensor, in order."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for p in params:
        flat = p.detach().reshape(-1)
        idx = torch.randint(0, flat.numel(), (min(DUMP_PARAMS_PER_TENSOR, flat.numel()),), generator=g)
        parts.append(flat[idx.to(flat.device)].float())
    return torch.cat(parts)


def dump_outputs(path, arrays, seed=0):
    """--dump-outputs: every tensor of `arrays` as path/<name>.npy in float32; one of more than DUMP_SAMPLE elements becomes a fixed, seeded
    sample of DUMP_SAMPLE of them (flattened)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            t = t.reshape(-1)[torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=g).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def cpu_baseline_worker(size, threads, check_path=None):
    """BASELINE.json configs[0]: one 640x640 image + 16-token caption, detection-only forward + one matcher call on the
    fp32 oracle (a port of the reference CPU path, pinned to the reference by tests/golden).  SURVEY.md 8(d): 3 warm-up + 10 timed
    iterations, median.  With `check_path` (outputs of the GPU step dumped by the parent) it also counts the (layer, image) pairs
    whose HIP assignment differs from the oracle matcher's on the SAME fp32 logits / boxes.  Prints one JSON line."""
    import numpy as np
    import toist_amd
    from oracle import matcher_ref, model_ref
    from toist_amd import harness
    torch.set_num_threads(threads)
    res = {}
    if check_path:
        d = np.load(check_path)
        bad = checked = 0
        for bi in range(int(d["nb"])):
            logits, boxes, pm = torch.from_numpy(d[f"logits{bi}"]), torch.from_numpy(d[f"boxes{bi}"]), torch.from_numpy(d[f"pm{bi}"])
            sizes = d[f"sizes{bi}"].tolist()
            tb = torch.from_numpy(d[f"tgt_boxes{bi}"])
            tgts = [tb[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))]
            moff = np.concatenate([[0], np.cumsum([min(logits.shape[2], s_) for s_ in sizes])])
            for l in range(logits.shape[0]):
                ref = matcher_ref.hungarian_match(logits[l], boxes[l], tgts, pm)
                for i, (ri, rj) in enumerate(ref):
                    a, b = d[f"src{bi}"][l, moff[i]:moff[i + 1]], d[f"tgt{bi}"][l, moff[i]:moff[i + 1]]
                    bad += int(not (np.array_equal(a, ri.numpy()) and np.array_equal(b, rj.numpy())))
            checked += int(logits.shape[0] * logits.shape[1])
        res.update(matcher_mismatch_images=bad, matcher_checked=checked)
    args = harness.default_args(device="cpu")
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    del model
    samples, tok, targets, pmap = harness.synthetic_batch(1, size, size, tokens=16, seed=1000, max_targets=10)

    def fwd():
        with torch.no_grad():
            mc = model_ref.mdetr_encode(sd, samples.tensors, samples.mask, tok["input_ids"], tok["attention_mask"])
            out = model_ref.mdetr_decode(sd, mc)
            return matcher_ref.hungarian_match(out["pred_logits"], out["pred_boxes"], [t["boxes"] for t in targets], pmap)

    for _ in range(3):
        fwd()
    times = []
    for _ in range(10):
        t0 = time.time()
        fwd()
        times.append(time.time() - t0)
    dt = sorted(times)[len(times) // 2]
    res.update({"value": round(1.0 / dt, 4), "unit": "images/s (forward + matcher, B=1)", "cores": threads, "kind": "port",
                "sample": f"configs[0]: oracle fp32 detection forward + Hungarian matcher, 1 image {size}x{size} + 16 tokens, "
                          f"3 warm-up + 10 timed iterations on {threads} threads, median"})
    print(json.dumps(res))


def cpu_baseline(size, check_path=None):
    """Runs the CPU baseline (and the matcher bit-match check) in a child process with a hard time limit so a pathological host can
    never stall the bench."""
    import subprocess
    threads = min(os.cpu_count() or 1, 64)
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", str(size), str(threads)] + ([check_path] if check_path else []),
                             capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:  # timeout or failure: report, never block the GPU numbers
        return {"value": None, "unit": "images/s (forward + matcher, B=1)", "cores": threads, "kind": "port", "sample": f"not measured: {type(e).__name__}"}


def secondary_legs():
    """configs[2] (mask head, everything trainable), configs[2] with the reference's frozen-detector recipe and configs[4] (distillation,
    batch 4 pairs) as child runs of this script: {name: {value, unit, ms_per_step, steps, launch, workload} | {error}}."""
    import subprocess
    legs = (("configs[2]", ["--masks"]), ("configs[2] frozen recipe", ["--masks", "--frozen"]), ("configs[4]", ["--distill", "--batch", "4"]),
            ("configs[1] mixed image sizes (library CapturedTrainStep)", ["--mixed-sizes", "--steps", "12"]))
    out = {}
    for name, flags in legs:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--full", "--no-cpu-baseline", "--no-roofline", "--no-secondary", "--repeats", "1", "--steps", "10",
                                "--warmup", "3"] + flags, capture_output=True, text=True, timeout=420)
            line = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')][-1]
            d = json.loads(line)
            out[name] = {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "steps": d["steps"], "launch": d["config"].get("launch"),
                         "mfma_frac_whole_step": d["config"].get("mfma_frac_whole_step"), "workload": d["config"]["workload"]}
            for extra in ("eager_pairs_per_s", "graph_replay_any_batch_pairs_per_s", "mask_logit_parity"):
                if extra in d["config"]:
                    out[name][extra] = d["config"][extra]
        except Exception as e:
            out[name] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    return out


def pmc_traffic_live(families, timeout=300):
    """HBM bytes per launch of the roofline kernel, measured now: two rocprofv3 PMC passes over a short eager run of this script
    (FETCH_SIZE and WRITE_SIZE in SEPARATE runs, counters only with --kernel-trace, from /tmp), units and corrections as
    /opt/skills/guides/MI355X_MICROARCH.md prescribes (both counters in KiB; FETCH_SIZE doubled on gfx950 for 16-byte-per-lane loads).
    `families` = {name: (kernel-name substrings)}.  Returns ({name: (bytes_per_launch, dispatches)}, note); a family that was not
    seen is missing from the dict, a failed pass gives ({}, reason)."""
    import csv
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {}, "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="toist_pmc_", dir="/tmp")
    kib = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
                   "--no-cpu-baseline", "--no-graph", "--no-roofline", "--steps", "2", "--warmup", "1"]
            subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, timeout=timeout)
            path = os.path.join(out, "p_counter_collection.csv")
            acc = {fam: [0.0, 0] for fam in families}
            with open(path) as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") != ctr:
                        continue
                    kn = row.get("Kernel_Name", "")
                    for fam, subs in families.items():
                        if any(k_ in kn for k_ in subs):
                            acc[fam][0] += float(row["Counter_Value"])
                            acc[fam][1] += 1
            kib[ctr] = {fam: (t / n, n) for fam, (t, n) in acc.items() if n}
        out = {}
        for fam in families:
            if fam in kib["FETCH_SIZE"] and fam in kib["WRITE_SIZE"]:
                out[fam] = (int(2 * kib["FETCH_SIZE"][fam][0] * 1024 + kib["WRITE_SIZE"][fam][0] * 1024), kib["FETCH_SIZE"][fam][1])
        return out, (None if out else "no dispatch of %s in the PMC passes" % (sorted(families),))
    except Exception as e:  # profiler missing / timed out / unreadable output: the committed passes are quoted instead
        return {}, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_stats_live(families, steps, warmup, timeout=300, keep=None):
    """Average launch duration of the roofline kernel families in the REPLAYED step: one `rocprofv3 --kernel-trace --stats` pass (no counters)
    over this script's own default timed loop (hipGraph replay), i.e. the command whose summary is committed as profiles/rNN_bench_kernel_stats.csv.
    Returns ({family: (avg_us, calls)}, note).  `keep`: a path that receives a copy of the kernel_stats CSV."""
    import csv
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {}, "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="toist_kt_", dir="/tmp")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
               "--full", "--no-cpu-baseline", "--no-roofline", "--no-secondary", "--steps", str(steps), "--warmup", str(warmup)]
        subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, timeout=timeout)
        path = os.path.join(tmp, "p_kernel_stats.csv")
        acc = {fam: [0.0, 0] for fam in families}
        with open(path) as f:
            for row in csv.DictReader(f):
                kn = row.get("Name", "")
                for fam, subs in families.items():
                    if any(k_ in kn for k_ in subs):
                        acc[fam][0] += float(row["TotalDurationNs"])
                        acc[fam][1] += int(row["Calls"])
        if keep:
            os.makedirs(os.path.dirname(keep), exist_ok=True)
            shutil.copyfile(path, keep)
        out = {fam: (t / n / 1000.0, n) for fam, (t, n) in acc.items() if n}
        return out, (None if out else "no dispatch of %s in the kernel trace" % (sorted(families),))
    except Exception as e:  # profiler missing / timed out / unreadable output: the HIP-event timing of the eager pass is reported instead
        return {}, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_distillation(a, dev, rank, world):
    """BASELINE configs[4] per GPU: noun-pronoun distillation step (engine.py:119-250) -- teacher and student forward,
    memory-bank update + k-means prototypes, paired criterion with softkd / nsthl2, backward through both models, one
    fused optimizer tail per model (the reference clips the two models separately)."""
    import toist_amd
    from toist_amd import harness, kernels, parallel
    from toist_amd.optim import FusedClipAdamWEMA
    args = harness.default_args(device="cuda", distillation=True, cluster=True, nsthl2_loss=True, softkd_loss=True, train_batch_size=a.batch)
    torch.manual_seed(0)
    model, criterion, cluster_criterion, weight_dict = toist_amd.build_model(args)
    model_noun, _, _, _ = toist_amd.build_model(args)
    for m in (model, model_noun):
        m.to(dev)
        parallel.broadcast_parameters(m)
        m.train()
    cluster_criterion.to(dev)
    cluster_criterion.full_label.fill_(1)   # steady state: banks full, k-means starts from the stored centres
    from toist_amd import engine as _engine
    _engine.REUSE_GRAD_BUFFERS = True
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)

    def tail(m):
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        groups = [{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
                  {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
                  {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}]
        src = [v for v in m.state_dict().values() if v.is_floating_point()]
        return FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm,
                                 ema=list(zip(src, [v.detach().clone() for v in src])), ema_decay=0.9998)

    opts = [tail(model), tail(model_noun)]
    batch = harness.synthetic_distill_batch(a.batch, a.size, a.size, tokens=16, seed=1000 + rank, device=dev)
    sync = parallel.GradSync([model, model_noun])

    def step():
        kernels.SEED_DEV.add_(1000003)
        for o in opts:
            o.zero_grad(set_to_none=True)
        with sync:
            total, _ = harness.distillation_step(model, model_noun, criterion, cluster_criterion, weight_dict, batch)
            total.backward()
            sync.finish()
        for o in opts:
            o.step()
        return total

    # everything below runs on ONE side stream -- the stream the step is captured on later: the launchers' per-stream scratch, the programs' reused gradient
    # buffers and autograd's accumulation nodes then never change streams between the eager steps and the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.set_stream(side)
    for _ in range(a.warmup):
        step()

    def timed(fn):
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = fn()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt_], device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt_ = float(t)
        return dt_, out

    dt, last = timed(step)             # eager: what a loop over NEW batches gets today (the caption-driven tables of a batch are built on the host)
    launch, eager_rate, graph_rate = "eager", round(a.batch * world * a.steps / dt, 3), None
    final_loss = round(float(last.detach()), 4)
    last_loss = last.detach()
    del last
    any_rate = None
    if world == 1 and not a.no_graph:
        # Round 6: ONE hipGraph of the step for ANY batch (toist_amd.harness.CapturedDistillStep): every per-batch table -- target counts / LSAP problem
        # sizes, the grouping of the images by task, the token tables of the captions -- lives at fixed device addresses (matcher.StaticTargets +
        # distill.DistillTables per side) that are refilled before each replay.  The timed loop feeds a DIFFERENT batch every step (a pool of resident
        # batches with other images, captions, target counts and tasks, their host tables packed ahead as a loader worker would).
        try:
            torch.cuda.synchronize()
            cap = harness.CapturedDistillStep(model, model_noun, criterion, cluster_criterion, opts, weight_dict, batch=a.batch, image_hw=(a.size, a.size), tokens=16,
                                              max_targets_per_image=10, stream=side)
            pool = []
            for j in range(4):
                b_j = harness.synthetic_distill_batch(a.batch, a.size, a.size, tokens=16, seed=2000 + 7919 * j + rank, device=dev)
                for side_t in b_j["targets"]:
                    for i, t in enumerate(side_t):
                        t["dataset_name"] = f"task_{1 + (i * (j + 1) + 3 * j) % 14}_train.json"
                pool.append(cap.pack(b_j))
            it = [0]

            def replayed():
                it[0] += 1
                return cap.step(packed=pool[it[0] % len(pool)])
            for _ in range(max(a.warmup, 2) + 1):
                replayed()
            dt_g, last_g = timed(replayed)
            from toist_amd.matcher import check_lsap_pending
            check_lsap_pending()
            kernels.xdec_check()      # (the XCD-resident decoder launches of the teacher's backward run beside the softkd solve: no bounded spin may have expired)
            assert cap.captures == 1 and math.isfinite(float(last_g))
            any_rate = graph_rate = round(a.batch * world * a.steps / dt_g, 3)
            launch = ("hipGraph replay, every step a different batch (harness.CapturedDistillStep: 1 graph, %d replays; 4 resident batches with different images, captions, "
                      "0..10 targets per image and tasks); eager list-of-dicts step: %.1f pairs/s" % (cap.replays, eager_rate))
            dt, final_loss, last_loss = dt_g, round(float(last_g.detach()), 4), last_g.detach()
        except Exception as e:      # stays on the eager number, loudly
            print(f"[bench] distillation: hipGraph capture failed ({type(e).__name__}: {e}); reporting the eager step", file=sys.stderr)
            torch.cuda.synchronize()
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"loss": last_loss.reshape(1), "params_sample": param_sample(p for p in model.parameters() if p.requires_grad),
                                      "noun_params_sample": param_sample(p for p in model_noun.parameters() if p.requires_grad)})
    if rank == 0:
        print(json.dumps({"metric": "train images/sec/node (640x640) + matcher index bit-match", "value": round(a.batch * world * a.steps / dt, 3), "unit": "images/s (pairs)",
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(1000 * dt / a.steps, 3), "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                          "config": {"workload": f"configs[4]: noun-pronoun distillation, teacher + student (ResNet-101 + RoBERTa-base + 6+6 each), batch {a.batch} pairs/GPU "
                                                 f"{a.size}x{a.size}, cluster memory 1024 x 14 tasks + k-means(3), softkd + nsthl2 + cluster losses, two fused optimizer tails",
                                     "global_batch": a.batch * world, "parallelism": f"dp{world}", "final_loss": final_loss, "launch": launch, "eager_pairs_per_s": eager_rate,
                                     "graph_replay_any_batch_pairs_per_s": any_rate}}))
    if world > 1:
        torch.distributed.destroy_process_group()


def bench_mixed_sizes(a, dev):
    """configs[1] through toist_amd.harness.CapturedTrainStep on a stream that alternates three image sizes (the reference resizes to
    480..800 x <= 1333, datasets/tdod.py:305-319): every bucket's graph is captured on first use, then the timed region replays them."""
    import toist_amd
    from toist_amd import harness, kernels
    from toist_amd.optim import FusedClipAdamWEMA
    args = harness.default_args(device="cuda", contrastive_align_loss=True)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev).train()
    criterion.train()
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
              {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
              {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}]
    src = [v for v in model.state_dict().values() if v.is_floating_point()]
    opt = FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, ema=list(zip(src, [v.detach().clone() for v in src])),
                            ema_decay=0.9998)
    cap = harness.CapturedTrainStep(model, criterion, opt, weight_dict, batch=a.batch, max_targets_per_image=10, pad_hw=64, max_graphs=4)
    sizes = ((640, 640), (576, 704), (512, 768))
    from toist_amd.matcher import StaticTargets
    packer = StaticTargets(a.batch, 10, args.num_queries, 256, dev)      # same arena layout as the buckets' own (batch, capacity, queries, K)
    pool = []
    for i in range(6):
        h, w = sizes[i % 3]
        s_i, tok_i, t_i, pm_i = harness.synthetic_batch(a.batch, h, w, tokens=16, seed=1000 + 7919 * i, max_targets=10)
        packed = packer.pack(t_i, pm_i, criterion.token_masks_host(t_i, None))
        pool.append((s_i.to(dev), tok_i.to(dev), t_i, pm_i, packed))
    for i in range(max(a.warmup, 6)):      # first pass: one eager step + capture per bucket
        s_i, tok_i, t_i, pm_i, packed = pool[i % 6]
        cap.step(s_i, tok_i, t_i, pm_i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        s_i, tok_i, t_i, pm_i, packed = pool[i % 6]
        last = cap.step(s_i, tok_i, packed=packed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {"loss": last.detach().reshape(1), "params_sample": param_sample(p for _, p in named)})
    print(json.dumps({"metric": "train images/sec/node (640x640, bs=8/GPU) + matcher index bit-match", "value": round(a.batch * a.steps / dt, 3), "unit": "images/s", "n_gpus": 1,
                      "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(1000 * dt / a.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                      "dtype": "bf16", "data": "synthetic",
                      "config": {"workload": f"configs[1] recipe on a stream alternating three image sizes {sizes} (equal pixel counts within 4 %), batch {a.batch}, 16-token captions, 0..10 targets "
                                             "per image, through toist_amd.harness.CapturedTrainStep (one cached hipGraph per padded shape bucket)",
                                 "global_batch": a.batch, "parallelism": "dp1", "final_loss": round(float(last), 4), "launch": f"hipGraph replay, {cap.captures} cached graphs, {cap.replays} replays"}}))


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--cpu-baseline-worker":
        cpu_baseline_worker(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] if len(sys.argv) > 4 else None)
        return
    a = parse()
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    backend = os.environ.get("TOIST_DIST_BACKEND", "nccl")   # "gloo": single-GPU smoke test of the N > 1 control flow
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", init_method="env://", world_size=world, rank=rank, device_id=dev)
        else:
            torch.distributed.init_process_group(backend, init_method="env://", world_size=world, rank=rank)

    import toist_amd
    from toist_amd import harness, kernels, parallel
    from toist_amd.mdetr import weighted_total
    # Three GEMM kernel families are timed launch by launch (HIP events on the launch stream) -- together ~50 % of the step's kernel time:
    #   tile code 65   gemm_kernel<64,64,64,...>: the generic 64 x 64 tile -- the transformer's and the text encoder's linears, their data and weight
    #                  gradients, small convolutions (15 template instantiations; the largest family by summed time in round 4, untimed until round 5)
    #   tile code 135  panel2_kernel: 1x1 convolutions / linears with K <= 256 and their data gradients (HBM-bound: ~100 flop per algorithmic byte,
    #                  below the ridge 2500 TFLOP/s / 8 TB/s = 312)
    #   tile code 136  gemm128_kernel: 3x3 convolutions of ResNet layers 2-4, their data gradients, 1x1 / linear launches with K >= 768
    # `roofline` = the family with the largest summed time in THIS run.
    global ROOFLINE_KEYS
    ROOFLINE_KEYS = lambda key: key[0] in (65, 135, 136)
    if a.distill:
        return bench_distillation(a, dev, rank, world)
    if a.mixed_sizes:
        if world > 1:
            raise SystemExit("--mixed-sizes is a single-GPU leg")
        return bench_mixed_sizes(a, dev)
    # the reference's default detection recipe (scripts/train_dete.sh): labels + boxes + cardinality + contrastive_align, 5 aux layers;
    # the segmentation recipe (scripts/train_seg.sh) passes --no_contrastive_align_loss
    contrastive = not a.no_contrastive and not a.masks
    if a.frozen and not a.masks:
        raise SystemExit("--frozen is the segmentation recipe: use it with --masks")
    args = harness.default_args(device="cuda", masks=a.masks, mask_model="smallconv" if a.masks else "none", contrastive_align_loss=contrastive,
                                frozen_weights="detector_checkpoint.pth" if a.frozen else None, aux_loss=not a.frozen)
    torch.manual_seed(0)
    model, criterion, _, weight_dict = toist_amd.build_model(args)
    model.to(dev)
    parallel.broadcast_parameters(model)
    model.train()
    criterion.train()

    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [
        {"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
        {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
        # "late" (--late-text-tail): the text encoder's share of the optimizer tail (67 % of its bytes) is issued at the head of the next step's
        # text branch, beside the ResNet forward (toist_amd.optim.FusedClipAdamWEMA).  Measured NEGATIVE (profiles/r04_late_tail_ab.txt:
        # 12.48 -> 13.3 ms per step; the forward pass is sensitive to the 4.7 GB of HBM traffic beside it), so it is off by default.
        {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr, "late": a.late_text_tail and not a.torch_optimizer and not a.defer_ema,
         "early_norm": not a.no_early_norm},
    ]
    from toist_amd import engine as _engine
    _engine.REUSE_GRAD_BUFFERS = True   # this loop never keeps a gradient across optimizer.zero_grad()
    if a.no_overlap:
        _engine.OVERLAP = "off"
    use_graph = not a.no_graph and not a.profile_all
    split_graph = use_graph and (world > 1 or a.split_graph)
    parallel.enable_backward_cuts(model, split_graph)
    if a.torch_optimizer:
        opt = torch.optim.AdamW(groups, lr=args.lr, weight_decay=args.weight_decay, fused=True, capturable=use_graph)
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)  # bumped every step: fresh dropout masks per replay
    ema_src = [v for v in model.state_dict().values() if v.is_floating_point()]
    ema = [v.detach().clone() for v in ema_src]
    all_params = [p for _, p in named]
    if not a.torch_optimizer:
        # clip_grad_norm_(0.1) + AdamW (3 groups) + EMA + bf16 compute-copy refresh: csrc/optim.hip, 3 launches per step
        from toist_amd.optim import FusedClipAdamWEMA
        # --defer-ema: the moving average of step i is folded in on a side stream beside the forward pass of step i+1 (same values, one
        # update per step); off by default -- the extra HBM traffic slows the forward pass by more than the tail gains
        opt = FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, ema=list(zip(ema_src, ema)),
                                ema_decay=0.9998, defer_ema=a.defer_ema)
    ema_stream = torch.cuda.Stream() if (not a.torch_optimizer and a.defer_ema) else None

    samples, tok, targets, pmap = harness.synthetic_batch(a.batch, a.size, a.size, tokens=16, seed=1000 + rank, device=dev, with_masks=a.masks)
    sync = parallel.GradSync(model)
    # Shape-agnostic step: NBATCH different synthetic batches (images, token ids, 0..10 targets per image) are resident in HBM; before
    # every step the next one is copied into the fixed-address input buffers the captured graph reads (device copies of images /
    # ids, one pinned H2D copy of the packed targets: matcher.StaticTargets; with --masks the ground-truth masks of the batch travel
    # in the same object, round 5).
    dynamic = not a.static_batch
    crit_targets, crit_pmap = targets, pmap
    feed = None
    if dynamic:
        from toist_amd.matcher import StaticTargets
        NBATCH = 4
        st = StaticTargets(a.batch, 10, args.num_queries, 256, dev, mask_hw=(a.size, a.size) if a.masks else None)
        pool = []
        for i in range(NBATCH):
            s_i, tok_i, t_i, pm_i = harness.synthetic_batch(a.batch, a.size, a.size, tokens=16, seed=1000 + rank + 7919 * i, max_targets=10, with_masks=a.masks)
            masks_i = criterion.token_masks_host(t_i, None) if contrastive else None
            pool.append((s_i.tensors.to(dev), tok_i["input_ids"].to(dev), st.pack(t_i, pm_i, masks_i), t_i, pm_i))
        crit_targets, crit_pmap = st, None
        state = {"i": 0}

        def feed():
            img, ids, packed, _, _ = pool[state["i"] % NBATCH]
            state["i"] += 1
            samples.tensors.copy_(img)
            tok["input_ids"].copy_(ids)
            st.load_packed(packed)

        feed()

    flats = []  # flat fp32 gradient buffers of the backward programs (filled by the GradSync hook)

    cut_state = {}

    if a.stamps:
        kernels.STAMPS = {"buf": torch.zeros(64, dtype=torch.int64, device=dev), "names": []}

    def fwd_bwd():
        kernels.stamp("step.start")
        kernels.SEED_DEV.add_(1000003)
        if ema_stream is not None:          # EMA of the previous step's parameters, beside this forward / backward
            ema_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(ema_stream):
                opt.ema_update()
        mc = model(samples, tok, encode_and_save=True)
        out = model(samples, tok, encode_and_save=False, memory_cache=mc)
        losses = criterion(mc, out, crit_targets, crit_pmap, None)
        total = weighted_total(losses, weight_dict)
        total.backward()                     # with the backbone cut (N > 1): everything but the backbone
        if ema_stream is not None:
            torch.cuda.current_stream().wait_stream(ema_stream)     # joined before the optimizer rewrites the parameters
        cut_state["mc"] = mc
        if a.dump_outputs:      # the step's predictions (static tensors of the captured graph): read after the timed steps
            cut_state["pred"] = {"pred_logits": out["_stacked"]["pred_logits"], "pred_boxes": out["_stacked"]["pred_boxes"],
                                 **({"pred_masks": out["pred_masks"]} if "pred_masks" in out else {})}
        return total

    def bwd_cut(name):
        parallel.backward_cut(cut_state["mc"], name)

    def optimize():
        if not a.torch_optimizer:
            kernels.stamp("opt.start")
            opt.step()
            kernels.stamp("opt.end")
            return
        torch.nn.utils.clip_grad_norm_(all_params, args.clip_max_norm, foreach=True)
        opt.step()
        with torch.no_grad():
            torch._foreach_mul_(ema, 0.9998)
            torch._foreach_add_(ema, ema_src, alpha=1.0 - 0.9998)

    def step(zero=True):
        """Eager step: every kernel launched from Python; gradient all-reduce overlapped with backward."""
        if zero:
            opt.zero_grad(set_to_none=True)
        if feed is not None:
            feed()
        with sync:
            total = fwd_bwd()
            for name in parallel.BACKWARD_CUTS:      # text | layer4 | layer3 | stem .. layer2: each flat buffer is all-reduced when its segment is done
                bwd_cut(name)
            sync.finish()
        optimize()
        return total

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    if a.glue_report:
        import collections
        import traceback
        from torch.utils._python_dispatch import TorchDispatchMode
        NO_KERNEL = ("aten.empty", "aten.new_empty", "aten.empty_like", "aten.empty_strided", "aten.resize_", "aten.set_", "aten.record_stream", "aten._local_scalar_dense",
                     "aten.lift_fresh", "aten.is_", "aten.sym_", "aten._has_compatible", "aten.is_pinned")

        def launches(func, out):
            name = str(func)
            if any(name.startswith(v) for v in NO_KERNEL):
                return False
            try:        # a pure view: the result aliases an argument without writing it
                rets = func._schema.returns
                if rets and all(r.alias_info is not None and not r.alias_info.is_write for r in rets):
                    return False
            except Exception:
                pass
            return True

        agg = collections.OrderedDict()

        class Glue(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                name = str(func)
                if not launches(func, out):
                    return out
                on_dev = any(torch.is_tensor(x) and x.is_cuda for x in list(args) + list((kwargs or {}).values()) + ([out] if torch.is_tensor(out) else []))
                if not on_dev:
                    return out
                fr = "(no toist frame)"
                for f in reversed(traceback.extract_stack()[:-1]):
                    if ("toist_amd/" in f.filename or f.filename.endswith("bench.py")) and not f.filename.endswith("kernels.py"):
                        fr = f"{'toist_amd/' + f.filename.split('toist_amd/')[-1] if 'toist_amd/' in f.filename else 'bench.py'}:{f.lineno} {f.name}"
                        break
                ent = agg.setdefault((fr, name), [0])
                ent[0] += 1
                return out

        for _ in range(2):
            step()
        torch.cuda.synchronize()
        with Glue():
            step()
        torch.cuda.synchronize()
        print(f"[bench] torch operators on device tensors in one eager step (views excluded): {sum(v[0] for v in agg.values())}", file=sys.stderr)
        for (frame, name), (calls,) in agg.items():
            print(f"  {calls:3d} x {name:34s} {frame}", file=sys.stderr)
        return

    if use_graph:
        # The step (forward, criterion, backward, clip, AdamW, EMA: ~1500 kernel launches) is captured once into
        # hipGraphs and replayed: the Python/ctypes launch path (~10-20 us per launch) would otherwise bound the
        # step.  Inputs are static device tensors; dropout masks change per replay through the device-side seed
        # word.  With several ranks the step is four graphs (see run_step below): the autograd graph is cut at the
        # outputs of the backbone and of the text encoder so the all-reduce of every other gradient (RoBERTa +
        # transformer + heads, 80 % of the bytes) runs on RCCL's stream underneath the backbone backward.
        try:
            from toist_amd import functions
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), kernels.tables_beside_graph():     # pointer tables of grouped launches: filled once, beside the captures
                for _ in range(max(a.warmup, 2)):
                    step()
                opt.zero_grad(set_to_none=True)
                if not split_graph:
                    graph = torch.cuda.CUDAGraph()
                    if a.dump_graph:
                        graph.enable_debug_mode()
                    with torch.cuda.graph(graph, stream=side):
                        static_loss = fwd_bwd()
                        optimize()
                    if a.dump_graph:
                        graph.debug_dump(a.dump_graph)
                else:
                    # no collective inside a capture: the hook only collects the flat gradient buffers of each segment
                    functions.GRAD_SYNC = lambda f: flats.append(f) if f is not None else None
                    graph_a = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph_a, stream=side):
                        static_loss = fwd_bwd()
                    n_head = len(flats)
                    graph_text = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph_text, stream=side):
                        bwd_cut("text")
                    n_text = len(flats)
                    # the ResNet body backward as three graphs (layer4 | layer3 | stem .. layer2; --masks: one, the body is one program):
                    # the all-reduce of a stage's gradients is issued between them
                    bb_graphs, bb_ends = [], []
                    for name in parallel.BACKWARD_CUTS[1:]:
                        if name != "backbone" and name not in cut_state["mc"].get("_native", {}).get("cuts", {}):
                            continue
                        g_ = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g_, stream=side):
                            bwd_cut(name)
                        bb_graphs.append(g_)
                        bb_ends.append(len(flats))
                    functions.GRAD_SYNC = None
                    # gradients that no program's flat buffer carries (parameters fed to a program as an INPUT and differentiated by
                    # autograd: query_embed.weight): static tensors of the captured head graph, reduced with the head segment
                    spans = [(f.data_ptr(), f.data_ptr() + f.numel() * f.element_size()) for f in flats]
                    rest_grads = [p.grad for _, p in named if p.grad is not None and not any(lo <= p.grad.data_ptr() < hi for lo, hi in spans)]
                    graph_b = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph_b, stream=side):
                        optimize()
        except Exception as e:   # N > 1 with --allow-eager-fallback: eager launches with overlapped all-reduces (a different protocol, labelled in config.launch)
            if world == 1 or not a.allow_eager_fallback:
                raise
            print(f"[bench] rank {rank}: hipGraph capture failed ({type(e).__name__}: {e}); running eager", file=sys.stderr)
            functions.GRAD_SYNC = None
            parallel.enable_backward_cuts(model, False)
            torch.cuda.synchronize()
            use_graph = split_graph = False
    if use_graph:
        torch.cuda.current_stream().wait_stream(side)

        if not split_graph:
            def run_step():
                if feed is not None:
                    feed()
                graph.replay()
                return static_loss
        else:
            text_stream = torch.cuda.Stream()

            def run_step():
                # main stream: [forward + criterion + backward of heads / decoder / encoder] -> [backbone backward] -> tail
                # text stream:                                                  [RoBERTa backward] (beside the backbone)
                # RCCL stream:               all-reduce(transformer) -> all-reduce(text) -> all-reduce(layer4) -> all-reduce(layer3) -> all-reduce(layer2)
                main = torch.cuda.current_stream()
                if feed is not None:
                    feed()
                graph_a.replay()
                if world > 1:
                    h_head = parallel.all_reduce_mean_async(flats[:n_head] + rest_grads, bf16=a.bf16_grads)
                text_stream.wait_stream(main)
                with torch.cuda.stream(text_stream):
                    graph_text.replay()
                    if world > 1:
                        h_text = parallel.all_reduce_mean_async(flats[n_head:n_text], bf16=a.bf16_grads)
                h_bb, beg = [], n_text
                for g_, end in zip(bb_graphs, bb_ends):      # layer4 -> all-reduce under layer3 -> all-reduce under layer2 -> ...
                    g_.replay()
                    if world > 1 and end > beg:
                        h_bb.append(parallel.all_reduce_mean_async(flats[beg:end], bf16=a.bf16_grads))
                    beg = end
                if world > 1:
                    h_head.wait()
                    h_text.wait()
                    for h_ in h_bb:
                        h_.wait()
                main.wait_stream(text_stream)
                graph_b.replay()
                return static_loss
        # W untimed steps on the path that is timed (the eager steps above only prepared the capture).  A plain run times ONE region, and the
        # first region after a short warm-up runs 1-3 % slower than the ones after it (`repeats.first` of --full, whose `value` is the median
        # region): it replays at least SETTLE_REPLAYS steps first, a fixed count, so every rank runs the same steps and the outputs repeat
        warm_run = {"eager_steps": max(a.warmup, 2), "replayed_steps": max(a.warmup, 1 if a.full else SETTLE_REPLAYS)}
        for _ in range(warm_run["replayed_steps"]):
            run_step()
    else:
        warm_run = {"eager_steps": a.warmup}
        for _ in range(a.warmup):
            step()
        run_step = step
    prof = None
    if rank == 0 and not a.no_roofline and not use_graph:
        prof = {"key": None if a.profile_all else ROOFLINE_KEYS, "records": [], "other": {}}
    barrier()
    kernels.PROFILE = prof
    t0 = time.perf_counter()
    host_us = []
    for _ in range(a.steps):
        th = time.perf_counter()
        last = run_step()
        host_us.append(1e6 * (time.perf_counter() - th))
    barrier()
    dt = time.perf_counter() - t0
    if a.stamps and rank == 0:
        st_ = kernels.STAMPS
        vals = st_["buf"][:len(st_["names"])].tolist()
        t00 = vals[st_["names"].index("step.start")] if "step.start" in st_["names"] else min(vals)
        print("[bench] stamps of the last step (us from step.start; 100 MHz device clock): " +
              ", ".join(f"{n} {0.01 * (v - t00):.0f}" for n, v in sorted(zip(st_["names"], vals), key=lambda nv: nv[1])), file=sys.stderr)
    if a.host_times and rank == 0:
        print("[bench] host us inside each run_step() call: " + " ".join(f"{u:.0f}" for u in host_us) + f" | region {1e3 * dt:.2f} ms", file=sys.stderr)
    kernels.PROFILE = None
    loss_val = float(last)
    kernels.xdec_check()        # a bounded spin of an XCD-resident decoder launch expired (its group was not co-resident): the numbers would be invalid
    # the same K-step region again (replayed graphs only: nothing is instrumented there): boxes of the pool differ by +- 8 % and one
    # 0.3 s region is one sample -- `value` stays the FIRST region, the spread is reported beside it
    region_ms = [1000 * dt / a.steps]
    if use_graph and prof is None:
        for _ in range(max(a.repeats, 1) - 1):
            barrier()
            t1 = time.perf_counter()
            for _ in range(a.steps):
                run_step()
            barrier()
            region_ms.append(1000 * (time.perf_counter() - t1) / a.steps)
        if len(region_ms) > 1:      # `value` = the MEDIAN region (every region is K steps between barrier + synchronize); the first one is kept in `repeats`
            dt = sorted(region_ms)[len(region_ms) // 2] * a.steps / 1000.0
    if not a.torch_optimizer:
        opt.finish()        # the late group's update of the last replay (outside the timed regions: every timed step applied one update per group)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"loss": last.reshape(1), **cut_state["pred"], "params_sample": param_sample(p for _, p in named)})
    if not a.no_roofline and use_graph:
        # kernel-level timing needs per-launch HIP events, which a replayed graph cannot carry: time the
        # same K steps once more, eagerly, on the same stream right after the timed region (every rank runs
        # them -- they contain the gradient / num_boxes collectives -- only rank 0 records)
        if rank == 0:
            prof = {"key": ROOFLINE_KEYS, "records": [], "other": {}}
            kernels.PROFILE = prof
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        kernels.PROFILE = None
    if world > 1:
        t = torch.tensor([dt], device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
    params_identical, params_differing = None, []
    if world > 1 and a.full:
        # after the timed steps every rank must hold the same parameters (same broadcast start, averaged gradients, same optimizer tail)
        with torch.no_grad():
            digest = torch.stack([p.detach().double().sum() for _, p in named]).to(dev)
            lo, hi = digest.clone(), digest.clone()
            torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
            torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
            params_identical = bool(torch.equal(lo, hi))
            params_differing = [named[i][0] for i in (lo != hi).nonzero().flatten().tolist()]
    collectives = None
    if world > 1 and a.full and use_graph and split_graph and flats:
        # the three gradient collectives of the step, each alone on the machine: what the RCCL ring achieves per xGMI link
        collectives = {name: parallel.measure_all_reduce(fl, bf16=a.bf16_grads) for name, fl in
                       [("transformer+heads", flats[:n_head]), ("text_encoder", flats[n_head:n_text])] +
                       [("backbone stage %d of %d (layer4 first)" % (i + 1, len(bb_ends)), flats[b_:e_]) for i, (b_, e_) in enumerate(zip([n_text] + bb_ends[:-1], bb_ends))] if fl}

    if rank == 0:
        ips = a.batch * world * a.steps / dt
        gflop_img = (GFLOP_PER_IMG_TRAIN_MASKS_FROZEN if a.frozen else GFLOP_PER_IMG_TRAIN_MASKS) if a.masks else GFLOP_PER_IMG_TRAIN
        res = {
            "metric": "train images/sec/node (640x640, bs=8/GPU) + matcher index bit-match", "value": round(ips, 3), "unit": "images/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(1000 * dt / a.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": (("configs[2], the reference's FROZEN-detector segmentation recipe (scripts/train_seg.sh: --frozen_weights --no_aux_loss --no_contrastive_align_loss; only bbox_attention / mask_head train): " if a.frozen else "configs[2] (det + mask head + mask losses, everything trainable): ") + "mask head backward on the matched maps only (<= 10 pair slots per image of 100 maps; loss_masks reads pred_masks[src_idx], every other map's gradient is exactly zero; gflop_per_image counts executed flops, the dense count is 839.9 / 583.5); " if a.masks else "") + f"configs[1]: ResNet-101 + RoBERTa-base + 6+6 transformer, 100 queries, batch {a.batch}/GPU {a.size}x{a.size}, "
                                   "16-token captions, detection loss (labels+boxes+cardinality" + ("+contrastive_align" if contrastive else "") + (", no aux layers" if a.frozen else ", 5 aux layers") + "), dropout 0.1, "
                                   "clip 0.1 + AdamW + EMA" + (" (torch)" if a.torch_optimizer else " (fused HIP tail)") + "; random-init weights; " +
                                   ("every step a different batch (4 resident batches, 0..10 targets per image) through fixed-address inputs" if dynamic else "one fixed batch"),
                       "untimed_steps_run": warm_run,     # `warmup` is the argument; these ran before the timed steps (a plain replayed run: >= SETTLE_REPLAYS)
                       "global_batch": a.batch * world, "parallelism": f"dp{world}", "final_loss": round(loss_val, 4), "launch": ("%d hipGraphs (head | text || backbone layer4 | layer3 | layer2 | tail), gradient all-reduces under the backbone backward" % (3 + len(bb_graphs)) if split_graph else "hipGraph replay") if use_graph else "eager",
                       **({"mask_logit_parity": "STATED DEVIATION from SURVEY 8(d) (atol 5e-2, rtol 5e-2): pred_masks of all 800 maps at 640x640 against the fp32 oracle are within "
                                                "1e-1 + 5e-2*|ref| element-wise (measured max abs error 0.113 on logits of magnitude <= 2.5, worst excess over 5e-2*|ref| 0.097, relative "
                                                "Frobenius error 0.023: five bf16-stored 3x3 convolution + GroupNorm stages); gradients of all 31 mask-branch tensors: cosine >= 0.9992 "
                                                "(tests/test_gpu_b8_masks_parity.py, profiles/r06_masks_grad_parity.json)"} if a.masks else {}),
                       "decoder": ("2 XCD-resident launches (toist_xdec_fwd / toist_xdec_bwd, one image per XCD)" if kernels.XDEC_LAUNCHES > 0 else
                                   "per-op launches (the XCD-resident launches need the GPU to themselves: ranks share a device, TOIST_XDEC=0, or not 8 XCDs x 32 CUs)"),
                       "gflop_per_image": gflop_img,
                       "mfma_frac_whole_step": round(ips / world * gflop_img / 1000.0 / PEAK_BF16_TFLOPS, 5)},
        }
        if len(region_ms) > 1:
            srt = sorted(region_ms)
            res["repeats"] = {"ms_per_step": [round(v, 3) for v in region_ms], "min": round(srt[0], 3), "median": round(srt[len(srt) // 2], 3),
                              "images_per_s_median": round(a.batch * world / (srt[len(srt) // 2] * 1e-3), 1),
                              "first": round(region_ms[0], 3),
                              "note": "the K-step timed region (barrier + synchronize on both sides) run %d times back to back; `value` / `ms_per_step` are the MEDIAN region, `first` is the first" % len(region_ms)}
        if world > 1 and a.full:
            res["config"]["parameters_identical_across_ranks"] = params_identical
        if collectives is not None:
            res["collectives"] = collectives
            if not params_identical:
                res["config"]["parameters_differing"] = {"count": len(params_differing), "first": params_differing[:12]}
            res["config"]["gradient_wire_dtype"] = "bf16" if a.bf16_grads else "f32"
        if prof is not None and prof["records"] and prof["key"] is not None:
            # Three kernel families are timed launch by launch (HIP events on the launch stream, the eager steps): the generic 64 x 64 tile
            # (tile code 65), the short-K panel kernel (135, HBM-bound) and gemm128_kernel (136, MFMA-bound).  `roofline` is the family with the
            # LARGEST share of the step's kernel time in THIS run; each one is also reported under its own name, with `traffic` from one pair
            # of rocprofv3 PMC passes.
            FAMS = {"generic": (65, ("gemm_kernel<64, 64, 64",)), "hbm": (135, ("panel_kernel", "panel2_kernel")),
                    "mfma": (136, ("gemm128_kernel",))}
            fams = {fam: [r for r in prof["records"] if r[3][0] == code] for fam, (code, _) in FAMS.items()}
            pmc, why = {}, "PMC passes skipped (--no-pmc / N > 1)"
            if world == 1 and not a.no_pmc:
                pmc, why = pmc_traffic_live({fam: subs for fam, (_, subs) in FAMS.items()})
            # launch durations: the family's average in a rocprofv3 kernel trace of the REPLAYED step (what profiles/rNN_bench_kernel_stats.csv holds);
            # the HIP events around the eager launches of the pass above stay in the entry as `avg_launch_us_hip_events` (they read 10-20 % longer:
            # a launch between two event records on an otherwise idle stream starts cold)
            ktrace, why_kt = {}, "kernel-trace pass skipped (--no-pmc / N > 1)"
            if world == 1 and not a.no_pmc and use_graph:
                ktrace, why_kt = kernel_stats_live({fam: subs for fam, (_, subs) in FAMS.items()}, a.steps, a.warmup,
                                                   keep=os.path.join("gpurun_out", "bench_kernel_stats.csv") if os.path.isdir("gpurun_out") else None)
            pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
            pname = next((n_ for n_ in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json") if os.path.exists(os.path.join(pdir, n_))), None)
            KERNEL_TEXT = {"generic": "gemm_kernel<64,64,64,A kind,B kind,ring slots,lean epilogue> (tile code 65: the generic 64x64x64 tile -- linears of the cross-modal transformer and of RoBERTa, their data and weight gradients, small convolutions)",
                           "hbm": "panel2_kernel<{B_ROWK,B_KROW},act,BM> (tile code 135: 1x1 convolutions / linears with K <= 256 and their data gradients)",
                           "mfma": "gemm128_kernel<A kind, B kind, NS> (tile code 136: 3x3 convolutions of ResNet layers 2-4, their data gradients, 1x1 / linear launches with K >= 768; 128x128 tiles, 64x64 wave tiles)"}
            entries, fam_ms = {}, {}
            for fam, recs in fams.items():
                if not recs:
                    continue
                ms = sum(r[0].elapsed_time(r[1]) for r in recs)
                fl, nb, n = sum(r[2] for r in recs), sum(r[5] for r in recs), len(recs)
                ms_events = ms
                timed = "HIP events around each launch, %d eager steps %s" % (a.steps, "after the graph-replayed timed region" if use_graph else "inside the timed region")
                if fam in ktrace:          # per-launch flops / bytes from the eager pass's records, duration from the replayed step's kernel trace
                    ms = ktrace[fam][0] * 1e-3 * n
                    timed = ("rocprofv3 --kernel-trace --stats of `bench.py --full --no-cpu-baseline --no-roofline --no-secondary --steps %d --warmup %d` (hipGraph replay): "
                             "family TotalDurationNs / Calls over %d dispatches; algorithmic flops / bytes per launch from the eager pass" % (a.steps, a.warmup, ktrace[fam][1]))
                fam_ms[fam] = ms / a.steps
                tfl, gbs = fl / (ms * 1e-3) / 1e12, nb / (ms * 1e-3) / 1e9
                subs = FAMS[fam][1]
                traffic, traffic_src = None, None
                if fam in pmc:
                    traffic = pmc[fam][0]
                    traffic_src = ("measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, --kernel-trace only) over `bench.py --no-graph --steps 2`, "
                                   "%d dispatches per pass, 2*FETCH_SIZE + WRITE_SIZE per launch (KiB units, gfx950 FETCH correction)" % pmc[fam][1])
                elif pname is not None:
                    meta = json.load(open(os.path.join(pdir, pname)))
                    ks = {k_: v for k_, v in meta["kernels"].items() if any(s_ in k_ for s_ in subs)}
                    disp = sum(v["dispatches"] for v in ks.values())
                    if disp:
                        traffic = round(sum(v["hbm_bytes_per_launch"] * v["dispatches"] for v in ks.values()) / disp)
                        traffic_src = ("profiles/" + pname + ": rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes of `bench.py --no-graph` at commit " + str(meta.get("commit", "?"))
                                       + " (2*FETCH_SIZE + WRITE_SIZE per launch, gfx950 correction applied); not re-measured in this run -- " + str(why))
                common = {"traffic": traffic, "traffic_unit": "bytes/launch", "traffic_source": traffic_src if traffic is not None else str(why),
                          "algorithmic_bytes_per_launch": round(nb / n), "launches": n, "launches_per_step": n // a.steps, "ms_per_step": round(ms / a.steps, 3),
                          "avg_launch_us": round(1000 * ms / n, 2), "avg_launch_us_hip_events": round(1000 * ms_events / n, 2),
                          "avg_gflop_per_launch": round(fl / n / 1e9, 3), "timed": timed if fam in ktrace else timed + " (" + str(why_kt) + ")"}
                # which roofline bounds the family: flop per algorithmic byte against the ridge (dense bf16 MFMA peak / HBM peak = 312)
                bound = "hbm" if fam == "hbm" or (fam == "generic" and fl / max(nb, 1) < PEAK_BF16_TFLOPS * 1e3 / PEAK_HBM_GBS) else "mfma"
                if bound == "hbm":
                    entries[fam] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 5),
                                    "kernel": KERNEL_TEXT[fam], "tflops": round(tfl, 2), "mfma_frac": round(tfl / PEAK_BF16_TFLOPS, 5), "flop_per_byte": round(fl / max(nb, 1), 1)}
                else:
                    entries[fam] = {"bound": "mfma", "achieved": round(tfl, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tfl / PEAK_BF16_TFLOPS, 5),
                                    "kernel": KERNEL_TEXT[fam], "algorithmic_gbs": round(gbs, 1), "flop_per_byte": round(fl / max(nb, 1), 1)}
                entries[fam].update(common)
            if entries:
                NAME = {"generic": "gemm_kernel<64,64,64>", "hbm": "panel2_kernel", "mfma": "gemm128_kernel"}
                top = max(fam_ms, key=fam_ms.get)
                res["roofline"] = dict(entries[top], why_this_kernel="largest summed time per step among the three timed GEMM families in this run: " +
                                       ", ".join("%s %.2f ms/step" % (NAME[f_], v) for f_, v in sorted(fam_ms.items(), key=lambda kv: -kv[1])))
                for fam, ent in entries.items():
                    res["roofline_" + fam] = ent
        elif prof is not None and prof["records"]:
            tot_ms = sum(r[0].elapsed_time(r[1]) for r in prof["records"])
            tot_fl = sum(r[2] for r in prof["records"])
            n = len(prof["records"])
            per_key = {}
            for e0, e1, fl, key, shape, nbytes in prof["records"]:
                k_ = per_key.setdefault(str(key), [0.0, 0.0, 0])
                k_[0] += e0.elapsed_time(e1)
                k_[1] += fl
                k_[2] += 1
            ach = tot_fl / (tot_ms * 1e-3) / 1e12
            res["roofline"] = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 5),
                               "kernel": "all gemm launches", "traffic": None, "launches": n, "avg_launch_us": round(1000 * tot_ms / n, 2),
                               "avg_gflop_per_launch": round(tot_fl / n / 1e9, 3)}
            if a.profile_all:
                shapes = {}
                for e0, e1, fl, key, shape, nbytes in prof["records"]:
                    s_ = shapes.setdefault(str(key) + str(shape), [0.0, 0.0, 0, nbytes])
                    s_[0] += e0.elapsed_time(e1)
                    s_[1] += fl
                    s_[2] += 1
                rows = sorted(shapes.items(), key=lambda kv: -kv[1][0])
                os.makedirs("gpurun_out", exist_ok=True)
                with open("gpurun_out/gemm_shapes.txt", "w") as f:
                    f.write("# (tile,a_kind,b_kind)(M,N,K,batch,split,taps)  ms/step  launches/step  us/launch  TFLOP/s  GB/s(algorithmic)  t_mfma_us  t_hbm_us\n")
                    for name, (ms, fl, cnt, nb) in rows:
                        us = 1000 * ms / cnt
                        f.write("%-60s %8.3f %4d %9.1f %8.1f %8.0f %8.1f %8.1f\n" % (name, ms / a.steps, cnt // a.steps, us, fl / cnt / us / 1e6,
                                                                                 nb / us / 1e3, fl / cnt / 2.5e9, nb / 6.3e6))
                res["roofline"]["per_variant"] = {k_: {"ms_per_step": round(v[0] / a.steps, 3), "tflops": round(v[1] / (v[0] * 1e-3) / 1e12, 1),
                                                      "launches_per_step": v[2] // a.steps} for k_, v in per_key.items()}
        if not a.no_cpu_baseline and world == 1:
            # matcher index bit-match (the second half of the metric): the 6-layer outputs of one more step and the
            # HIP assignment on them go to the CPU child, which re-matches them with the oracle and counts differing (layer, image) pairs
            check_path = None
            try:
                import tempfile
                import numpy as np
                # every resident batch (4 x 8 images x 6 layers = 192 (layer, image) pairs with the default settings), one forward + criterion each
                batches = [(p_[0], p_[1], p_[3], p_[4]) for p_ in pool] if dynamic else [(samples.tensors, tok["input_ids"], targets, pmap)]
                arrays = {"nb": np.array(len(batches))}
                for bi, (img, ids, t_i, pm_i) in enumerate(batches):
                    samples.tensors.copy_(img)
                    tok["input_ids"].copy_(ids)
                    t_dev = [{k_: (v.to(dev) if torch.is_tensor(v) else v) for k_, v in t.items()} for t in t_i]
                    with torch.no_grad():
                        mc = model(samples, tok, encode_and_save=True)
                        out = model(samples, tok, encode_and_save=False, memory_cache=mc)
                        criterion(mc, out, t_dev, pm_i.to(dev), None)
                    m = criterion.last_match
                    m.check()
                    st = out["_stacked"]
                    arrays.update({f"logits{bi}": st["pred_logits"].float().cpu().numpy(), f"boxes{bi}": st["pred_boxes"].float().cpu().numpy(),
                                   f"pm{bi}": pm_i.float().cpu().numpy(), f"sizes{bi}": np.array(m.sizes),
                                   f"tgt_boxes{bi}": (m.tgt_boxes.cpu().numpy() if m.tgt_boxes is not None else np.zeros((0, 4), np.float32)),
                                   f"src{bi}": m.src.cpu().numpy(), f"tgt{bi}": m.tgt.cpu().numpy()})
                check_path = os.path.join(tempfile.mkdtemp(prefix="toist_bench_"), "match.npz")
                np.savez(check_path, **arrays)
            except Exception as e:  # the throughput line must survive a failing check; the field then says why
                res["matcher_mismatch_images"] = f"not checked: {type(e).__name__}: {e}"
            cb = cpu_baseline(a.size, check_path)
            if "matcher_mismatch_images" in cb:
                res["matcher_mismatch_images"] = cb.pop("matcher_mismatch_images")
                res["matcher_checked_layer_image_pairs"] = cb.pop("matcher_checked")
            res["cpu_baseline"] = cb
        if world == 1 and not a.no_secondary and not a.masks and not a.no_cpu_baseline and use_graph:
            # the other single-GPU configurations of BASELINE.json, short runs in child processes (time-boxed like cpu_baseline): the driver
            # runs `bench.py --gpus 1` once, so this is where configs[2] / configs[4] get a driver-witnessed number
            del model, criterion, opt
            torch.cuda.empty_cache()
            res["secondary"] = secondary_legs()
        print(json.dumps(res))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
