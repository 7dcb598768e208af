"""Task-sweep inference on one MI355X: T = 14 captions over batches of B = 8 synthetic 640 x 640 images (P = 112 (image, caption) pairs per image
batch, 16-token captions, detection model), four ways, in (image, task) pairs per second:
  a  per_pair_captured   what a user does today: 14 CapturedEvalStep(batch=8) replays per image batch (one per caption; ResNet and RoBERTa run 14 times)
  b  per_pair_eager      the eager per-pair body, 14 times per image batch: encode -> decode -> PostProcess -> status check
  c  sweep_eager         harness.evaluate_sweep: one image pass per image, one text pass per caption for the whole region, one pair stage of P = 112
  d  sweep_captured      CapturedSweepStep(batch=8, captions=14): one upload + one graph launch + status check per image batch
(+ c with max_pairs = 8: one pair stage per caption, the shapes of the per-pair body.)
Every leg is warmed on every shape it uses; a timed region is `--steps` image batches (a different batch every step) on a host clock and ends in a
device synchronise; the legs alternate inside one process and the figure of a leg is the median of its `--repeats` regions.  Also measured:
the toist_sweep_assemble launch alone at the workload's shape (HIP events) against its traffic floor, the kernel launches per image batch of every leg
(torch.profiler on eager passes, after the timings), and how far the results of (c) and (d) are from those of (b).
Prints ONE JSON line and writes it to profiles/task_sweep.json; --parity FILE merges the measured oracle errors the test suite wrote out
(task_sweep_parity.json of tests/test_gpu_zz_task_sweep.py) into it.
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


def assemble_alone(dev, B, T, HW, L, D, iters=50):
    """The assemble launch at the workload's shape: the mean of `iters` launches between two HIP events, against the bytes it must move."""
    from toist_amd import kernels as k
    from toist_amd.sweep import pair_tables
    g = torch.Generator().manual_seed(0)
    img_tok, img_pos = (torch.randn(B, HW, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    txt_tok = torch.randn(T, L, D, generator=g).to(torch.bfloat16).to(dev)
    img_pad, txt_pad = torch.zeros(B, HW, dtype=torch.uint8, device=dev), torch.zeros(T, L, dtype=torch.uint8, device=dev)
    pi, pc, P = pair_tables(B, T)
    pi, pc = pi.to(dev), pc.to(dev)
    out = k.sweep_assemble(img_tok, img_pos, img_pad, txt_tok, txt_pad, pi, pc)
    for _ in range(5):
        k.sweep_assemble(img_tok, img_pos, img_pad, txt_tok, txt_pad, pi, pc, out=out, check=False)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        k.sweep_assemble(img_tok, img_pos, img_pad, txt_tok, txt_pad, pi, pc, out=out, check=False)
    b.record()
    torch.cuda.synchronize()
    k.sweep_check()
    ms = a.elapsed_time(b) / iters
    S = HW + L
    written = 2 * P * S * D * 2 + P * S
    read = 2 * P * HW * D * 2 + P * L * D * 2 + P * S + 8 * P               # every source row once per pair (the repeats of an image may come from L2)
    read_unique = 2 * B * HW * D * 2 + T * L * D * 2 + B * HW + T * L + 8 * P
    return {"shape": {"B": B, "T": T, "P": P, "HW": HW, "L": L, "D": D}, "launch_ms": ms, "bytes_written": written, "bytes_read_per_pair": read,
            "bytes_read_unique": read_unique, "traffic_floor_ms": (written + read_unique) / HBM_PEAK * 1e3,
            "traffic_floor_no_reuse_ms": (written + read) / HBM_PEAK * 1e3, "hbm_peak_fraction": (written + read_unique) / (ms * 1e-3) / HBM_PEAK,
            "includes": "launch overhead of back-to-back launches on one stream; HIP events, not a kernel trace"}


def count_kernels(fn):
    """Device kernel launches of one EAGER call of fn(), by torch.profiler; None when the profiler yields nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as e:                                                    # diagnostic only: the timings do not depend on it
        sys.stderr.write(f"bench_task_sweep: kernel count not measured ({type(e).__name__}: {e})\n")
        return None


def run(a):
    import toist_amd
    from toist_amd import harness, kernels as k
    from toist_amd.postprocessors import PostProcess
    from toist_amd.transformer import TokenizedText
    dev = torch.device("cuda:0")
    B, T, H, W, L = a.batch, a.captions, a.size, a.size, 16
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cuda"))[0].to(dev).eval()
    post = PostProcess()
    _, captions, _, _ = harness.synthetic_batch(T, 32, 32, tokens=L, seed=77, device=dev, max_targets=0)                 # the T captions of the evaluation
    per_caption = [TokenizedText({"input_ids": captions["input_ids"][t:t + 1].expand(B, L).contiguous(),
                                  "attention_mask": captions["attention_mask"][t:t + 1].expand(B, L).contiguous()}) for t in range(T)]
    batches = [harness.synthetic_batch(B, H, W, tokens=L, seed=900 + i, device=dev, max_targets=0)[0] for i in range(a.steps)]
    orig = [(480, 640)] * B
    orig_dev = torch.tensor(orig, device=dev)
    tasks = [(f"task_{t + 1}", f"caption {t + 1}") for t in range(T)]
    eval_step = harness.CapturedEvalStep(model, batch=B, pad_hw=64)
    sweep_step = harness.CapturedSweepStep(model, batch=B, captions=T, pad_hw=64)
    as_batch = lambda s: {"samples": s, "image_ids": list(range(B)), "orig_sizes": orig}

    def leg_a(samples):
        kept = []
        for t in range(T):
            r = eval_step.step(samples, per_caption[t], orig, [(H, W)] * B)
            kept.append((torch.stack([x["scores"] for x in r]), torch.stack([x["boxes"] for x in r])))       # the next replay overwrites the bucket's buffers
        return kept

    def leg_b(samples):
        out = []
        for t in range(T):
            mc = model(samples, per_caption[t], encode_and_save=True)
            outputs = model(samples, per_caption[t], encode_and_save=False, memory_cache=mc)
            out.append(post(outputs, orig_dev))
            k.xdec_check()
        return out

    def leg_c(samples_list, max_pairs=None):
        return harness.evaluate_sweep(model, post, [as_batch(s) for s in samples_list], tasks, dev, tokenized=captions, max_pairs=max_pairs)

    def leg_d(samples):
        return sweep_step.step(samples, captions, orig)

    def region(fn, whole=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if whole:
            fn(batches)
        else:
            for s in batches:
                fn(s)
        torch.cuda.synchronize()
        return len(batches) * B * T / (time.perf_counter() - t0)

    legs = {"a_per_pair_captured": (leg_a, False), "b_per_pair_eager": (leg_b, False), "c_sweep_eager": (leg_c, True),
            "c_sweep_eager_max_pairs_8": (lambda bs: leg_c(bs, max_pairs=B), True), "d_sweep_captured": (leg_d, False)}
    rates = {name: [] for name in legs}
    with torch.no_grad():
        for name, (fn, whole) in legs.items():                    # every shape of every leg, before any clock starts
            for _ in range(a.warmup):
                fn(batches[:1]) if whole else fn(batches[0])
        torch.cuda.synchronize()
        for _ in range(a.repeats):                                # alternated: the legs share whatever else the host is doing
            for name, (fn, whole) in legs.items():
                rates[name].append(region(fn, whole))
                sys.stderr.write(f"bench_task_sweep: {name} {rates[name][-1]:.1f} pairs/s\n")
                sys.stderr.flush()
        # the same answers: per (image, task), the sweeps against the eager per-pair body on one batch
        want = leg_b(batches[0])
        got_c = leg_c(batches[:1])
        got_c8 = leg_c(batches[:1], max_pairs=B)                 # pair stages of B pairs: the shapes of the per-pair body
        res_d, pi, pc, live = leg_d(batches[0])
        diff = {name: {"scores": 0.0, "boxes": 0.0} for name in ("c", "c_max_pairs_8", "d")}
        for p in range(live):
            i, t = int(pi[p]), int(pc[p])
            for name, r in (("c", got_c[(i, tasks[t][0])]), ("c_max_pairs_8", got_c8[(i, tasks[t][0])]), ("d", res_d[p])):
                for k_ in ("scores", "boxes"):
                    diff[name][k_] = max(diff[name][k_], float((r[k_] - want[t][i][k_]).abs().max()))
    HW = (H // 32) * (W // 32)
    out = {"tool": "tools/bench_task_sweep.py", "device": "MI355X",
           "workload": {"images_per_batch": B, "captions": T, "pairs_per_image_batch": B * T, "image_hw": [H, W], "tokens": L, "queries": 100,
                        "image_batches_per_region": a.steps, "repeats": a.repeats, "warmup_passes": a.warmup},
           "pairs_per_s": {name: _median(v) for name, v in rates.items()}, "pairs_per_s_all": rates,
           "d_over_a": _median(rates["d_sweep_captured"]) / _median(rates["a_per_pair_captured"]),
           "c_over_b": _median(rates["c_sweep_eager"]) / _median(rates["b_per_pair_eager"]),
           "xdec_in_graph": {"a_per_pair_captured": bool(next(iter(eval_step._buckets.values()))["xdec"]),
                             "d_sweep_captured": bool(next(iter(sweep_step._buckets.values()))["xdec"])},
           "xdec_failed": bool(k.XDEC_FAILED),
           "max_abs_difference_to_per_pair_eager": diff, "difference_units": "scores: probability; boxes: pixels of the 480 x 640 originals",
           "captures": {"a": eval_step.captures, "d": sweep_step.captures}, "replays": {"a": eval_step.replays, "d": sweep_step.replays},
           "assemble": assemble_alone(dev, B, T, HW, L, 256)}

    # launches per image batch, in a pass of its own (a profiler slows the host).  The eager legs are counted as they run; a captured leg replays the
    # launch sequence of its eager first pass, which is what is counted for it -- no profiler is attached to a graph replay.
    def twin_a(samples):
        for t in range(T):
            mc = model(samples, per_caption[t], encode_and_save=True)
            outputs = model(samples, per_caption[t], encode_and_save=False, memory_cache=mc)
            k.postprocess(outputs["pred_logits"], outputs["pred_boxes"], orig_dev)

    def twin_d(samples):
        state, text = model.sweep_stages(samples, captions)
        outputs = model.decode(model.sweep_pairs(state, text, pi, pc))
        k.postprocess(outputs["pred_logits"], outputs["pred_boxes"], orig_dev[pi.long().to(dev)])

    def counts():
        with torch.no_grad():
            return {"a_per_pair_captured (its eager first pass)": count_kernels(lambda: twin_a(batches[0])), "b_per_pair_eager": count_kernels(lambda: leg_b(batches[0])),
                    "c_sweep_eager (text stage included)": count_kernels(lambda: leg_c(batches[:1])),
                    "d_sweep_captured (its eager first pass)": count_kernels(lambda: twin_d(batches[0]))}
    return out, counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--captions", type=int, default=14)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=30, help="image batches per timed region")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-count", action="store_true", help="skip the torch.profiler pass that counts kernel launches")
    ap.add_argument("--parity", default=None, help="task_sweep_parity.json as the test suite wrote it: its measured oracle errors are merged into the output")
    ap.add_argument("--out", default=os.path.join("profiles", "task_sweep.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_task_sweep: no GPU; nothing is measured without one")

    def rnd(v):
        if isinstance(v, float):
            return round(v, 3) if abs(v) >= 1 else float(f"{v:.3g}")
        if isinstance(v, list):
            return [rnd(x) for x in v]
        if isinstance(v, dict):
            return {k_: rnd(x) for k_, x in v.items()}
        return v

    out, counts = run(a)
    out = rnd(out)
    if a.parity and os.path.exists(a.parity):
        with open(a.parity) as f:
            out["oracle_parity"] = json.load(f)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)

    def write():
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")

    out["kernel_launches_per_image_batch"] = "not measured"
    write()                                                   # the timings are safe before the profiler pass starts
    if not a.no_count:
        out["kernel_launches_per_image_batch"] = {name: (n if n is not None else "not measured") for name, n in counts().items()}
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
