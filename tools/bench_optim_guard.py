#!/usr/bin/env python
"""Cost of the optimizer tail's non-finite guard (FusedClipAdamWEMA(skip_nonfinite=True)) at full model size.

Builds the default model (~185 M parameters), the three parameter groups of bench.py, max_norm = 0.1 and the EMA, gives every parameter a fixed
random gradient, and times the tail's three launches (sqnorm, finish_norm, adamw_ema) with device events: each launch on its own and the three
together, as medians of --repeats timed repeats after --warmup untimed ones.  `--guard off` times the plain finish_norm (it also runs on a tree that
predates the option: compare against the parent commit in the same GPU visit), `--guard on` the guarded one with two veto words registered, as a
captured training step has them (the loss word and the decoder status word).  One JSON line on stdout.

    python tools/bench_optim_guard.py --guard off --repeats 30
    python tools/bench_optim_guard.py --guard on  --repeats 30
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guard", choices=("off", "on"), default="off")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default=None, help="copied into the result line")
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("--repeats: at least 20 timed repeats")

    import torch
    import toist_amd
    from toist_amd import harness
    from toist_amd import kernels as k
    from toist_amd.optim import FusedClipAdamWEMA
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_guard needs the GPU: a CPU run cannot time the tail")
    dev = torch.device("cuda:0")
    args = harness.default_args(device="cuda")
    torch.manual_seed(0)
    model, _, _, _ = toist_amd.build_model(args)
    model.to(dev).train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if "backbone" not in n and "text_encoder" not in n]},
              {"params": [p for n, p in named if "backbone" in n], "lr": args.lr_backbone},
              {"params": [p for n, p in named if "text_encoder" in n], "lr": args.text_encoder_lr}]
    src = [v for v in model.state_dict().values() if v.is_floating_point()]
    ema = [v.detach().clone() for v in src]
    extra = {"skip_nonfinite": True} if a.guard == "on" else {}
    opt = FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, ema=list(zip(src, ema)), ema_decay=0.9998,
                            **extra)
    if a.guard == "on":
        opt.add_veto(torch.zeros(1, dtype=torch.float32, device=dev))
        opt.add_veto(torch.zeros(1, dtype=torch.int32, device=dev))
    for _, p in named:
        p.grad = torch.randn_like(p).mul_(1e-3)          # (preserve_format: the parameter's own strides, as the tail requires)
    opt.step()              # a real first step: builds the tables, uploads the gradient pointers
    torch.cuda.synchronize()
    b1, b2 = opt.betas

    def sqnorm():
        k.opt_sqnorm(opt._table, opt._grads_dev, opt._chunks, opt._n_chunks, opt._partial)

    def finish():
        if a.guard == "on":
            k.opt_finish_norm_guarded(opt._partial, opt._n_chunks, opt.max_norm, b1, b2, opt.state, opt._veto_dev[0], len(opt._veto_words[0]),
                                      opt._veto_dev[1], len(opt._veto_words[1]))
        else:
            k.opt_finish_norm(opt._partial, opt._n_chunks, opt.max_norm, b1, b2, opt.state)

    def adamw():
        k.opt_adamw_ema(opt._table, opt._grads_dev, opt._chunks, opt._n_now, opt._groups_dev, opt.state, b1, b2, opt.eps, opt.ema_decay)

    def tail():
        sqnorm()
        finish()
        adamw()

    def timed(fn):
        for _ in range(a.warmup):
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
        times.sort()
        return {"median_us": round(statistics.median(times), 2), "min_us": round(times[0], 2), "max_us": round(times[-1], 2)}

    out = {"tool": "bench_optim_guard", "label": a.label, "guard": a.guard, "parameters": int(sum(p.numel() for _, p in named)), "chunks": int(opt._n_chunks),
           "repeats": a.repeats, "warmup": a.warmup, "tail": timed(tail), "sqnorm": timed(sqnorm), "finish_norm": timed(finish), "adamw_ema": timed(adamw)}
    st = opt.device_state()
    out["steps_applied"] = st["step"]
    out["skipped_total"] = st.get("skipped_total")
    assert all(bool(torch.isfinite(p).all()) for _, p in named[:8])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
