#!/usr/bin/env python
"""The optimizer tail alone on the full-size parameter set: dense against row-sparse, as hipGraph replays interleaved in one process.

Builds the default model (~185 M parameters), the three parameter groups of bench.py, max_norm = 0.1 and the EMA.  Every parameter but RoBERTa's word
and position tables gets a fixed random gradient; the two tables get theirs from the embedding scatter of 8 x 16 token ids drawn uniformly from
[3, 50265), as harness.synthetic_batch draws them, redrawn before every round.  Two graphs over the SAME state:

    dense   zero-fill of both table gradients, toist_embed_bwd, toist_opt_sqnorm, finish_norm, toist_opt_adamw_ema (the tables have their bf16 copy)
    sparse  toist_sparse_clear, toist_embed_bwd_sparse, toist_opt_sqnorm_sparse, finish_norm, toist_opt_adamw_ema_sparse (no bf16 copy of the tables)

Both compute the same update (tests/test_gpu_zz_zzzzzzz_sparse_tail.py), so the rounds may alternate on one state.  Per round each graph is replayed
--replays times between two device events; one JSON line on stdout with the per-replay microseconds of every round and the medians.

    python tools/bench_sparse_tail.py --rounds 9 --replays 20
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    a = ap.parse_args()

    import torch
    import toist_amd
    from toist_amd import engine, harness
    from toist_amd import kernels as k
    from toist_amd.optim import FusedClipAdamWEMA
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_tail needs the GPU: a CPU run cannot time the tail")
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
    opt = FusedClipAdamWEMA(groups, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, ema=list(zip(src, ema)), ema_decay=0.9998)
    emb = model.transformer.text_encoder.embeddings
    word, pos = emb.word_embeddings.weight, emb.position_embeddings.weight
    C = engine.opt_chunk()
    for _, p in named:
        p.grad = torch.zeros_like(p) if p is word or p is pos else torch.randn_like(p).mul_(1e-3)
    touched = [torch.zeros((p.numel() + C - 1) // C, dtype=torch.uint8, device=dev) for p in (word, pos)]
    n_tok, D = 8 * 16, word.shape[1]
    ids = torch.zeros(n_tok, dtype=torch.int64, device=dev)
    pids = (torch.arange(n_tok, dtype=torch.int64, device=dev) % 16) + 2
    tok_grad = torch.randn(n_tok, D, device=dev).mul_(1e-3).to(torch.bfloat16)
    pad = model.transformer.text_encoder.config.pad_token_id
    b1, b2 = opt.betas

    # the dense table: the two tables have a bf16 compute copy, as every 2-D parameter had before the fp32-only declaration
    cache = {}
    for i, p in enumerate((word, pos)):
        engine.compute_copy(p, engine._cast_bf16, cache, "t%d" % i)
    opt._sparse = False
    opt.step()
    dense_table = opt._table.clone()
    for p in (word, pos):
        del engine.COPIES[p.data_ptr()]
    engine.COPY_GEN += 1
    for p, t in zip((word, pos), touched):
        p.grad.zero_()
        engine.register_touched(p.grad, t)
    opt._sparse = True
    opt.step()                  # rebuilds the table (no copy of the tables now) and uploads the touched addresses
    torch.cuda.synchronize()
    tch, g = opt._touched_dev(), opt._grads_dev

    def dense():
        word.grad.zero_()
        pos.grad.zero_()
        k.embed_bwd(tok_grad, ids, pids, pad, word.grad, pos.grad, None)
        k.opt_sqnorm(dense_table, g, opt._chunks, opt._n_chunks, opt._partial)
        k.opt_finish_norm(opt._partial, opt._n_chunks, opt.max_norm, b1, b2, opt.state)
        k.opt_adamw_ema(dense_table, g, opt._chunks, opt._n_now, opt._groups_dev, opt.state, b1, b2, opt.eps, opt.ema_decay)

    def sparse():
        k.sparse_clear([(word.grad, touched[0]), (pos.grad, touched[1])], C)
        k.embed_bwd_sparse(tok_grad, ids, pids, pad, word.grad, pos.grad, None, touched[0], touched[1], C)
        k.opt_sqnorm(opt._table, g, opt._chunks, opt._n_chunks, opt._partial, touched=tch)
        k.opt_finish_norm(opt._partial, opt._n_chunks, opt.max_norm, b1, b2, opt.state)
        k.opt_adamw_ema(opt._table, g, opt._chunks, opt._n_now, opt._groups_dev, opt.state, b1, b2, opt.eps, opt.ema_decay, touched=tch, hot=opt._hot_dev)

    touched[0].fill_(1)         # the dense graph does not keep the bytes: the first sparse replay after a dense one clears everything once
    touched[1].fill_(1)
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name, fn in (("dense", dense), ("sparse", sparse)):
            fn()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=side):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    gen = torch.Generator().manual_seed(1)
    rounds = {"dense": [], "sparse": []}
    for r in range(a.rounds):
        ids.copy_(torch.randint(3, word.shape[0], (n_tok,), generator=gen))
        for name in (("dense", "sparse") if r % 2 == 0 else ("sparse", "dense")):
            if name == "sparse":        # the dense replays wrote rows without flagging them: bring the slot back under its invariant, untimed
                touched[0].fill_(1)
                touched[1].fill_(1)
                graphs[name].replay()
            graphs[name].replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                graphs[name].replay()
            e1.record()
            e1.synchronize()
            rounds[name].append(round(e0.elapsed_time(e1) * 1e3 / a.replays, 2))
    med = {n: statistics.median(v) for n, v in rounds.items()}
    hot = opt.hot_chunks([i for i, p in enumerate(opt.params) if p is word][0])
    out = {"tool": "bench_sparse_tail", "parameters": int(sum(p.numel() for _, p in named)), "chunks": int(opt._n_chunks), "rounds": a.rounds, "replays": a.replays,
           "us_per_tail": rounds, "median_us": med, "dense_minus_sparse_us": round(med["dense"] - med["sparse"], 2),
           "dense_spread_us": round(max(rounds["dense"]) - min(rounds["dense"]), 2), "word_table_chunks": int(hot.numel()), "word_table_hot_chunks": int(hot.sum()),
           "steps_applied": opt.device_state()["step"]}
    assert all(bool(torch.isfinite(p).all()) for _, p in named[:8])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
