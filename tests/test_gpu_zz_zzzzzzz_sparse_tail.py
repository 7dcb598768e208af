"""Row-sparse gradient slots and the optimizer tail that honours them (csrc/rows.hip: embed_bwd_kernel's touched bytes, sparse_clear_kernel;
csrc/optim.hip: the touched / hot tables of sqnorm_kernel and adamw_ema_kernel; engine.ParamSet, optim.FusedClipAdamWEMA, parallel).

Everything here is bit for bit: the yardstick is the dense path through the entry points that were there before (toist_embed_bwd on a zeroed
buffer, toist_opt_sqnorm, toist_opt_adamw_ema[_blocks]), compared on .view(torch.int32) so that NaN positions compare too.  No tolerance
anywhere.  (The file sorts behind every other GPU test file and builds no model and no captured step: DESIGN.md section 8 item 6.)"""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 8192            # toist_opt_chunk_elems()
PAD = 1             # the padding id: that row never receives a gradient
N_TOK = 8

# (rows, columns, offset in floats of the table inside its allocation)
#   43 x 768    row 10 straddles chunks 0 / 1; row 31 ends exactly at 3 C and must not flag chunk 3; the last chunk has 256 elements
#   3000 x 6    row 1365 straddles chunks 0 / 1
#   3 x 20000   one row spans several chunks
#   43 x 768 at an offset of one float: the scalar paths of every kernel
TABLES = {"43x768": (43, 768, 0), "3000x6": (3000, 6, 0), "3x20000": (3, 20000, 0), "43x768+1": (43, 768, 1)}
# the six steps: rows {0, a, b}; nothing; a row in the last, partly filled chunk; an old row again; duplicate ids; nothing
ROWS = {"43x768": ([0, 10, 31], [], [42], [10], [5, 5, 7, 5, 7], []),
        "3000x6": ([0, 1365, 31], [], [2999], [1365], [5, 5, 7, 5, 7], []),
        "3x20000": ([0], [], [2], [0], [2, 2, 0, 2], []),
        "43x768+1": ([0, 10, 31], [], [42], [10], [5, 5, 7, 5, 7], [])}
DENSE_N = C + 5     # the ordinary tensor beside the table: one full chunk and a scalar tail


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().contiguous().view(torch.int16) if t.dtype == torch.bfloat16 \
        else t.detach()


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _host_chunks(rows, D, n_chunks):
    """the chunks the rows overlap, computed on the host"""
    want = torch.zeros(n_chunks, dtype=torch.uint8)
    for r in rows:
        if r != PAD:
            want[r * D // C:((r + 1) * D - 1) // C + 1] = 1
    return want


def _ids(rows):
    ids = torch.full((N_TOK,), PAD, dtype=torch.int64)
    ids[:len(rows)] = torch.tensor(rows, dtype=torch.int64) if rows else ids[:0]
    return ids


class _Run:
    """One table (with EMA and bf16 compute copy) and one dense tensor (with EMA) under FusedClipAdamWEMA.  sparse=False: the yardstick -- the
    gradient buffer is zeroed in full and written by toist_embed_bwd, the tail runs through the dense entry points.  sparse=True: the buffer is
    a registered row-sparse slot, cleared by toist_sparse_clear and written by toist_embed_bwd_sparse."""

    def __init__(self, dev, table, sparse, late=False, **opt_kw):
        from toist_amd import engine, optim
        R, D, off = TABLES[table]
        gen = torch.Generator().manual_seed(5)
        self.dev, self.R, self.D, self.sparse, self.late = dev, R, D, sparse, late
        n = R * D
        self.n_chunks = (n + C - 1) // C
        self.table = torch.nn.Parameter(torch.zeros(n + 4, device=dev)[off:off + n].view(R, D).copy_(torch.randn(R, D, generator=gen)))
        self.dense = torch.nn.Parameter(torch.randn(DENSE_N, generator=gen).to(dev))
        self.emas = [self.table.detach().clone(), self.dense.detach().clone()]
        self.cache = {}
        self.w = engine.compute_copy(self.table, engine._cast_bf16, self.cache, "table")
        self.grad = torch.zeros(n + 4, device=dev)[off:off + n].view(R, D)
        self.touched = torch.zeros(self.n_chunks, dtype=torch.uint8, device=dev) if sparse else None
        if sparse:
            engine.register_touched(self.grad, self.touched)
        self.ids = torch.full((N_TOK,), PAD, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(N_TOK, dtype=torch.int64, device=dev)
        self.tok_grad = torch.zeros(N_TOK, D, dtype=torch.bfloat16, device=dev)
        self.dense_grad = torch.zeros(DENSE_N, device=dev)
        groups = [{"params": [self.table], "lr": 3e-3, "late": late}, {"params": [self.dense], "lr": 1e-3}]
        kw = dict(lr=1e-4, weight_decay=1e-2, max_norm=0.1, ema_decay=0.99)
        kw.update(opt_kw)
        self.opt = optim.FusedClipAdamWEMA(groups, ema=list(zip([self.table, self.dense], self.emas)), **kw)
        self.opt._sparse = sparse
        self.table.grad, self.dense.grad = self.grad, self.dense_grad

    def feed(self, step, rows, nan=False):
        """the inputs of one step into the fixed buffers"""
        gen = torch.Generator().manual_seed(100 + step)
        self.ids.copy_(_ids(rows))
        self.tok_grad.copy_(torch.randn(N_TOK, self.D, generator=gen).to(torch.bfloat16))
        dg = torch.randn(DENSE_N, generator=gen) * (3.0 if step % 2 else 1e-3)
        if nan:
            dg[C + 2] = float("nan")
        self.dense_grad.copy_(dg)

    def backward(self):
        from toist_amd import kernels as k
        if self.sparse:
            k.sparse_clear([(self.grad, self.touched)], C)
            k.embed_bwd_sparse(self.tok_grad, self.ids, self.pos, PAD, self.grad, None, None, self.touched, None, C)
        else:
            self.grad.zero_()
            k.embed_bwd(self.tok_grad, self.ids, self.pos, PAD, self.grad, None, None)

    def step(self):
        self.backward()
        self.opt.step()
        if self.late:
            self.opt.flush_late()

    def tensors(self):
        o = self.opt
        return {"p": self.table, "p_dense": self.dense, "m": o.exp_avg[0], "m_dense": o.exp_avg[1], "v": o.exp_avg_sq[0], "v_dense": o.exp_avg_sq[1],
                "ema": self.emas[0], "ema_dense": self.emas[1], "w": self.w, "partial": o._partial, "state": o.state, "grad": self.grad}

    def hot(self):
        return self.opt.hot_chunks(0).cpu()

    def hot_exact(self):
        """the chunks of the table that hold a moment whose bit pattern is not +0"""
        o = self.opt
        nz = (_bits(o.exp_avg[0]).view(-1) != 0) | (_bits(o.exp_avg_sq[0]).view(-1) != 0)
        nz = torch.cat([nz, nz.new_zeros((-nz.numel()) % C)])
        return nz.view(-1, C).any(dim=1).to(torch.uint8).cpu()


def _compare(a, b, where):
    torch.cuda.synchronize()
    ta, tb = a.tensors(), b.tensors()
    bad = [n for n in ta if not _same(ta[n], tb[n])]
    assert not bad, f"{where}: sparse and dense runs differ in {bad}"


def _six_steps(dev, table, nan_at=None, guarded=False, **kw):
    sp, de = _Run(dev, table, True, skip_nonfinite=guarded, **kw), _Run(dev, table, False, skip_nonfinite=guarded, **kw)
    for s, rows in enumerate(ROWS[table], start=1):
        nan = s == nan_at
        before = {n: t.clone() for n, t in sp.tensors().items() if n not in ("partial", "state", "grad")} if nan and guarded else None
        hot_before = sp.hot()
        for r in (sp, de):
            r.feed(s, rows, nan=nan)
            r.step()
        _compare(sp, de, f"{table} step {s}")
        torch.cuda.synchronize()
        assert torch.equal(sp.touched.cpu(), _host_chunks(rows, sp.D, sp.n_chunks)), f"{table} step {s}: touched bytes"
        hot, exact = sp.hot(), sp.hot_exact()
        assert bool((hot >= exact).all()), f"{table} step {s}: a chunk with a non-zero moment is not hot"
        if s <= 2:                      # (the rows of the first step leave chunks out in every table: those took the cold path)
            assert int(hot.sum()) < sp.n_chunks, f"{table} step {s}: every chunk is hot, the cold path never ran"
        if before is not None:          # a skipped step changes no byte, hot included
            now = sp.tensors()
            assert sp.opt.device_state()["skipped"] and all(_same(now[n], before[n]) for n in before) and torch.equal(hot, hot_before)
    assert torch.equal(sp.hot(), sp.hot_exact()), f"{table}: hot is not exactly the chunks with a non-zero moment"
    return sp, de


@pytest.mark.parametrize("table", list(TABLES))
def test_sparse_tail_equals_dense_tail(dev, table):
    sp, de = _six_steps(dev, table)
    assert sp.opt.device_state()["step"] == 6 == de.opt.device_state()["step"]
    if table.startswith("43x768"):
        # the dense run holds the oracle's values (tolerances of tests/test_gpu_optim.py: fp32 in another association order)
        from oracle import optim_ref
        ref = _Run(dev, table, False)
        p, m, v, e = ([x.detach().cpu().clone() for x in (ref.table, ref.dense)], [torch.zeros(43, 768), torch.zeros(DENSE_N)],
                      [torch.zeros(43, 768), torch.zeros(DENSE_N)], [x.cpu().clone() for x in ref.emas])
        for s, rows in enumerate(ROWS[table], start=1):
            ref.feed(s, rows)
            ref.backward()
            torch.cuda.synchronize()
            grads = [ref.grad.cpu().clone(), ref.dense_grad.cpu().clone()]
            p, m, v, e, _ = optim_ref.tail_step(p, grads, m, v, [0, 1], [(3e-3, 1e-2), (1e-3, 1e-2)], s, 0.1, emas=e, ema_decay=0.99)
        torch.testing.assert_close(sp.table.detach().cpu(), p[0], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(sp.opt.exp_avg[0].cpu(), m[0], rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(sp.emas[0].cpu(), e[0], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("variant", ["weight_decay_0", "max_norm_0", "nan_unguarded", "nan_guarded", "slim_launch"])
def test_sparse_tail_variants(dev, variant, monkeypatch):
    from toist_amd import optim
    if variant == "weight_decay_0":
        _six_steps(dev, "43x768", weight_decay=0.0)
    elif variant == "max_norm_0":
        _six_steps(dev, "43x768", max_norm=0.0)
    elif variant == "nan_unguarded":            # the clip coefficient is NaN: everything goes NaN, the never-touched chunks included, identically
        sp, _ = _six_steps(dev, "43x768", nan_at=3)
        assert bool(torch.isnan(sp.table).all()) and bool(torch.isnan(sp.opt.exp_avg[0]).all()) and int(sp.hot().sum()) == sp.n_chunks
    elif variant == "nan_guarded":
        sp, _ = _six_steps(dev, "43x768", nan_at=3, guarded=True)
        assert bool(torch.isfinite(sp.table).all()) and sp.opt.device_state()["step"] == 5
    else:                                       # two workgroups walk the five chunks of the table
        monkeypatch.setattr(optim, "LATE_BLOCKS", 2)
        sp, _ = _six_steps(dev, "43x768", late=True)
        assert sp.opt._n_late == sp.n_chunks > 2


def test_embed_bwd_bytes_and_the_clear(dev):
    from toist_amd import kernels as k
    R, D = 43, 768
    n_chunks = (R * D + C - 1) // C
    gen = torch.Generator().manual_seed(9)
    passes = [[0, 10, 31, 10, PAD, 42, 0, 31], [7, 7, PAD, 20, 41, 7, 3, PAD]]     # duplicates, the padding id, row 0, the last row, rows 10 and 31
    pos = torch.zeros(N_TOK, dtype=torch.int64, device=dev)
    grad = torch.zeros(R, D, device=dev)
    touched = torch.zeros(n_chunks, dtype=torch.uint8, device=dev)
    for i, rows in enumerate(passes):
        ids = torch.tensor(rows, dtype=torch.int64, device=dev)
        tok = torch.randn(N_TOK, D, generator=gen).to(torch.bfloat16).to(dev)
        want = torch.zeros(R, D, device=dev)
        k.embed_bwd(tok, ids, pos, PAD, want, None, None)
        if i:                                   # the second pass lands on the CLEARED buffer: no fill in between
            k.sparse_clear([(grad, touched)], C)
            torch.cuda.synchronize()
            assert int(touched.sum()) == 0 and bool((_bits(grad) == 0).all()), "after the clear the buffer is +0 and every byte is clear"
        k.embed_bwd_sparse(tok, ids, pos, PAD, grad, None, None, touched, None, C)
        torch.cuda.synchronize()
        assert torch.equal(touched.cpu(), _host_chunks(rows, D, n_chunks)), f"pass {i}: bytes"
        assert _same(grad, want), f"pass {i}: gradient"
        assert bool((_bits(grad).view(-1, D)[PAD] == 0).all())
    # both tables in one launch, as the text program issues it: the position table's bytes, and two slots per clear
    R2 = 30
    gpos, tpos = torch.zeros(R2, D, device=dev), torch.zeros((R2 * D + C - 1) // C, dtype=torch.uint8, device=dev)
    grad.zero_()
    touched.zero_()
    ids = torch.tensor(passes[0], dtype=torch.int64, device=dev)
    pid = torch.tensor([2, 3, 4, 5, PAD, 29, 2, 11], dtype=torch.int64, device=dev)
    tok = torch.randn(N_TOK, D, generator=gen).to(torch.bfloat16).to(dev)
    w1, w2 = torch.zeros(R, D, device=dev), torch.zeros(R2, D, device=dev)
    k.embed_bwd(tok, ids, pid, PAD, w1, w2, None)
    k.embed_bwd_sparse(tok, ids, pid, PAD, grad, gpos, None, touched, tpos, C)
    torch.cuda.synchronize()
    assert _same(grad, w1) and _same(gpos, w2)
    assert torch.equal(touched.cpu(), _host_chunks(passes[0], D, n_chunks)) and torch.equal(tpos.cpu(), _host_chunks(pid.tolist(), D, tpos.numel()))
    k.sparse_clear([(grad, touched), (gpos, tpos)], C)
    torch.cuda.synchronize()
    assert int(touched.sum()) == 0 == int(tpos.sum()) and bool((_bits(grad) == 0).all()) and bool((_bits(gpos) == 0).all())


def test_replayed_sparse_step_equals_eager_dense_steps(dev):
    """sparse clear -> embed_bwd -> sqnorm -> finish_norm -> adamw_ema captured once on one stream, replayed four times with other ids in the fixed
    id buffer, against four eager dense steps"""
    table = "43x768"
    sp, de = _Run(dev, table, True), _Run(dev, table, False)
    sp.opt._build_table()
    sp.opt.sync_hyperparams()
    steps = ROWS[table][:4]
    sp.feed(1, steps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sp.step()
    torch.cuda.current_stream().wait_stream(side)
    for s, rows in enumerate(steps, start=1):
        sp.feed(s, rows)
        graph.replay()
        de.feed(s, rows)
        de.step()
        _compare(sp, de, f"replay {s}")
    assert sp.opt.device_state()["step"] == 4
    assert torch.equal(sp.hot(), sp.hot_exact())


def test_checkpoint_recomputes_hot(dev):
    """two steps, state_dict, a fresh optimizer, load_state_dict, two more steps == four uninterrupted dense steps; the recomputed hot bytes are
    the uninterrupted run's"""
    table = "43x768"
    steps = ROWS[table][:4]
    whole_sp, whole_de, first = _Run(dev, table, True), _Run(dev, table, False), _Run(dev, table, True)
    for s, rows in enumerate(steps, start=1):
        for r in (whole_sp, whole_de) + ((first,) if s <= 2 else ()):
            r.feed(s, rows)
            r.step()
    sd = first.opt.state_dict()
    resumed = _Run(dev, table, True)
    with torch.no_grad():
        resumed.table.copy_(first.table)
        resumed.dense.copy_(first.dense)
        for a, b in zip(resumed.emas, first.emas):
            a.copy_(b)
        resumed.w.copy_(first.w)
    resumed.opt.load_state_dict(sd)
    torch.cuda.synchronize()
    assert torch.equal(resumed.hot(), first.hot()) and torch.equal(resumed.hot(), first.hot_exact())
    for s, rows in list(enumerate(steps, start=1))[2:]:
        resumed.feed(s, rows)
        resumed.step()
    _compare(resumed, whole_de, "resumed")
    assert torch.equal(resumed.hot(), whole_sp.hot()) and resumed.opt.device_state()["step"] == 4


TEXT = dict(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, max_position_embeddings=64)


def test_text_program_fp32_only_tables_and_sparse_slots(dev, monkeypatch):
    """The tiny text encoder of tests/test_gpu_train_mode_reference.py.  With the switch on the two embedding tables have no bf16 compute copy and
    row-sparse gradient slots; output and every gradient equal the run with the switch off, bit for bit, also on the second pass over a reused
    gradient buffer (the clear instead of the fill)."""
    import copy
    from toist_amd import engine, transformer
    orig = transformer.roberta_config
    monkeypatch.setattr(transformer, "roberta_config", lambda **kw: orig(**dict(TEXT, **kw)))
    monkeypatch.setattr(engine, "REUSE_GRAD_BUFFERS", True)
    torch.manual_seed(0)
    m_on = transformer.Transformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=512, dropout=0.0).to(dev).eval()
    m_off = copy.deepcopy(m_on)
    gen = torch.Generator().manual_seed(41)
    B, L = 3, 11
    results = {}
    for on, m in ((True, m_on), (False, m_off)):
        monkeypatch.setattr(engine, "SPARSE_TAIL", on)
        outs = []
        g2 = torch.Generator().manual_seed(42)
        for it in range(2):
            ids = torch.randint(2, TEXT["vocab_size"], (B, L), generator=g2)
            att = torch.ones(B, L, dtype=torch.int64)
            att[1, L - 3:] = 0
            ids[1, L - 3:] = PAD
            g_out = torch.randn(B * L, 256, generator=g2).to(torch.bfloat16)
            m.zero_grad(set_to_none=True)
            out, _ = m.encode_text({"input_ids": ids.to(dev), "attention_mask": att.to(dev)})
            (out.float() * g_out.to(dev).float()).sum().backward()
            torch.cuda.synchronize()
            outs.append((out.detach().clone(), {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None}, ids))
        results[on] = outs
    emb = m_on.text_encoder.embeddings
    for q in (emb.word_embeddings.weight, emb.position_embeddings.weight):
        assert engine.copy_of(q) is None and engine.touched_of(q.grad) is not None
    assert engine.copy_of(m_off.text_encoder.embeddings.word_embeddings.weight) is not None
    assert engine.touched_of(m_off.text_encoder.embeddings.word_embeddings.weight.grad) is None
    for it in range(2):
        (o1, g1, ids), (o0, g0, _) = results[True][it], results[False][it]
        assert _same(o1, o0), f"pass {it}: output"
        assert set(g1) == set(g0)
        bad = [n for n in g1 if not _same(g1[n], g0[n])]
        assert not bad, f"pass {it}: gradients differ in {bad}"
    tb = engine.touched_of(emb.word_embeddings.weight.grad).cpu()
    rows = [r for r in results[True][1][2].flatten().tolist()]
    assert torch.equal(tb, _host_chunks(rows, TEXT["hidden_size"], tb.numel()))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from toist_amd import parallel
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    table = "43x768"
    rows_of = {0: ([0, 10], [42]), 1: ([31], [5, 5])}           # other ids on every rank, two steps
    res = {}
    for sparse in (True, False):
        r = _Run(dev, table, sparse)
        for s in range(2):
            r.feed(10 * rank + s + 1, rows_of[rank][s])
            r.backward()
            parallel.all_reduce_mean([r.grad, r.dense_grad])        # reduces the touched bytes of r.grad with MAX beside it
            r.opt.step()
        torch.cuda.synchronize()
        res[sparse] = {n: t.detach().cpu().clone() for n, t in r.tensors().items()}
        if sparse:
            res["touched"] = r.touched.cpu().clone()
    gathered = [None] * world
    dist.all_gather_object(gathered, res[True])
    out[rank] = {"same_as_dense": [n for n in res[True] if not _same(res[True][n], res[False][n])],
                 "same_on_ranks": [n for n in res[True] if not _same(gathered[0][n], gathered[1][n])],
                 "touched": res["touched"].tolist()}
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reduce_the_touched_bytes(dev):
    import torch.multiprocessing as mp
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(world, _free_port(), out), nprocs=world, join=True)
    want = _host_chunks([42, 5], 768, 5).tolist()      # the second step: the union of both ranks' rows
    for r in range(world):
        assert out[r]["same_as_dense"] == [] and out[r]["same_on_ranks"] == [], out[r]
        assert out[r]["touched"] == want, out[r]
