"""Tensor-level launchers for the C-ABI kernels of libtoist_hip.so.

Every function takes torch tensors that already live on the HIP device, passes raw pointers + sizes
through ctypes on torch's current stream, and returns immediately (no host sync).  torch is used for
memory and streams only.  There is no fallback: a CPU tensor or a missing library raises.
"""
import ctypes
import os

import torch

from . import _lib
from .devcache import DeviceCache, keep
from .folds import FOLDS, _raw_stream
from .knobs import knob
from ._lib import (A_CONV, A_CONVT, A_KROW, A_ROWK, ACT_GELU, ACT_GELU_BWD, ACT_MASK_POS, ACT_NONE, ACT_RELU,
                   ACT_SIGMOID, ACT_SIGMOID_BWD, B_CONVX, B_KROW, B_ROWK, Epilogue, Gemm, Operand)

__all__ = [
    "A_ROWK", "A_KROW", "A_CONV", "A_CONVT", "B_ROWK", "B_KROW", "B_CONVX", "ACT_NONE", "ACT_RELU", "ACT_GELU",
    "ACT_SIGMOID", "ACT_MASK_POS", "ACT_GELU_BWD", "ACT_SIGMOID_BWD", "ConvGeom", "operand", "gemm", "matcher",
    "layernorm_fwd", "layernorm_bwd", "softmax_fwd", "softmax_bwd", "colsum", "add", "dropout", "pack_image", "maxpool3x3s2", "stem_fwd",
    "unpack_nhwc", "sine_position", "embed_fwd", "embed_bwd", "criterion_fwd", "criterion_bwd", "attnmap_softmax_fwd", "attnmap_softmax_bwd",
    "groupnorm_fwd", "groupnorm_apply", "groupnorm_bwd", "upsample_add", "upsample_add_bwd", "sum_queries", "sum_segments", "upsample_add_rows", "mask_stage_fwd", "mask_loss_fwd", "mask_loss_bwd",
]


# bench.py sets this to {"key": (tile, a_kind, b_kind) | set of such | predicate(key) | None, "records": [], "other": {}} to time GEMM
# launches with HIP events on the launch stream (roofline accounting); None = no instrumentation.
PROFILE = None
# Optional int64[1] device tensor added to every dropout seed inside the kernels.  A training loop that
# replays a captured hipGraph bumps it once per step so each replay draws fresh dropout masks.
SEED_DEV = None
FORCE_TILE = 0    # experiments: overrides tile == 0 (auto) in every gemm() call
FORCE_SPLIT = 0   # experiments: overrides split_k when > 0 and the call accumulates
DEBUG_FLAGS = 0   # experiments: extra flag bits (ablation switches of the PROF kernels) when DEBUG_WS is set
DEBUG_WS = None   # experiments: f32 device buffer handed to un-split gemm() calls as `workspace` with flags bit 11 (per-phase cycle counters of panel2_kernel)


_WS = {}


def _workspace(elems, device):
    """Caller-owned split-K scratch handed to the library (grown on demand, reused across calls)."""
    key = (device, _raw_stream())  # one scratch per stream: launches on different streams overlap
    ws = _WS.get(key)
    if ws is None or ws.numel() < elems:
        ws = _WS[key] = torch.empty(max(elems, 1 << 22), dtype=torch.float32, device=device)     # a graph that wrote the old one keeps it
    return keep(ws)


# ---- deferred split-K reductions -----------------------------------------------------------------------------
# A weight-gradient GEMM with few output tiles is cut into k-slices whose fp32 partials land in an arena; with
# defer_reduce=True the fold into the gradient buffer is not launched per GEMM (178 launches of ~6 us per step) but
# queued (toist_amd/folds.py).  The queue must be flushed before anything reads those outputs: engine.Tape.backward() does it at program end.
GEMM_DEFER_REDUCE = _lib.CONSTANTS["TOIST_GEMM_DEFER_REDUCE"]
GEMM_SPLIT_EPILOGUE = _lib.CONSTANTS["TOIST_GEMM_SPLIT_EPILOGUE"]
GEMM_COLSUM_SLICES = _lib.CONSTANTS["TOIST_GEMM_COLSUM_SLICES"]    # a_colsum = [k-slice][M] partials, folded in slice order


def flush_reductions():
    """Fold every queued split-K partial of the current stream into its output (one launch per 48 GEMMs)."""
    FOLDS.flush()


GROUP_MAX = 64


_GROUP_TABLES = DeviceCache(limit=1024)      # (device, rows) -> filled device table


def group_table(rows, device):
    """Device toist_group table from host rows [a_ptr, b_ptr, c_off, rscale_off, colsum_off] (csrc/gemm.hip: the rows travel as kernel
    arguments).  Tables are kept: a training loop presents the same pointers step after step (always under hipGraph replay, nearly
    always with the caching allocator), so the 25 fill launches of a step run once -- a table filled before a capture is simply read
    by the captured launches, which keep it (devcache).  A table needed DURING a capture is filled beside the graph (see below)."""
    key = (str(device), tuple(int(v) for r in rows for v in (list(r) + [0] * (6 - len(r)))))
    return _GROUP_TABLES.get(key, lambda: _fill_group_table(key[1], len(rows), device))


def _fill_group_table(values, n, device):
    flat = (ctypes.c_int64 * (6 * n))(*values)
    if torch.cuda.is_current_stream_capturing() and FILL_TABLES_OUTSIDE_GRAPH:
        # The pointers in `rows` are fixed for the life of the graph being captured, so the table is filled NOW, by a launch on a
        # stream that is not capturing, instead of by a kernel node that would re-write the same 48 bytes per row on every replay
        # (25 launches per training step).  The table must NOT come from the graph's memory pool: a block handed out during a capture
        # may have held an earlier temporary of the same capture, whose producer kernels run again at every replay and would overwrite
        # a table that is no longer re-filled behind them (seen as a memory fault in the first replayed step).  It is carved from an
        # arena allocated before the capture; when the arena is exhausted the fill stays a graph node.
        dev = _arena_table(str(device), n)
        if dev is not None:
            side = _fill_stream(device)
            _lib.check(_lib.lib().toist_group_fill(ctypes.cast(flat, ctypes.c_void_p), n, _p(dev), ctypes.c_void_p(side.cuda_stream)), "toist_group_fill")
            return dev
    dev = torch.empty(n, 6, dtype=torch.int64, device=device)
    _lib.check(_lib.lib().toist_group_fill(ctypes.cast(flat, ctypes.c_void_p), n, _p(dev), _stream()), "toist_group_fill")
    return dev


# Opt-in (harness.CapturedTrainStep, bench.py): whoever captures sets this around the capture and calls sync_table_fills() before the first
# replay -- the fill is not ordered against the graph by any stream dependency (a wait on it cannot be recorded into the capture, and
# synchronising the fill stream during a capture invalidates the capture on ROCm 7.2).  Other captures keep the fill as a graph node.
FILL_TABLES_OUTSIDE_GRAPH = False
_TABLE_ARENAS = {}      # device -> [int64 tensor [rows, 6] allocated outside any capture, rows used]
_TABLE_ARENA_ROWS = 1 << 16     # 3 MB: ~2000 tables of 32 problems
_FILL_STREAMS = {}


def _arena_table(dev_key, n):
    ar = _TABLE_ARENAS.get(dev_key)
    if ar is None or ar[1] + n > ar[0].shape[0]:
        return None
    t = keep(ar[0])[ar[1]:ar[1] + n]       # a graph that took tables from an arena keeps that arena
    ar[1] += n
    return t


def _arena_prepare(device):
    """(outside captures) make sure the table arena of `device` has room for a capture's worth of tables"""
    key = str(device)
    ar = _TABLE_ARENAS.get(key)
    if ar is None or ar[1] + 4096 > ar[0].shape[0]:
        _TABLE_ARENAS[key] = [torch.empty(_TABLE_ARENA_ROWS, 6, dtype=torch.int64, device=device), 0]


def _fill_stream(device):
    s = _FILL_STREAMS.get(str(device))
    if s is None:
        s = torch.cuda.Stream(device=device)
        _FILL_STREAMS[str(device)] = s
    return s


def sync_table_fills():
    """Wait for table fills launched beside a capture (call once after capture_end, before the first replay)."""
    for s in _FILL_STREAMS.values():
        s.synchronize()


class tables_beside_graph:
    """with kernels.tables_beside_graph(): <capture(s)> -- pointer tables of grouped launches are filled once, beside the capture, and
    the fills are joined on exit (TOIST_FILL_OUTSIDE_GRAPH=0 keeps them inside the graph)."""

    def __enter__(self):
        global FILL_TABLES_OUTSIDE_GRAPH
        self.old = FILL_TABLES_OUTSIDE_GRAPH
        FILL_TABLES_OUTSIDE_GRAPH = knob("TOIST_FILL_OUTSIDE_GRAPH", True)
        if FILL_TABLES_OUTSIDE_GRAPH and not torch.cuda.is_current_stream_capturing():
            _arena_prepare(torch.device("cuda", torch.cuda.current_device()))
        return self

    def __exit__(self, *exc):
        global FILL_TABLES_OUTSIDE_GRAPH
        FILL_TABLES_OUTSIDE_GRAPH = self.old
        sync_table_fills()
        return False


def _stream():
    return ctypes.c_void_p(_raw_stream())


def _p(t, dtype=None):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors: no CPU path exists."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("toist_amd kernels need device tensors (got a CPU tensor); there is no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


class ConvGeom:
    """Gather geometry of an implicit-GEMM operand: source [N,SH,SW,SC] NHWC, pixel space [N,PH,PW]."""

    __slots__ = ("SH", "SW", "SC", "PH", "PW", "R", "S", "stride", "pad", "dil")

    def __init__(self, SH, SW, SC, PH, PW, R, S, stride, pad, dil=1):
        self.SH, self.SW, self.SC, self.PH, self.PW = SH, SW, SC, PH, PW
        self.R, self.S, self.stride, self.pad, self.dil = R, S, stride, pad, dil


def operand(t, ld=0, bs_outer=0, bs_inner=0, kin=0, tap_stride=0, geom=None):
    o = Operand()
    o.ptr = _p(t, torch.bfloat16)
    o.ld, o.bs_outer, o.bs_inner, o.kin, o.tap_stride = ld, bs_outer, bs_inner, kin, tap_stride
    if geom is not None:
        o.SH, o.SW, o.SC, o.PH, o.PW = geom.SH, geom.SW, geom.SC, geom.PH, geom.PW
        o.R, o.S, o.stride, o.pad, o.dil = geom.R, geom.S, geom.stride, geom.pad, geom.dil
    return o


def gemm(M, N, K, a_kind, a, b_kind, b, c, ldc, *, batch=1, batch_inner=1, cs_outer=0, cs_inner=0, split_k=1, tile=0,
         flags=0, alpha=1.0, scale=None, shift=None, rscale=None, res=None, ldr=0, aux=None, ldaux=0, act=ACT_NONE, pre_out=None,
         accumulate=False, cmap=None, drop_where=0, drop_p=0.0, drop_seed=0, flops=0, a_colsum=None, res_bcast=None,
         defer_reduce=False, group=None, group_out=None, a2=None, a2_from=0, split_epilogue=False):
    """C = epilogue(A @ B^T); see include/toist_hip.h.  `a`/`b` are Operand structs from operand().
    `flops` = algorithmic FLOPs of the call (bench.py's roofline accounting only)."""
    if tile == 0 and FORCE_TILE:
        tile = FORCE_TILE
    if FORCE_SPLIT and accumulate:
        split_k = FORCE_SPLIT
    d = Gemm()
    d.M, d.N, d.K, d.a_kind, d.b_kind, d.a, d.b = M, N, K, a_kind, b_kind, a, b
    if c.dtype == torch.float32:
        d.epi.out_f32 = 1
    elif c.dtype != torch.bfloat16:
        raise TypeError("gemm output must be bf16 or f32")
    d.c, d.ldc = _p(c), ldc
    d.cs_outer, d.cs_inner, d.batch, d.batch_inner = cs_outer, cs_inner, batch, batch_inner
    d.split_k, d.tile, d.flags = split_k, tile, flags
    e = d.epi
    e.alpha = alpha
    e.scale, e.shift = _p(scale, torch.float32), _p(shift, torch.float32)
    e.rscale = _p(rscale, torch.float32)
    e.res, e.ldr = _p(res, torch.bfloat16), ldr
    e.aux, e.ldaux = _p(aux, torch.bfloat16), ldaux
    e.act = act
    e.pre_out = _p(pre_out, torch.bfloat16)
    e.accumulate = 1 if accumulate else 0
    if cmap is not None:
        e.cmap = 1
        e.cH, e.cW, e.cOH, e.cOW, e.cst = cmap
    if res_bcast is not None:
        e.res_div, e.res_mod = res_bcast
    e.drop_where, e.drop_p, e.drop_seed = drop_where, drop_p, drop_seed
    e.drop_seed_dev = _p(SEED_DEV) if drop_where else None
    d.a_colsum = _p(a_colsum, torch.float32)
    d.group = _p(group, torch.int64)          # [batch, 6] int64 rows (a, b pointers; c, rscale, colsum, shift offsets): toist_group
    if a2 is not None:                        # output columns >= a2_from take their A rows from a2 (packed in_proj on two inputs)
        d.a2, d.a2_from = _p(a2, torch.bfloat16), a2_from
    folds = []      # queued behind the launch: the column sums' fold first, then one per output
    if split_k > 1 and split_epilogue:
        # k-slices folded by a second kernel that applies the complete epilogue (any output type): csrc/gemm.hip splitk_epilogue_kernel
        d.workspace = _p(_workspace(split_k * M * N, c.device), torch.float32)
        d.flags |= GEMM_SPLIT_EPILOGUE
    elif split_k > 1:
        # grouped + split: [problem][k-slice][M][N] partials, one queued fold per problem (group_out = [(c_i, rscale_i)]); else one fold when deferred
        outs = group_out if group is not None else [(c, rscale)] if defer_reduce else ()
        slice_sums = a_colsum is not None and group is None
        # the slices the launch will make, asked once: it sizes the fold arena and the per-slice column sums (neither changes the answer)
        eff = int(_lib.lib().toist_gemm_effective_split(ctypes.byref(d))) if outs or slice_sums else 0
        if outs and eff > 1:
            ws = FOLDS.acquire(eff * M * N * (batch if group is not None else 1), c.device, [ci for ci, _ in outs])
            d.workspace = _p(ws, torch.float32)
            d.flags |= GEMM_DEFER_REDUCE
            folds = [dict(ws=ws.data_ptr() + 4 * i * eff * M * N, out=ci, rscale=ri, splits=eff, M=M, N=N, ldc=ldc, alpha=alpha, accumulate=accumulate)
                     for i, (ci, ri) in enumerate(outs)]
        elif group is not None:
            d.split_k = 1
        else:
            d.workspace = _p(_workspace(split_k * M * N, c.device), torch.float32)
        # the bias gradient of a split-K weight-gradient GEMM: each k-slice stores its column sums in a row of its own and one fold adds
        # the rows in slice order -- float atomics would add them in whatever order the slices finish, a different sum in every run
        if slice_sums and eff > 1 and M % 4 == 0 and a_colsum.data_ptr() % 16 == 0:      # (otherwise: one atomic add per slice, as before)
            cs = torch.empty(eff * M, dtype=torch.float32, device=c.device)      # (not the arena: a take may flush / move it under this GEMM)
            d.a_colsum = cs.data_ptr()
            d.flags |= GEMM_COLSUM_SLICES
            # folded on its own right after this GEMM when the GEMM is not deferred, or when a queued fold already adds into the same bias
            # (two folds of one output must not share a launch); the other queued folds stay batched
            folds.insert(0, dict(ws=cs.data_ptr(), out=a_colsum, splits=eff, M=1, N=M, ldc=M, keep=(cs,),
                                 now=not d.flags & GEMM_DEFER_REDUCE, when_busy="now"))
    if DEBUG_WS is not None and split_k <= 1:
        d.workspace = _p(DEBUG_WS, torch.float32)
        d.flags |= 2048 | DEBUG_FLAGS
    prof, events = PROFILE, None
    if prof is not None:
        if not flops:
            flops = 2 * M * N * K * max(batch, 1)
        t = int(_lib.lib().toist_gemm_pick_tile(ctypes.byref(d)))
        key = (t, a_kind, b_kind)
        want = prof["key"]
        if want is not None and not (want(key) if callable(want) else (key == want or (isinstance(want, (set, frozenset)) and key in want))):
            prof["other"][key] = prof["other"].get(key, 0) + flops
        else:
            events = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            events[0].record()
    _lib.check(_lib.lib().toist_gemm_bf16(ctypes.byref(d), _stream()), "toist_gemm_bf16")
    if events is not None:
        events[1].record()
    for f in folds:
        FOLDS.queue(**f)
    if events is None:
        return
    ta = max(int(a.R) * int(a.S), 1) if a_kind in (A_CONV, A_CONVT) else 1
    tb = max(int(b.R) * int(b.S), 1) if b_kind == B_CONVX else 1
    nb = max(batch, 1)
    nbytes = 2 * M * K * nb // ta + 2 * N * K * nb // tb + (4 if c.dtype == torch.float32 else 2) * M * N * nb
    nbytes += 2 * M * N * nb * ((res is not None) + (aux is not None) + (pre_out is not None))
    prof["records"].append((*events, flops, key, (M, N, K, nb, split_k, ta * tb), nbytes))


class ConvPair(ctypes.Structure):
    """toist_conv_pair (include/toist_hip.h); tests/test_cpu_conv_pair_check.py holds every field against the C compiler"""
    _fields_ = [("M", ctypes.c_int32), ("C", ctypes.c_int32), ("dgrad", ctypes.c_int32), ("lda", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("a", "w_first", "w_second", "shift_mid", "shift_out", "res", "aux_mid", "aux_out", "mid", "out")] + \
               [(n, ctypes.c_int32) for n in ("ldr", "ldaux_mid", "ldaux_out", "ldmid", "ldout", "reserved")]


# conv3 of a layer-3 bottleneck and conv1 of the next one in one launch (csrc/gemm.hip conv_pair_kernel): bit 0 = forward, bit 1 = data
# gradient (conv1 of a block with conv3 of the previous one); 0 = the per-op calls everywhere
CONV_PAIR = knob("TOIST_CONV_PAIR", 3)
CONV_PAIR_CALLS = [0, 0]     # launches so far: forward, data gradient (tests)


def conv_pair(a, w_first, w_second, res, mid, out, *, dgrad=False, shift_mid=None, shift_out=None, aux_mid=None, aux_out=None):
    """mid [M, 1024], out [M, 256] of two chained 1x1 convolutions on the rows of a [M, 256] (see toist_conv_pair in include/toist_hip.h).
    Every tensor is a 2-D bf16 view whose rows are contiguous (stride(1) == 1); weights are contiguous."""
    M, C = a.shape
    for t in (a, res, mid, out, aux_mid, aux_out):
        if t is not None and (t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != M):
            raise ValueError("conv_pair: operands are [M, width] views with contiguous rows")
    if tuple(w_first.shape) != ((C, 4 * C) if dgrad else (4 * C, C)) or tuple(w_second.shape) != ((4 * C, C) if dgrad else (C, 4 * C)) \
            or not (w_first.is_contiguous() and w_second.is_contiguous()):
        raise ValueError("conv_pair: weights are contiguous [4C, C] / [C, 4C] (forward) or [C, 4C] / [4C, C] (data gradient)")
    if tuple(res.shape) != (M, 4 * C) or tuple(mid.shape) != (M, 4 * C) or tuple(out.shape) != (M, C):
        raise ValueError("conv_pair: res / mid are [M, 4C], out is [M, C]")
    d = ConvPair()
    d.M, d.C, d.dgrad, d.lda = M, C, 1 if dgrad else 0, a.stride(0)
    d.a, d.w_first, d.w_second = _p(a, torch.bfloat16), _p(w_first, torch.bfloat16), _p(w_second, torch.bfloat16)
    d.shift_mid, d.shift_out = _p(shift_mid, torch.float32), _p(shift_out, torch.float32)
    d.res, d.ldr = _p(res, torch.bfloat16), res.stride(0)
    d.aux_mid, d.ldaux_mid = _p(aux_mid, torch.bfloat16), aux_mid.stride(0) if aux_mid is not None else 0
    d.aux_out, d.ldaux_out = _p(aux_out, torch.bfloat16), aux_out.stride(0) if aux_out is not None else 0
    d.mid, d.ldmid, d.out, d.ldout = _p(mid, torch.bfloat16), mid.stride(0), _p(out, torch.bfloat16), out.stride(0)
    CONV_PAIR_CALLS[1 if dgrad else 0] += 1
    _lib.check(_lib.lib().toist_conv_pair_bf16(ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), _stream()), "toist_conv_pair_bf16")


def matcher(logits, boxes, tgt_boxes, pos_map, tgt_off, match_off, max_T, w_class, w_bbox, w_giou, src_idx, tgt_idx,
            status, cost_out=None):
    L, B, Q, K = logits.shape
    _lib.check(
        _lib.lib().toist_matcher(_p(logits, torch.float32), _p(boxes, torch.float32), _p(tgt_boxes, torch.float32),
                                 _p(pos_map, torch.float32), _p(tgt_off, torch.int32), _p(match_off, torch.int32), L, B, Q,
                                 K, max_T, w_class, w_bbox, w_giou, _p(src_idx, torch.int64), _p(tgt_idx, torch.int64),
                                 _p(status, torch.int32), _p(cost_out, torch.float32), _stream()), "toist_matcher")


def layernorm_fwd(x, gamma, beta, eps, y, mean=None, rstd=None, add=None, y2=None):
    rows, D = x.shape
    _lib.check(
        _lib.lib().toist_layernorm_fwd(_p(x, torch.bfloat16), _p(gamma, torch.float32), _p(beta, torch.float32), eps, rows, D,
                                       _p(y, torch.bfloat16), _p(mean, torch.float32), _p(rstd, torch.float32), _p(add, torch.bfloat16),
                                       _p(y2, torch.bfloat16), _stream()),
        "toist_layernorm_fwd")


LN_DEFER = knob("TOIST_LN_DEFER", True)


def _queue_ln_param_grads(blocks, D, dgamma, dbeta):
    """Arena space for two stacked [blocks, D] partial blocks, with their folds into dgamma and dbeta (f32 [D], accumulated) queued."""
    partials = FOLDS.acquire(2 * blocks * D, dgamma.device, (dgamma, dbeta))
    for i, out in enumerate((dgamma, dbeta)):
        FOLDS.queue(partials.data_ptr() + 4 * i * blocks * D, out, blocks, 1, D, D)
    return partials


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma=None, dbeta=None, dx_drop=None, drop_p=0.0, seed=0, defer=False):
    """defer=True: dgamma / dbeta (f32, accumulated) are not updated by contended atomics inside the kernel -- every block writes its
    partial sums to the split-K arena and the fold is queued for flush_reductions() (engine.Tape.backward ends with it)."""
    rows, D = x.shape
    partials, blocks = None, 0
    if defer and LN_DEFER and dgamma is not None:
        blocks = int(_lib.lib().toist_layernorm_bwd_blocks(rows))
        partials = _queue_ln_param_grads(blocks, D, dgamma, dbeta)
    _lib.check(
        _lib.lib().toist_layernorm_bwd(_p(dy, torch.bfloat16), _p(x, torch.bfloat16), _p(mean, torch.float32),
                                       _p(rstd, torch.float32), _p(gamma, torch.float32), rows, D, _p(dx, torch.bfloat16),
                                       None if partials is not None else _p(dgamma, torch.float32),
                                       None if partials is not None else _p(dbeta, torch.float32), _p(dx_drop, torch.bfloat16),
                                       drop_p, seed, _p(SEED_DEV), _p(partials, torch.float32), blocks, _stream()), "toist_layernorm_bwd")


def softmax_fwd(scores, key_pad, nbatch, H, Sq, Sk, ld, p, p_drop=None, drop_p=0.0, seed=0):
    _lib.check(
        _lib.lib().toist_softmax_fwd(_p(scores, torch.bfloat16), _p(key_pad, torch.uint8), nbatch, H, Sq, Sk, ld,
                                     _p(p, torch.bfloat16), _p(p_drop, torch.bfloat16), drop_p, seed, _p(SEED_DEV), _stream()),
        "toist_softmax_fwd")


def softmax_bwd(p, dp, rows, Sk, ld, ds, drop_p=0.0, seed=0):
    _lib.check(
        _lib.lib().toist_softmax_bwd(_p(p, torch.bfloat16), _p(dp, torch.bfloat16), rows, Sk, ld, _p(ds, torch.bfloat16),
                                     drop_p, seed, _p(SEED_DEV), _stream()), "toist_softmax_bwd")


def colsum(g, M, N, ld, out):
    _lib.check(_lib.lib().toist_colsum(_p(g, torch.bfloat16), M, N, ld, _p(out, torch.float32), _stream()), "toist_colsum")


def add(a, b, out, b_period=None):
    n = a.numel()
    _lib.check(
        _lib.lib().toist_add_bf16(_p(a, torch.bfloat16), _p(b, torch.bfloat16), n, n if b_period is None else b_period,
                                  _p(out, torch.bfloat16), _stream()), "toist_add_bf16")


STAMPS = None      # diagnostic (bench.py --stamps): {"buf": int64 device tensor, "names": [...]}: stamp(name) dates a point of the step on its stream


def stamp(name):
    st = STAMPS
    if st is None:
        return
    names = st["names"]
    if name in names:
        idx = names.index(name)
    else:
        idx = len(names)
        if idx >= st["buf"].numel():
            return
        names.append(name)
    _lib.check(_lib.lib().toist_stamp(_p(st["buf"], torch.int64), idx, _stream()), "toist_stamp")


def dropout(x, p, seed, out):
    _lib.check(_lib.lib().toist_dropout_bf16(_p(x, torch.bfloat16), x.numel(), p, seed, _p(SEED_DEV), _p(out, torch.bfloat16), _stream()),
               "toist_dropout_bf16")


def pack_image(nchw, out):
    N, C, H, W = nchw.shape
    _lib.check(_lib.lib().toist_pack_image(_p(nchw, torch.float32), N, C, H, W, _p(out, torch.bfloat16), _stream()), "toist_pack_image")


def stem_fwd(images, w, shift, out):
    """csrc/stem.hip: f32 NCHW images -> conv 7x7/2 (w bf16 [64,7,7,8], BN scale folded) + shift + ReLU + max-pool 3x3/2 -> bf16 NHWC `out`."""
    N, C, H, W = images.shape
    assert tuple(w.shape) == (64, 7, 7, 8) and w.is_contiguous() and images.is_contiguous() and out.is_contiguous()
    _lib.check(_lib.lib().toist_stem_fwd(_p(images, torch.float32), _p(w, torch.bfloat16), _p(shift, torch.float32), N, C, H, W,
                                         _p(out, torch.bfloat16), _stream()), "toist_stem_fwd")


def maxpool3x3s2(x, out):
    N, H, W, C = x.shape
    _lib.check(_lib.lib().toist_maxpool3x3s2(_p(x, torch.bfloat16), N, H, W, C, _p(out, torch.bfloat16), _stream()), "toist_maxpool3x3s2")


def unpack_nhwc(x, out):
    """bf16 [N, HW, C] -> f32 [N, C, HW]"""
    N, HW, C = x.shape
    _lib.check(_lib.lib().toist_unpack_nhwc(_p(x, torch.bfloat16), N, HW, C, _p(out, torch.float32), _stream()), "toist_unpack_nhwc")


def sine_position(mask_u8, num_pos_feats, temperature, out_tok=None, out_nchw=None):
    B, H, W = mask_u8.shape
    _lib.check(_lib.lib().toist_sine_position(_p(mask_u8, torch.uint8), B, H, W, num_pos_feats, temperature, _p(out_tok, torch.bfloat16),
                                              _p(out_nchw, torch.float32), _stream()), "toist_sine_position")


def text_prep(ids, attention_mask, pad_id):
    """-> (position ids int64 [B, L], key_pad uint8 [B, L]) of a tokenized batch"""
    B, L = ids.shape
    pos_ids = torch.empty(B, L, dtype=torch.int64, device=ids.device)
    key_pad = torch.empty(B, L, dtype=torch.uint8, device=ids.device)
    _lib.check(_lib.lib().toist_text_prep(_p(ids, torch.int64), _p(attention_mask, torch.int64), B, L, pad_id, _p(pos_ids), _p(key_pad), _stream()),
               "toist_text_prep")
    return pos_ids, key_pad


def sine_position_seq(mask_u8, num_pos_feats, temperature, out_tok):
    """out_tok bf16 [B, S, 2F], S >= H*W: rows H*W .. S-1 of every image are zero"""
    B, H, W = mask_u8.shape
    _lib.check(_lib.lib().toist_sine_position_seq(_p(mask_u8, torch.uint8), B, H, W, num_pos_feats, temperature, _p(out_tok, torch.bfloat16),
                                                  out_tok.shape[1], _stream()), "toist_sine_position_seq")


def embed_fwd(ids, pos_ids, word, pos, type0, out):
    n, D = out.shape
    _lib.check(_lib.lib().toist_embed_fwd(_p(ids, torch.int64), _p(pos_ids, torch.int64), _p(word, torch.float32), _p(pos, torch.float32),
                                          _p(type0, torch.float32), n, D, _p(out, torch.bfloat16), _stream()), "toist_embed_fwd")


def embed_bwd(g, ids, pos_ids, pad_id, dword, dpos, dtype0):
    n, D = g.shape
    _lib.check(_lib.lib().toist_embed_bwd(_p(g, torch.bfloat16), _p(ids, torch.int64), _p(pos_ids, torch.int64), n, D, pad_id,
                                          _p(dword, torch.float32), _p(dpos, torch.float32), _p(dtype0, torch.float32), _stream()),
               "toist_embed_bwd")


def embed_bwd_sparse(g, ids, pos_ids, pad_id, dword, dpos, dtype0, touched_word, touched_pos, chunk):
    """embed_bwd into row-sparse gradient slots: touched_word / touched_pos (uint8, one byte per `chunk` elements of dword / dpos, or None) receive 1
    for every chunk a written row overlaps (include/toist_hip.h: toist_embed_bwd_sparse)"""
    n, D = g.shape
    for grad, t in ((dword, touched_word), (dpos, touched_pos)):
        if t is not None and (grad is None or t.numel() * chunk < grad.numel()):
            raise ValueError("embed_bwd_sparse: a touched array needs one byte per chunk of its gradient")
    _lib.check(_lib.lib().toist_embed_bwd_sparse(_p(g, torch.bfloat16), _p(ids, torch.int64), _p(pos_ids, torch.int64), n, D, pad_id,
                                                 _p(dword, torch.float32), _p(dpos, torch.float32), _p(dtype0, torch.float32),
                                                 _p(touched_word, torch.uint8), _p(touched_pos, torch.uint8), chunk, _stream()),
               "toist_embed_bwd_sparse")


def sparse_clear(slots, chunk):
    """slots: one or two (gradient, touched) pairs of row-sparse slots: zero every chunk whose byte is set and clear the byte, in one launch"""
    if not 1 <= len(slots) <= 2:
        raise ValueError("sparse_clear: one or two slots per launch")
    for grad, t in slots:
        if not grad.is_contiguous() or t.numel() * chunk < grad.numel():
            raise ValueError("sparse_clear: a contiguous gradient and one byte per chunk of it")
    (g0, t0), (g1, t1) = slots[0], (slots[1] if len(slots) > 1 else (None, None))
    _lib.check(_lib.lib().toist_sparse_clear(_p(g0, torch.float32), _p(t0, torch.uint8), g0.numel(), _p(g1, torch.float32), _p(t1, torch.uint8),
                                             0 if g1 is None else g1.numel(), chunk, _stream()), "toist_sparse_clear")


def criterion_fwd(logits, boxes, tgt_boxes, pos_map, tgt_off, match_off, src_idx, tgt_idx, num_boxes, eos_coef, losses, status=None):
    L, B, Q, K = logits.shape
    _lib.check(_lib.lib().toist_criterion_fwd(_p(logits, torch.float32), _p(boxes, torch.float32), _p(tgt_boxes, torch.float32),
                                              _p(pos_map, torch.float32), _p(tgt_off, torch.int32), _p(match_off, torch.int32),
                                              _p(src_idx, torch.int64), _p(tgt_idx, torch.int64), _p(num_boxes, torch.float32), L, B, Q, K,
                                              eos_coef, _p(losses, torch.float32), _p(status, torch.int32), _stream()), "toist_criterion_fwd")


def criterion_bwd(logits, boxes, tgt_boxes, pos_map, tgt_off, match_off, src_idx, tgt_idx, num_boxes, eos_coef, upstream, dlogits, dboxes):
    L, B, Q, K = logits.shape
    _lib.check(_lib.lib().toist_criterion_bwd(_p(logits, torch.float32), _p(boxes, torch.float32), _p(tgt_boxes, torch.float32),
                                              _p(pos_map, torch.float32), _p(tgt_off, torch.int32), _p(match_off, torch.int32),
                                              _p(src_idx, torch.int64), _p(tgt_idx, torch.int64), _p(num_boxes, torch.float32), L, B, Q, K,
                                              eos_coef, _p(upstream, torch.float32), _p(dlogits, torch.float32), _p(dboxes, torch.float32),
                                              _stream()), "toist_criterion_bwd")


def contrastive_fwd(pq, pt, tok_mask, tgt_off, match_off, src_idx, tgt_idx, num_boxes, temperature, losses, live_tokens=None):
    """live_tokens: device int32 [1] = how many of pt's T token columns are live (the rest is caption padding of a bucket); None = all of them."""
    L, B, Q, D = pq.shape
    if live_tokens is None:
        _lib.check(_lib.lib().toist_contrastive_fwd(_p(pq, torch.float32), _p(pt, torch.float32), _p(tok_mask, torch.int64), _p(tgt_off, torch.int32),
                                                    _p(match_off, torch.int32), _p(src_idx, torch.int64), _p(tgt_idx, torch.int64),
                                                    _p(num_boxes, torch.float32), L, B, Q, pt.shape[1], D, temperature, _p(losses, torch.float32),
                                                    _stream()), "toist_contrastive_fwd")
        return
    _lib.check(_lib.lib().toist_contrastive_fwd_live(_p(pq, torch.float32), _p(pt, torch.float32), _p(tok_mask, torch.int64), _p(tgt_off, torch.int32),
                                                     _p(match_off, torch.int32), _p(src_idx, torch.int64), _p(tgt_idx, torch.int64),
                                                     _p(num_boxes, torch.float32), L, B, Q, pt.shape[1], D, temperature, _p(live_tokens, torch.int32),
                                                     _p(losses, torch.float32), _stream()), "toist_contrastive_fwd_live")


def contrastive_bwd(pq, pt, tok_mask, tgt_off, match_off, src_idx, tgt_idx, num_boxes, temperature, upstream, dpq, dpt, live_tokens=None, workspace=None):
    """dpt +=: the caller zeroes it; with live_tokens (see contrastive_fwd) its dead rows are set to zero whatever they held.  workspace: fp32
    [L * B * T * D] scratch of the caller's, allocated here when None."""
    L, B, Q, D = pq.shape
    ws = workspace if workspace is not None else \
        torch.empty(L * B * pt.shape[1] * D, dtype=torch.float32, device=pq.device)     # each layer's token gradient, folded in layer order
    if ws.numel() < L * B * pt.shape[1] * D:
        raise ValueError(f"contrastive_bwd: the workspace holds {ws.numel()} floats, L * B * T * D = {L * B * pt.shape[1] * D}")
    if live_tokens is None:
        _lib.check(_lib.lib().toist_contrastive_bwd_ws(_p(pq, torch.float32), _p(pt, torch.float32), _p(tok_mask, torch.int64), _p(tgt_off, torch.int32),
                                                       _p(match_off, torch.int32), _p(src_idx, torch.int64), _p(tgt_idx, torch.int64),
                                                       _p(num_boxes, torch.float32), L, B, Q, pt.shape[1], D, temperature, _p(upstream, torch.float32),
                                                       _p(dpq, torch.float32), _p(dpt, torch.float32), _p(ws, torch.float32), _stream()), "toist_contrastive_bwd_ws")
        return
    _lib.check(_lib.lib().toist_contrastive_bwd_ws_live(_p(pq, torch.float32), _p(pt, torch.float32), _p(tok_mask, torch.int64), _p(tgt_off, torch.int32),
                                                        _p(match_off, torch.int32), _p(src_idx, torch.int64), _p(tgt_idx, torch.int64),
                                                        _p(num_boxes, torch.float32), L, B, Q, pt.shape[1], D, temperature,
                                                        _p(live_tokens, torch.int32), _p(upstream, torch.float32), _p(dpq, torch.float32),
                                                        _p(dpt, torch.float32), _p(ws, torch.float32), _stream()), "toist_contrastive_bwd_ws_live")


def l2norm_fwd(x, y):
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    _lib.check(_lib.lib().toist_l2norm_fwd(_p(x, torch.float32), rows, D, _p(y, torch.float32), _stream()), "toist_l2norm_fwd")


def l2norm_bwd(x, dy, dx):
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    _lib.check(_lib.lib().toist_l2norm_bwd(_p(x, torch.float32), _p(dy, torch.float32), rows, D, _p(dx, torch.float32), _stream()), "toist_l2norm_bwd")


# ---- segmentation branch ---------------------------------------------------------------------------------
BF16, F32 = torch.bfloat16, torch.float32


def attnmap_softmax_fwd(scores, key_pad, B, Q, H, HW, ld, out):
    _lib.check(_lib.lib().toist_attnmap_softmax_fwd(_p(scores, BF16), _p(key_pad, torch.uint8), B, Q, H, HW, ld, _p(out, BF16), _stream()),
               "toist_attnmap_softmax_fwd")


def attnmap_softmax_bwd(prob, dprob, BQ, H, HW, ld, dscores):
    _lib.check(_lib.lib().toist_attnmap_softmax_bwd(_p(prob, BF16), _p(dprob, BF16), BQ, H, HW, ld, _p(dscores, BF16), _stream()),
               "toist_attnmap_softmax_bwd")


def groupnorm_fwd(x, gamma, beta, N, HW, C, G, eps, relu, y, stats):
    _lib.check(_lib.lib().toist_groupnorm_fwd(_p(x, BF16), _p(gamma, F32), _p(beta, F32), N, HW, C, G, eps, 1 if relu else 0, _p(y, BF16),
                                              _p(stats, F32), _stream()), "toist_groupnorm_fwd")


def groupnorm_apply(x, stats, gamma, beta, N, HW, C, G, eps, relu, y):
    _lib.check(_lib.lib().toist_groupnorm_apply(_p(x, BF16), _p(stats, F32), _p(gamma, F32), _p(beta, F32), N, HW, C, G, eps, 1 if relu else 0, _p(y, BF16),
                                                _stream()), "toist_groupnorm_apply")


def groupnorm_bwd(dy, y, x, stats, gamma, N, HW, C, G, eps, relu, dx, dgamma, dbeta, bstats, beta=None):
    """y = None with beta given: the ReLU mask is re-derived from x (two passes over the activation fewer)"""
    _lib.check(_lib.lib().toist_groupnorm_bwd(_p(dy, BF16), _p(y, BF16), _p(x, BF16), _p(stats, F32), _p(gamma, F32), _p(beta, F32), N, HW, C, G, eps,
                                              1 if relu else 0, _p(dx, BF16), _p(dgamma, F32), _p(dbeta, F32), _p(bstats, F32), _stream()),
               "toist_groupnorm_bwd")


def upsample_add(inp, fpn, BQ, Q, H, W, C, out):
    _lib.check(_lib.lib().toist_upsample_add(_p(inp, BF16), _p(fpn, BF16), BQ, Q, H, W, C, _p(out, BF16), _stream()), "toist_upsample_add")


def resize_add(inp, fpn, rows, n, Q, H, W, OH, OW, C, out):
    """out [n, OH, OW, C] = fpn[image] + nearest-resized inp [n, H, W, C] (any target size; rows = None or the int64 map indices of a gathered subset)."""
    _lib.check(_lib.lib().toist_resize_add(_p(inp, BF16), _p(fpn, BF16), _p(rows, torch.int64), n, Q, H, W, OH, OW, C, _p(out, BF16), _stream()), "toist_resize_add")


def resize_add_bwd(dout, BQ, H, W, OH, OW, C, din):
    _lib.check(_lib.lib().toist_resize_add_bwd(_p(dout, BF16), BQ, H, W, OH, OW, C, _p(din, BF16), _stream()), "toist_resize_add_bwd")


def upsample_add_rows(inp, fpn, rows, n, Q, H, W, C, out):
    """upsample_add on gathered maps: map i of inp / out is map rows[i] (int64, device) of the batch."""
    _lib.check(_lib.lib().toist_upsample_add_rows(_p(inp, BF16), _p(fpn, BF16), _p(rows, torch.int64), n, Q, H, W, C, _p(out, BF16), _stream()),
               "toist_upsample_add_rows")


def mask_stage_fwd(src, src_stats, gamma, beta, fpn_conv, w, bias, out, out_stats, N, Q, H, W, c_in, c_out, w_rows, gn_in, up, eps=1e-5):
    """One fused stage of the mask head's tail (csrc/maskstage.hip): [GroupNorm + ReLU of the source] -> [2x upsample] -> 3x3 conv [+ fpn_conv, the
    image's lay(adapter(fpn)) [N/Q,H,W,c_out]] -> raw output + its GroupNorm sums (c_out > 1: out bf16 [N,H,W,c_out]) or the f32 mask logits
    (c_out == 1: out f32 [N,H,W])."""
    _lib.check(_lib.lib().toist_mask_stage_fwd(_p(src, BF16), _p(src_stats, F32), _p(gamma, F32), _p(beta, F32), _p(fpn_conv, BF16), _p(w, BF16), _p(bias, F32),
                                               _p(out, F32 if c_out == 1 else BF16), _p(out_stats, F32), N, Q, H, W, c_in, c_out, w_rows,
                                               1 if gn_in else 0, 1 if up else 0, eps, _stream()), "toist_mask_stage_fwd")


def upsample_add_bwd(dout, BQ, H, W, C, din):
    _lib.check(_lib.lib().toist_upsample_add_bwd(_p(dout, BF16), BQ, H, W, C, _p(din, BF16), _stream()), "toist_upsample_add_bwd")


def sum_queries(inp, B, Q, per, out):
    _lib.check(_lib.lib().toist_sum_queries(_p(inp, BF16), B, Q, per, _p(out, BF16), _stream()), "toist_sum_queries")


def mask_loss_fwd(pred, pred_row, gt, gt_row, T, h, w, TH, TW, alpha, sums, valid_hw=None):
    """valid_hw: optional device int32 [4] = {VH, VW, hs, ws}, the batch's own corner of a larger bucket (include/toist_hip.h)."""
    _lib.check(_lib.lib().toist_mask_loss_fwd(_p(pred, F32), _p(pred_row, torch.int32), _p(gt, torch.uint8), _p(gt_row, torch.int32), T, h, w, TH,
                                              TW, alpha, _p(sums, F32), _p(valid_hw, torch.int32), _stream()), "toist_mask_loss_fwd")


def sum_segments(inp, seg, B, rows, per, out):
    """out[b] = sum of the maps inp[seg[b]:seg[b+1]] (seg int32 [B+1] on the device)."""
    _lib.check(_lib.lib().toist_sum_segments(_p(inp, BF16), _p(seg, torch.int32), B, rows, per, _p(out, BF16), _stream()), "toist_sum_segments")


def mask_loss_bwd(pred, pred_row, gt, gt_row, T, h, w, TH, TW, alpha, sums, coef, dpred, compact=False, valid_hw=None):
    if compact:     # dpred is [T,h,w]: pair t's gradient in row t
        _lib.check(_lib.lib().toist_mask_loss_bwd_compact(_p(pred, F32), _p(pred_row, torch.int32), _p(gt, torch.uint8), _p(gt_row, torch.int32), T, h, w,
                                                          TH, TW, alpha, _p(sums, F32), _p(coef, F32), _p(dpred, F32), _p(valid_hw, torch.int32), _stream()), "toist_mask_loss_bwd_compact")
        return
    _lib.check(_lib.lib().toist_mask_loss_bwd(_p(pred, F32), _p(pred_row, torch.int32), _p(gt, torch.uint8), _p(gt_row, torch.int32), T, h, w, TH,
                                              TW, alpha, _p(sums, F32), _p(coef, F32), _p(dpred, F32), _p(valid_hw, torch.int32), _stream()), "toist_mask_loss_bwd")


# ---- optimizer tail (include/toist_hip.h: toist_opt_*) ---------------------------------------------------------
def opt_chunk_elems():
    return int(_lib.lib().toist_opt_chunk_elems())


def opt_sqnorm(table, grads, chunks, n_chunks, partial, touched=None):
    """touched: int64 device table parallel to grads (the addresses of the row-sparse gradients' touched bytes, 0 = dense), or None"""
    if touched is not None:
        _lib.check(_lib.lib().toist_opt_sqnorm_sparse(_p(table, torch.uint8), _p(grads, torch.int64), _p(touched, torch.int64), _p(chunks, torch.int32),
                                                      n_chunks, _p(partial, torch.float32), _stream()), "toist_opt_sqnorm_sparse")
        return
    _lib.check(_lib.lib().toist_opt_sqnorm(_p(table, torch.uint8), _p(grads, torch.int64), _p(chunks, torch.int32), n_chunks,
                                           _p(partial, torch.float32), _stream()), "toist_opt_sqnorm")


def opt_finish_norm(partial, n_chunks, max_norm, beta1, beta2, state):
    _lib.check(_lib.lib().toist_opt_finish_norm(_p(partial, torch.float32), n_chunks, max_norm, beta1, beta2, _p(state, torch.uint8),
                                                _stream()), "toist_opt_finish_norm")


def opt_finish_norm_guarded(partial, n_chunks, max_norm, beta1, beta2, state, veto_i32, n_veto_i32, veto_f32, n_veto_f32):
    """finish_norm that skips the step when the norm is not finite or a veto word objects; veto_i32 / veto_f32: int64 device tensors holding the
    device addresses of the words (include/toist_hip.h: toist_opt_finish_norm_guarded)"""
    _lib.check(_lib.lib().toist_opt_finish_norm_guarded(_p(partial, torch.float32), n_chunks, max_norm, beta1, beta2, _p(state, torch.uint8),
                                                        _p(veto_i32, torch.int64), n_veto_i32, _p(veto_f32, torch.int64), n_veto_f32, _stream()),
               "toist_opt_finish_norm_guarded")


def opt_adamw_ema(table, grads, chunks, n_chunks, groups, state, beta1, beta2, eps, ema_decay, max_blocks=0, touched=None, hot=None):
    """touched, hot: int64 device tables parallel to grads (include/toist_hip.h: toist_opt_adamw_ema_sparse), both or neither"""
    if touched is not None or hot is not None:
        _lib.check(_lib.lib().toist_opt_adamw_ema_sparse(_p(table, torch.uint8), _p(grads, torch.int64), _p(touched, torch.int64), _p(hot, torch.int64),
                                                         _p(chunks, torch.int32), n_chunks, _p(groups, torch.float32), _p(state, torch.uint8), beta1,
                                                         beta2, eps, ema_decay, max_blocks, _stream()), "toist_opt_adamw_ema_sparse")
        return
    _lib.check(_lib.lib().toist_opt_adamw_ema_blocks(_p(table, torch.uint8), _p(grads, torch.int64), _p(chunks, torch.int32), n_chunks,
                                                     _p(groups, torch.float32), _p(state, torch.uint8), beta1, beta2, eps, ema_decay, max_blocks, _stream()),
               "toist_opt_adamw_ema")


def lsap(cost, offset, rows, cols, n, max_rows, max_cols, max_cells, out_off, row_idx, col_idx, status, ld=0):
    _lib.check(_lib.lib().toist_lsap(_p(cost, torch.float32), _p(offset, torch.int64), _p(rows, torch.int32), _p(cols, torch.int32), ld, n, max_rows,
                                     max_cols, max_cells, _p(out_off, torch.int64), _p(row_idx, torch.int64), _p(col_idx, torch.int64),
                                     _p(status, torch.int32), _stream()), "toist_lsap")


def conv3x3_small(dgrad, src, w, shift, res, out, n_img, H, W, c_src, c_out):
    """3x3 / s1 / p1 convolution (or its data gradient) with <= 32 channels on both sides; w is [Co,3,3,Ci] bf16."""
    w_co, w_ci = int(w.shape[0]), int(w.shape[3])
    _lib.check(_lib.lib().toist_conv3x3_small(1 if dgrad else 0, _p(src, torch.bfloat16), _p(w, torch.bfloat16), _p(shift, torch.float32),
                                              _p(res, torch.bfloat16), _p(out, torch.bfloat16), n_img, H, W, c_src, c_out, w_co, w_ci, _stream()),
               "toist_conv3x3_small")


def wgrad3x3_small(dy, x, out, defer=False, accumulate=True):
    """out [Co,3,3,C] (f32) += weight gradient of a 3x3 / s1 / p1 convolution with C in {16, 32}, Co in {8, 16} (csrc/smallconv.hip):
    per-workgroup partials into the split-K arena, folded by the batched reduction (queued when defer=True)."""
    n_img, H, W, C = x.shape
    Co = dy.shape[-1]
    blocks = int(_lib.lib().toist_wgrad3x3_small_blocks())
    ws = FOLDS.acquire(blocks * Co * 9 * C, x.device, (out,))
    _lib.check(_lib.lib().toist_wgrad3x3_small(_p(dy, torch.bfloat16), _p(x, torch.bfloat16), _p(ws, torch.float32), n_img, H, W, C, Co, _stream()),
               "toist_wgrad3x3_small")
    FOLDS.queue(ws.data_ptr(), out, blocks, Co, 9 * C, 9 * C, accumulate=accumulate)
    if not defer:
        flush_reductions()


def attn2_splits(Sk):
    return int(_lib.lib().toist_attn2_splits(Sk))


def attn2_fwd(q, kmat, v, key_pad, B, H, Sq, Sk, dh, scale, drop_p, seed, ctx, lse):
    """Flash-style attention core (csrc/attn2.hip): q / k / v / ctx are column slices of packed [B*S, ld] bf16 buffers; lse f32 [B*H, Sq, 2]."""
    _lib.check(_lib.lib().toist_attn2_fwd(_p(q, torch.bfloat16), q.stride(0), _p(kmat, torch.bfloat16), kmat.stride(0), _p(v, torch.bfloat16), v.stride(0),
                                          _p(key_pad, torch.uint8), B, H, Sq, Sk, dh, scale, drop_p, seed, _p(SEED_DEV) if drop_p > 0 else None,
                                          _p(ctx, torch.bfloat16), ctx.stride(0), _p(lse, torch.float32), _stream()), "toist_attn2_fwd")


def attn2_bwd(q, kmat, v, ctx, dctx, lse, key_pad, B, H, Sq, Sk, dh, scale, drop_p, seed, dq, dk, dv, dq_part=None):
    """Key-owning backward of attn2_fwd: dk / dv written once; dq directly when attn2_splits(Sk) == 1, else its per-split shares go to
    dq_part (bf16 [splits, B*Sq, H*dh]) for the consumer's fold (kernels.rowgemm(fold=...))."""
    _lib.check(_lib.lib().toist_attn2_bwd(_p(q, torch.bfloat16), q.stride(0), _p(kmat, torch.bfloat16), kmat.stride(0), _p(v, torch.bfloat16), v.stride(0),
                                          _p(ctx, torch.bfloat16), ctx.stride(0), _p(dctx, torch.bfloat16), dctx.stride(0), _p(lse, torch.float32),
                                          _p(key_pad, torch.uint8), B, H, Sq, Sk, dh, scale, drop_p, seed, _p(SEED_DEV) if drop_p > 0 else None,
                                          _p(dq, torch.bfloat16), dq.stride(0) if dq is not None else 0, _p(dk, torch.bfloat16), dk.stride(0),
                                          _p(dv, torch.bfloat16), dv.stride(0), _p(dq_part, torch.bfloat16), _stream()), "toist_attn2_bwd")


def rowgemm(a, w, out, *, b_kind, epi, K=None, bias=None, res=None, res2=None, drop_p=0.0, drop_seed=0, gamma=None, beta=None, eps=1e-5,
            z=None, mean=None, rstd=None, add=None, out2=None, fold=None, fold_cols=0, dgamma=None, dbeta=None):
    """Row-complete sub-layer launch (csrc/tlayer.hip, include/toist_hip.h: toist_rowgemm): out[M, 256] from a[M, K] and the nn.Linear
    weight copy `w` read in place (b_kind B_ROWK = forward, B_KROW = data gradient), finished on chip by epi = ROW_PLAIN / ROW_LN_FWD /
    ROW_LN_BWD.  fold = bf16 [parts, M, fold_cols] partial sums that replace (and are written back into) a[:, :fold_cols].
    ROW_LN_BWD: dgamma / dbeta (f32 [256], accumulated) receive the parameter gradients through per-block partials queued for
    flush_reductions(), exactly like layernorm_bwd(defer=True)."""
    M = a.shape[0]
    d = _lib.RowGemm()
    d.M, d.K, d.b_kind, d.epi = M, (a.shape[1] if K is None else K), b_kind, epi
    d.a, d.lda, d.w, d.ldw = _p(a, torch.bfloat16), a.stride(0), _p(w, torch.bfloat16), w.stride(0)
    if fold is not None:
        d.fold, d.fold_parts, d.fold_cols, d.fold_stride = _p(fold, torch.bfloat16), fold.shape[0], fold_cols, fold.stride(0)
        assert fold.shape[1] == M and fold.shape[2] == fold_cols and fold.stride(1) == fold_cols
    d.bias = _p(bias, torch.float32)
    if res is not None:
        d.res, d.ldr = _p(res, torch.bfloat16), res.stride(0)
    if res2 is not None:
        d.res2, d.ldr2 = _p(res2, torch.bfloat16), res2.stride(0)
    d.drop_p, d.eps, d.drop_seed = drop_p, eps, drop_seed
    d.drop_seed_dev = _p(SEED_DEV) if drop_p > 0 else None
    d.gamma, d.beta = _p(gamma, torch.float32), _p(beta, torch.float32)
    for name, t in (("z", z), ("add", add), ("out2", out2)):
        if t is not None:
            assert t.is_contiguous() and t.shape[-1] == 256
            setattr(d, name, _p(t, torch.bfloat16))
    d.mean, d.rstd = _p(mean, torch.float32), _p(rstd, torch.float32)
    d.out, d.ldo = _p(out, torch.bfloat16), out.stride(0)
    keep = None
    if epi == _lib.ROW_LN_BWD and dgamma is not None:
        keep = _queue_ln_param_grads(int(_lib.lib().toist_rowgemm_blocks(M)), 256, dgamma, dbeta)
        d.partials = _p(keep, torch.float32)
    _lib.check(_lib.lib().toist_rowgemm(ctypes.byref(d), _stream()), "toist_rowgemm")
    return keep


ROW_PLAIN, ROW_LN_FWD, ROW_LN_BWD = _lib.ROW_PLAIN, _lib.ROW_LN_FWD, _lib.ROW_LN_BWD


# ---- XCD-resident decoder stack (csrc/xdec.hip) ------------------------------------------------------------------------------------------
XDEC_PROF = None
XDEC_TEST_ABSENT = 0    # failure-path tests only (tests/test_gpu_xdec.py): that many workgroups per XCD leave the launch at once
XDEC_LAUNCHES = 0       # forward launches issued (or captured) so far: Transformer.decode_tokens learns from it whether its program used one
XDEC_FAILED = False     # process-wide: a launch reported an expired spin (xdec_check) -> the decoder runs on the per-op launches from then on
_XDEC_CTL = {}          # device -> int32[1024] control words (tickets, arrival counters, sticky status)


def _xdec_ctl(device, create=True):
    """One set of control words per device: the launches need the whole chip, so two of them never run at the same time on one device (the forward and
    the backward launch of a step are ordered by the stream).  Allocated EAGERLY: words taken from a capturing graph's pool would be re-zeroed by every
    replay, sticky status word included -- xdec_supported() therefore refuses the launches while a capture is running and no words exist yet
    (a capture is always preceded by an eager warm-up step in toist_amd.harness / bench.py, which allocates them)."""
    ctl = _XDEC_CTL.get(device)
    if ctl is None and create:
        if torch.cuda.is_current_stream_capturing():
            return None
        ctl = _XDEC_CTL[device] = torch.zeros(_lib.XDEC_CTL_WORDS, dtype=torch.int32, device=device)
    return ctl


def _ranks_share_a_device():
    """True when the ranks of this job on this node cannot have one GPU each (the XCD-resident launches need all 256 CUs to themselves).  LOCAL_WORLD_SIZE is
    what torchrun / the driver's launch line export; without it (a hand-made rendezvous) the world size is the best bound there is."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return False
    local = os.environ.get("LOCAL_WORLD_SIZE")
    local = int(local) if local and local.isdigit() else dist.get_world_size()
    return local > torch.cuda.device_count()


def xdec_supported(B, Q, S, L, ff=2048):
    """The XCD-resident decoder launches need all 256 CUs of the device to themselves (one 147 KB workgroup per CU, 32 co-resident per image): not
    when several ranks of one job share a GPU (the one-GPU multi-rank tests; two such launches from two processes would starve each other until their
    bounded spins expire), not after a launch has reported an expired spin (XDEC_FAILED), not for a dim_feedforward other than the compiled-in 2048
    (ADVICE r5), and never with TOIST_XDEC=0 (the opt-out for a GPU shared with another process or a CU-masked queue: INTEGRATION.md)."""
    if XDEC_FAILED or ff != 2048 or _ranks_share_a_device():
        return False
    if not _lib.lib().toist_xdec_supported(B, Q, S, L):
        return False
    return _xdec_ctl(torch.device("cuda", torch.cuda.current_device())) is not None


def xdec_fwd(B, Q, S, x0, qpos, kv, key_pad, drop_p, eps, out, layers, part, *, xe0):
    """All decoder layers in one launch (include/toist_hip.h: toist_xdec_fwd).  `out` = dict of the stacked per-layer tensors named as the
    descriptor's fields; `layers` = one dict per layer with the 18 parameter tensors + "seed" (6 ints).  xe0 = bf16(x0 + qpos), the rows layer 0's
    q | k projections read (required: a caller whose x0 is all zeros, the model's decoder, passes qpos itself)."""
    d = _lib.Xdec()
    d.B, d.Q, d.S, d.L = B, Q, S, len(layers)
    d.ff, d.test_absent = int(layers[0]["w1"].shape[0]), XDEC_TEST_ABSENT
    assert all(tuple(ly["w1"].shape) == (d.ff, 256) and tuple(ly["w2"].shape) == (256, d.ff) for ly in layers)
    d.x0, d.qpos, d.kv, d.ldkv = _p(x0, torch.bfloat16), _p(qpos, torch.bfloat16), _p(kv, torch.bfloat16), kv.stride(0)
    assert xe0.is_contiguous() and xe0.shape == qpos.shape
    d.xe0 = _p(xe0, torch.bfloat16)
    d.key_pad = _p(key_pad, torch.uint8) if key_pad is not None else None
    d.drop_p, d.eps = drop_p, eps
    d.seed_dev = _p(SEED_DEV) if drop_p > 0 else None
    for name in ("qkv", "ctx_s", "z1", "y1", "y1e", "qc", "ctx_c", "z3", "y3", "h", "z4", "y4", "y4e"):
        t = out[name]
        assert t.is_contiguous()
        setattr(d, name, _p(t, torch.bfloat16))
    for name in ("lse_s", "mean1", "rstd1", "lse_c", "mean3", "rstd3", "mean4", "rstd4"):
        t = out[name]
        assert t.is_contiguous()
        setattr(d, name, _p(t, torch.float32))
    assert part.is_contiguous() and part.numel() >= B * 32 * 128 * 256
    d.part = _p(part, torch.bfloat16)
    d.ctl = _xdec_ctl(x0.device).data_ptr()       # (never None here: xdec_supported() said yes)
    d.prof = XDEC_PROF.data_ptr() if XDEC_PROF is not None else None      # diagnostics (tools/r5/xdec_bench.py): int64 [256, L, 8]
    for i, ly in enumerate(layers):
        e = d.layer[i]
        for name in ("w_in", "w_os", "w_q", "w_oc", "w1", "w2"):
            t = ly[name]
            assert t.is_contiguous()
            setattr(e, name, _p(t, torch.bfloat16))
        for name in ("b_in", "b_os", "g1", "be1", "b_q", "b_oc", "g3", "be3", "b1", "b2", "g4", "be4"):
            t = ly[name]
            assert t.is_contiguous()
            setattr(e, name, _p(t, torch.float32))
        for j in range(6):
            e.seed[j] = ly["seed"][j]
    global XDEC_LAUNCHES
    XDEC_LAUNCHES += 1
    _lib.check(_lib.lib().toist_xdec_fwd(ctypes.byref(d), _stream()), "toist_xdec_fwd")


def xdec_bwd(B, Q, S, kv, key_pad, drop_p, saved, g_out, outs, layers, scratch):
    """Data-gradient chain of all decoder layers in one launch (include/toist_hip.h: toist_xdec_bwd).  saved = the forward's stacked tensors,
    g_out bf16 [L, B*Q, 256], outs = dict(gb4, dh, go3, go1, sink, dkv, ln_part), scratch = dict(dctx, part, dq_part)."""
    d = _lib.XdecBwd()
    d.B, d.Q, d.S, d.L = B, Q, S, len(layers)
    d.ff, d.test_absent = int(layers[0]["w1"].shape[0]), XDEC_TEST_ABSENT
    d.kv, d.ldkv = _p(kv, torch.bfloat16), kv.stride(0)
    d.key_pad = _p(key_pad, torch.uint8) if key_pad is not None else None
    d.drop_p = drop_p
    d.seed_dev = _p(SEED_DEV) if drop_p > 0 else None
    for name in ("qkv", "ctx_s", "z1", "qc", "ctx_c", "z3", "h", "z4"):
        assert saved[name].is_contiguous()
        setattr(d, name, _p(saved[name], torch.bfloat16))
    for name in ("lse_s", "mean1", "rstd1", "lse_c", "mean3", "rstd3", "mean4", "rstd4"):
        assert saved[name].is_contiguous()
        setattr(d, name, _p(saved[name], torch.float32))
    assert g_out.is_contiguous() and g_out.shape == (len(layers), B * Q, 256)
    d.g_out = _p(g_out, torch.bfloat16)
    for name in ("gb4", "dh", "go3", "go1"):
        assert outs[name].is_contiguous()
        setattr(d, name, _p(outs[name], torch.bfloat16))
    sink, dkv = outs["sink"], outs["dkv"]
    assert sink.stride(1) == 1 and dkv.stride(1) == 1
    d.sink, d.ldsink, d.dkv, d.lddkv = _p(sink, torch.bfloat16), sink.stride(0), _p(dkv, torch.bfloat16), dkv.stride(0)
    d.ln_part = _p(outs["ln_part"], torch.float32)
    for name in ("dctx", "part", "dq_part"):
        assert scratch[name].is_contiguous()
        setattr(d, name, _p(scratch[name], torch.bfloat16))
    d.ctl = _xdec_ctl(kv.device).data_ptr()
    d.prof = XDEC_PROF.data_ptr() if XDEC_PROF is not None else None
    for i, ly in enumerate(layers):
        e = d.layer[i]
        for name in ("w_in", "w_os", "w_q", "w_oc", "w1", "w2"):
            assert ly[name].is_contiguous()
            setattr(e, name, _p(ly[name], torch.bfloat16))
        for name in ("g1", "g3", "g4"):
            setattr(e, name, _p(ly[name], torch.float32))
        for j in range(6):
            e.seed[j] = ly["seed"][j]
    _lib.check(_lib.lib().toist_xdec_bwd(ctypes.byref(d), _stream()), "toist_xdec_bwd")


def queue_fold(partials, out, splits, keep=()):
    """out[256] += sum over `splits` rows of partials [splits, 256] (f32), folded with the other deferred reductions of the current stream
    (flush_reductions): the LayerNorm parameter gradients of the XCD-resident backward."""
    FOLDS.queue(partials.data_ptr(), out, splits, 1, 256, 256, keep=(partials,) + tuple(keep), when_busy="flush")


def xdec_check(raise_on_failure=True):
    """The sticky status words of the XCD-resident launches (synchronises: one 4-byte read per device).  A set word means a bounded spin expired -- the 32
    workgroups of an image were not co-resident (a second process on the GPU, a CU-masked queue, an unexpected dispatch order) -- and that launch's
    results are invalid (the launch also turned them into NaN, so the losses of that step are NaN).  The word is cleared, XDEC_FAILED is set so that
    every later decoder forward / backward runs on the per-op launches (graphs captured with the launches inside must be re-captured:
    harness.CapturedTrainStep does), and RuntimeError is raised unless raise_on_failure is False (then the return value says whether a launch failed).
    What the failed step did to TRAINING state depends on the optimizer: a FusedClipAdamWEMA(skip_nonfinite=True) inside a captured step has this word
    as a veto and skipped the update (captured._CapturedStep.resolve_skipped calls this function: repeat the step); without the guard the NaN
    gradients of that launch have already been applied to the weights, the moments and the EMA, and only a checkpoint helps.
    Called by harness.finite_or_exit, CapturedTrainStep when a replayed loss is not finite, harness.evaluate, Transformer's eval-mode decode, bench.py,
    smoke()."""
    global XDEC_FAILED
    failed = False
    for dev, ctl in _XDEC_CTL.items():
        if int(ctl[_lib.XDEC_CTL_WORDS - 1].item()) != 0:
            failed = True
            ctl[_lib.XDEC_CTL_WORDS - 1] = 0
    if failed:
        XDEC_FAILED = True
        if raise_on_failure:
            raise RuntimeError("toist_xdec: a workgroup gave up waiting for its XCD group (the 32 workgroups of an image were not co-resident); the results of "
                               "that step are invalid (NaN).  The XCD-resident decoder launches are now off for this process.  Inference, and training "
                               "under FusedClipAdamWEMA(skip_nonfinite=True) (the update of that step was skipped): repeat the step (per-op launches).  "
                               "Training without that guard: the step's NaN gradients are already in the weights, restore from a checkpoint.  Start "
                               "with TOIST_XDEC=0 when the GPU is shared")
    return failed


def scatter_rows(src, src_row, dst, dst_row):
    """dst[dst_row[i]] = src[src_row[i]] (f32 rows) for the i with both indices >= 0 (int64 device vectors); see toist_scatter_rows_f32."""
    assert src.is_contiguous() and dst.is_contiguous() and src.shape[-1] == dst.shape[-1]
    _lib.check(_lib.lib().toist_scatter_rows_f32(_p(src, torch.float32), _p(src_row, torch.int64), _p(dst, torch.float32), _p(dst_row, torch.int64), src_row.numel(),
                                                 src.shape[-1], _stream()), "toist_scatter_rows_f32")


def kmeans(banks, centers, group_task, group_off, members, features, tol, max_iter, pick, chosen_center, iters=None):
    """banks [T, N, D] f32, centers [T, K, D] f32 (updated in place); see toist_kmeans."""
    T, N, D = banks.shape
    K = centers.shape[1]
    _lib.check(_lib.lib().toist_kmeans(_p(banks, torch.float32), banks.stride(0), _p(centers, torch.float32), centers.stride(0), _p(group_task, torch.int32),
                                       _p(group_off, torch.int32), _p(members, torch.int32), group_task.numel(), _p(features, torch.float32), N, D, K, tol,
                                       max_iter, _p(pick, torch.int32), _p(chosen_center, torch.float32), _p(iters, torch.int32), _stream()), "toist_kmeans")


def sweep_prototypes(memory, memory_mod, pair_caption, tables, banks, centers, HW, tol=1e-4, max_iter=10000, pick=None, features=None, iters=None):
    """The prototype choice of a task sweep in one launch (include/toist_hip.h: toist_sweep_prototypes).  memory bf16 [P, S, D] (or [P * S, D]), the
    encoder output, read only; memory_mod: the same shape, holding a copy of it -- the rows of the word 'something' of every live pair receive the
    chosen prototype; pair_caption int32 [P] ON THE DEVICE; tables: a distill.SweepChoiceTables on that device (W_sth, sub_sth, cap_task, group_task,
    live); banks [T_tasks, N, D] f32, centers [T_tasks, K, D] f32 (updated in place); HW: the image rows in front of every pair's L caption rows.
    pick int32 [P] / features f32 [P, D] / iters int32 [P]: optional outputs, written for served pairs only.  ValueError before any launch: shapes that
    disagree, D > 256, K > 8, K * D > 1024, L > 256, a bank of more than 32768 rows (its choice bytes are the launch's dynamic LDS).  A pair_caption
    entry outside the captions raises the sweep status word (sweep_check)."""
    T, L = tables.W_sth.shape
    P = pair_caption.numel()
    n_tasks, N, D = banks.shape
    K = centers.shape[1]
    S = int(HW) + L
    dev = memory.device
    if memory.numel() != P * S * D or memory_mod.shape != memory.shape or memory.dtype != torch.bfloat16 or memory_mod.dtype != torch.bfloat16:
        raise ValueError(f"sweep_prototypes: memory and memory_mod are bf16 [P, S, D] = [{P}, {S}, {D}] (got {tuple(memory.shape)}, {tuple(memory_mod.shape)})")
    if memory.data_ptr() == memory_mod.data_ptr():
        raise ValueError("sweep_prototypes: memory_mod is a copy of memory, not memory itself (memory is never written)")
    if centers.shape[0] != n_tasks or centers.shape[2] != D or tuple(tables.sub_sth.shape) != (T, L) or tables.cap_task.numel() != T or \
            tables.group_task.numel() != T or tables.live.numel() != 1 or pair_caption.dim() != 1:
        raise ValueError("sweep_prototypes: banks [T_tasks, N, D], centers [T_tasks, K, D] and tables of T captions x L tokens must agree")
    if D > 256 or K > 8 or K * D > 1024 or L > 256 or N > 32768 or HW < 0:
        raise ValueError(f"sweep_prototypes: D <= 256, K <= 8, K * D <= 1024, L <= 256, N <= 32768 (D={D} K={K} L={L} N={N})")
    for t in (memory, memory_mod, pair_caption, banks[0], centers[0], tables.W_sth, tables.sub_sth):
        if not t.is_contiguous():
            raise ValueError("sweep_prototypes: every tensor must be contiguous (banks and centers per task)")
    for t, n in ((pick, P), (features, P * D), (iters, P)):
        if t is not None and (t.numel() != n or not t.is_contiguous()):
            raise ValueError("sweep_prototypes: pick [P], features [P, D] and iters [P], contiguous")
    status = sweep_status(dev)
    if status is None:
        raise RuntimeError("sweep_prototypes: the first sweep launch on a device cannot be captured (its status word is allocated outside any graph)")
    _lib.check(_lib.lib().toist_sweep_prototypes(_p(memory, torch.bfloat16), _p(memory_mod, torch.bfloat16), _p(pair_caption, torch.int32),
                                                 _p(tables.live, torch.int32), _p(tables.W_sth, torch.float32), _p(tables.sub_sth, torch.uint8),
                                                 _p(tables.cap_task, torch.int32), _p(tables.group_task, torch.int32), _p(banks, torch.float32),
                                                 banks.stride(0), _p(centers, torch.float32), centers.stride(0), P, int(HW), L, T, n_tasks, N, D, K, tol,
                                                 max_iter, _p(status, torch.int32), _p(pick, torch.int32), _p(features, torch.float32),
                                                 _p(iters, torch.int32), _stream()), "toist_sweep_prototypes")


def kmeans_init(banks, centers, group_task, group_off, members, features, tol, max_iter, pick, chosen_center, full_label, init_rows, status, iters=None):
    """kmeans() whose start the device decides per sample: full_label f32 [T], init_rows i32 [B, K] (bank rows drawn on the host, or -1), status i32 [1]
    (bit 0 = the two disagreed); see toist_kmeans_init."""
    T, N, D = banks.shape
    K = centers.shape[1]
    assert init_rows.is_contiguous() and init_rows.shape == (features.shape[0], K) and full_label.numel() == T and status.numel() == 1
    _lib.check(_lib.lib().toist_kmeans_init(_p(banks, torch.float32), banks.stride(0), _p(centers, torch.float32), centers.stride(0), _p(group_task, torch.int32),
                                            _p(group_off, torch.int32), _p(members, torch.int32), group_task.numel(), _p(features, torch.float32), N, D, K, tol,
                                            max_iter, _p(pick, torch.int32), _p(chosen_center, torch.float32), _p(iters, torch.int32),
                                            _p(full_label, torch.float32), _p(init_rows, torch.int32), _p(status, torch.int32), _stream()), "toist_kmeans_init")


def bank_fifo(banks, update_count, full_label, group_task, group_off, members, rows, fifo_when_full, lsap_rows):
    """FIFO memory-bank update + update_count / full_label bookkeeping for the groups whose task is still filling (or all, with fifo_when_full);
    lsap_rows i32 [n_groups] receives the row counts left to the nearest-replacement LSAP; see toist_bank_fifo."""
    T, N, D = banks.shape
    B = rows.shape[0]
    assert banks[0].is_contiguous() and rows.is_contiguous() and rows.shape[1] == D and update_count.numel() == T and full_label.numel() == T
    assert group_off.numel() == group_task.numel() + 1 and members.numel() >= B and lsap_rows.numel() == group_task.numel()
    _lib.check(_lib.lib().toist_bank_fifo(_p(banks, torch.float32), banks.stride(0), _p(update_count, torch.float32), _p(full_label, torch.float32),
                                          _p(group_task, torch.int32), _p(group_off, torch.int32), _p(members, torch.int32), group_task.numel(),
                                          _p(rows, torch.float32), T, B, N, D, int(bool(fifo_when_full)), _p(lsap_rows, torch.int32), _stream()), "toist_bank_fifo")


def attn_small_fwd(q, kmat, v, key_pad, B, H, S, dh, scale, drop_p, seed, ctx, stats, bq=None, bk=None, bv=None):
    """Whole-head self-attention for S <= 64, dh <= 64 (csrc/attn_small.hip); column slices of packed buffers, optional projection biases."""
    _lib.check(_lib.lib().toist_attn_small_fwd(_p(q, torch.bfloat16), q.stride(0), _p(kmat, torch.bfloat16), kmat.stride(0), _p(v, torch.bfloat16), v.stride(0),
                                               _p(key_pad, torch.uint8), B, H, S, dh, scale, drop_p, seed, _p(SEED_DEV) if drop_p > 0 else None,
                                               _p(ctx, torch.bfloat16), ctx.stride(0), _p(stats, torch.float32), _p(bq, torch.float32), _p(bk, torch.float32),
                                               _p(bv, torch.float32), _stream()), "toist_attn_small_fwd")


def attn_small_bwd(q, kmat, v, key_pad, B, H, S, dh, scale, drop_p, seed, stats, dctx, dq, dk, dv, bq=None, bk=None, bv=None):
    _lib.check(_lib.lib().toist_attn_small_bwd(_p(q, torch.bfloat16), q.stride(0), _p(kmat, torch.bfloat16), kmat.stride(0), _p(v, torch.bfloat16), v.stride(0),
                                               _p(key_pad, torch.uint8), B, H, S, dh, scale, drop_p, seed, _p(SEED_DEV) if drop_p > 0 else None,
                                               _p(stats, torch.float32), _p(dctx, torch.bfloat16), dctx.stride(0), _p(dq, torch.bfloat16), dq.stride(0),
                                               _p(dk, torch.bfloat16), dk.stride(0), _p(dv, torch.bfloat16), dv.stride(0), _p(bq, torch.float32),
                                               _p(bk, torch.float32), _p(bv, torch.float32), _stream()), "toist_attn_small_bwd")


# ---- evaluation masks (csrc/evalmask.hip): column-major bit planes [n, W, ceil(H/64)] stored in int64 tensors --------------
def mask_words(h):
    return (h + 63) // 64


def _plane(n, h, w, device):
    if h * w >= 2 ** 31:
        raise ValueError("mask planes address pixels with 31 bits")
    return torch.empty(n, w, mask_words(h), dtype=torch.int64, device=device)


def mask_resize_pack(logits, max_size, crop, out_size, threshold=0.5):
    """[n, h0, w0] fp32 mask logits -> bit planes of sigmoid(resize(resize(.)[:crop])) > threshold (PostProcessSegm's arithmetic)."""
    n, h0, w0 = logits.shape
    bits = _plane(n, out_size[0], out_size[1], logits.device)
    _lib.check(_lib.lib().toist_mask_resize_pack(_p(logits.contiguous(), torch.float32), n, h0, w0, int(max_size[0]), int(max_size[1]), int(crop[0]),
                                                 int(crop[1]), int(out_size[0]), int(out_size[1]), float(threshold), _p(bits), _stream()),
               "toist_mask_resize_pack")
    return bits


def mask_resize_pack_batch(logits, max_size, table, cap_hw, capacity_words, out, threshold=0.5):
    """mask_resize_pack for every image of a batch in one launch that reads its sizes from the device (include/toist_hip.h:
    toist_mask_resize_pack_batch).  logits [B, Q, h0, w0] fp32 contiguous, table int64 [B, 4] = (crop_h, crop_w, h, w) on the device, out int64
    [>= B * capacity_words]: image i's planes [Q, w_i, ceil(h_i/64)] start at word i * capacity_words.  No host read, no allocation: graph-capturable."""
    B, Q, h0, w0 = logits.shape
    if not logits.is_contiguous() or tuple(table.shape) != (B, 4) or not table.is_contiguous():
        raise ValueError("mask_resize_pack_batch: contiguous [B, Q, h0, w0] logits and a contiguous int64 [B, 4] table")
    if out.numel() < B * int(capacity_words):
        raise ValueError(f"mask_resize_pack_batch: the output holds {out.numel()} words, {B} x {int(capacity_words)} are needed")
    _lib.check(_lib.lib().toist_mask_resize_pack_batch(_p(logits, torch.float32), B, Q, h0, w0, int(max_size[0]), int(max_size[1]), _p(table, torch.int64),
                                                       int(cap_hw[0]), int(cap_hw[1]), int(capacity_words), float(threshold), _p(out, torch.int64), _stream()),
               "toist_mask_resize_pack_batch")
    return out


def image_prep(src, desc, arena, lut=None, out=None, mask=None, dst_u8=None, cap_hw=None):
    """Resize (Pillow-exact bilinear) + normalise + pad + mask of a batch of uint8 images in one launch that reads every size from the device
    (include/toist_hip.h: toist_image_prep).  src uint8 [bytes], desc int32 [batch capacity, PREP_DESC_WORDS], arena int32 [words]: fixed-address
    device buffers that toist_amd.preprocess.DevicePreprocessor fills.  Final mode: out fp32 [B, 3, Hp, Wp] + mask bool [B, Hp, Wp] + lut fp32 [3, 256];
    intermediate mode: dst_u8 uint8 [bytes] + cap_hw = the largest (h, w) the grid has to cover.  No host read, no allocation: graph-capturable."""
    if desc.dim() != 2 or desc.shape[1] != _lib.PREP_DESC_WORDS or not desc.is_contiguous() or not src.is_contiguous() or not arena.is_contiguous():
        raise ValueError(f"image_prep: contiguous buffers and an int32 [B, {_lib.PREP_DESC_WORDS}] descriptor table")
    B = desc.shape[0]
    if (out is None) == (dst_u8 is None):
        raise ValueError("image_prep: exactly one of `out` (final mode) and `dst_u8` (intermediate mode)")
    if out is not None:
        if mask is None or lut is None or tuple(lut.shape) != (3, 256) or not lut.is_contiguous():
            raise ValueError("image_prep: the final mode needs the mask and a contiguous fp32 [3, 256] normalisation table")
        Hp, Wp = int(out.shape[-2]), int(out.shape[-1])
        if tuple(out.shape) != (B, 3, Hp, Wp) or tuple(mask.shape) != (B, Hp, Wp) or not out.is_contiguous() or not mask.is_contiguous() or Wp % 4:
            raise ValueError(f"image_prep: contiguous out [{B}, 3, Hp, Wp] and mask [{B}, Hp, Wp] with Wp % 4 == 0 (got {tuple(out.shape)}, {tuple(mask.shape)})")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"image_prep: the mask holds bytes (bool or uint8), got {mask.dtype}")
        args = (_p(lut, torch.float32), B, Hp, Wp, _p(out, torch.float32), _p(mask), None, 0)
    else:
        if not dst_u8.is_contiguous() or cap_hw is None:
            raise ValueError("image_prep: the intermediate mode needs a contiguous uint8 destination and cap_hw")
        args = (None, B, int(cap_hw[0]), int(cap_hw[1]), None, None, _p(dst_u8, torch.uint8), dst_u8.numel())
    _lib.check(_lib.lib().toist_image_prep(_p(src, torch.uint8), src.numel(), _p(desc, torch.int32), _p(arena, torch.int32), arena.numel(), *args, _stream()),
               "toist_image_prep")


def target_masks(src, desc, arena, out):
    """The prepared masks of a batch's targets in one launch that reads every size from the device (include/toist_hip.h: toist_target_masks): a gather
    of single bits of the original-size masks through one row table and one column table per image.  src uint8 [bytes], desc int32 [slots,
    TMASK_DESC_WORDS], arena int32 [words]: fixed-address device buffers that toist_amd.preprocess.DeviceTargetMasks fills; out uint8 (or bool)
    [slots, cap_h, cap_w].  A slot whose row has out_h = 0 is left as it is.  No host read, no allocation: graph-capturable."""
    if desc.dim() != 2 or desc.shape[1] != _lib.TMASK_DESC_WORDS or not desc.is_contiguous() or not src.is_contiguous() or not arena.is_contiguous():
        raise ValueError(f"target_masks: contiguous buffers and an int32 [slots, {_lib.TMASK_DESC_WORDS}] descriptor table")
    S = desc.shape[0]
    if out.dim() != 3 or out.shape[0] != S or not out.is_contiguous():
        raise ValueError(f"target_masks: a contiguous output [{S}, cap_h, cap_w] (got {tuple(out.shape)})")
    if out.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"target_masks: the output holds bytes (uint8 or bool), got {out.dtype}")
    _lib.check(_lib.lib().toist_target_masks(_p(src, torch.uint8), src.numel(), _p(desc, torch.int32), _p(arena, torch.int32), arena.numel(), S,
                                             int(out.shape[1]), int(out.shape[2]), _p(out), _stream()), "toist_target_masks")
    return out


POLYGON_STRIP, POLYGON_MAX_ROWS = _lib.POLY_STRIP, _lib.POLY_MAX_ROWS      # columns of a workgroup's strip, rows of its LDS plane (the tallest image)


def polygon_masks(desc, polys, verts, dst, cap_hw=None):
    """The masks of a batch's polygon annotations in one launch that reads every size from the device (include/toist_hip.h: toist_polygon_masks), bit
    for bit what coco_eval.polygon_to_mask / convert_coco_poly_to_mask give on the host.  desc int32 [slots, POLY_DESC_WORDS], polys int32 [polygon
    capacity, POLY_REC_WORDS], verts int32 [vertex capacity, 2]: fixed-address device buffers that toist_amd.preprocess.DevicePolygonMasks fills.
    dst uint8 [bytes] + cap_hw = the largest (h, w) the grid has to cover: packed bits (pack_mask_bits' layout) at every row's dst_off; dst uint8 (or
    bool) [slots, cap_h, cap_w]: dense bytes, the live h x w region of every slot.  A slot whose row has h = 0 is left as it is.  No host read, no
    allocation: graph-capturable."""
    if desc.dim() != 2 or desc.shape[1] != _lib.POLY_DESC_WORDS or polys.dim() != 2 or polys.shape[1] != _lib.POLY_REC_WORDS or verts.dim() != 2 or \
            verts.shape[1] != 2 or not (desc.is_contiguous() and polys.is_contiguous() and verts.is_contiguous() and dst.is_contiguous()):
        raise ValueError(f"polygon_masks: contiguous int32 tables [slots, {_lib.POLY_DESC_WORDS}], [polygons, {_lib.POLY_REC_WORDS}], [vertices, 2] and a contiguous output")
    S = desc.shape[0]
    if dst.dim() == 3:
        if dst.shape[0] != S or cap_hw is not None and tuple(cap_hw) != tuple(dst.shape[1:]):
            raise ValueError(f"polygon_masks: a dense output is [{S}, cap_h, cap_w] (got {tuple(dst.shape)}, cap_hw {cap_hw})")
        if dst.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"polygon_masks: the output holds bytes (uint8 or bool), got {dst.dtype}")
        mode, (cap_h, cap_w) = _lib.POLY_DENSE, (int(dst.shape[1]), int(dst.shape[2]))
    elif dst.dim() == 1 and cap_hw is not None and dst.dtype == torch.uint8:
        mode, (cap_h, cap_w) = _lib.POLY_PACKED, (int(cap_hw[0]), int(cap_hw[1]))
    else:
        raise ValueError("polygon_masks: the output is uint8 [bytes] with cap_hw (packed bits) or [slots, cap_h, cap_w] (dense bytes)")
    if not 0 < cap_h <= POLYGON_MAX_ROWS or cap_w <= 0:
        raise ValueError(f"polygon_masks: a capacity of {cap_h} x {cap_w}: at most {POLYGON_MAX_ROWS} rows fit the kernel's plane")
    _lib.check(_lib.lib().toist_polygon_masks(_p(desc, torch.int32), S, _p(polys, torch.int32), polys.shape[0], _p(verts, torch.int32), verts.shape[0],
                                              cap_h, cap_w, _p(dst), dst.numel(), mode, _stream()), "toist_polygon_masks")
    return dst


def postprocess(pred_logits, pred_boxes, sizes_dev, pred_isfinal=None, out=None):
    """PostProcess in one launch (include/toist_hip.h: toist_postprocess).  pred_logits [B, Q, C] and pred_boxes [B, Q, 4] in bf16 or f32, pred_isfinal
    [B, Q] (or [B, Q, 1]) optional, sizes_dev int64 [B, 2] = (h, w) ON THE DEVICE.  -> dict(scores f32 [B, Q], boxes f32 [B, Q, 4] (+ scores_refexp));
    `out` = such a dict to write into (fixed addresses for a captured graph)."""
    B, Q, C = pred_logits.shape
    dev = pred_logits.device

    def kind(t, what):
        if t.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"postprocess: {what} must be bf16 or f32, got {t.dtype}")
        return 1 if t.dtype == torch.bfloat16 else 0

    if tuple(pred_boxes.shape) != (B, Q, 4) or tuple(sizes_dev.shape) != (B, 2):
        raise ValueError("postprocess: pred_boxes [B, Q, 4] and sizes [B, 2] must match pred_logits [B, Q, C]")
    if pred_isfinal is not None and pred_isfinal.numel() != B * Q:
        raise ValueError("postprocess: pred_isfinal must hold one value per query")
    if out is None:
        out = {"scores": torch.empty(B, Q, dtype=torch.float32, device=dev), "boxes": torch.empty(B, Q, 4, dtype=torch.float32, device=dev)}
        if pred_isfinal is not None:
            out["scores_refexp"] = torch.empty(B, Q, dtype=torch.float32, device=dev)
    logits, boxes = pred_logits.contiguous(), pred_boxes.contiguous()
    final = pred_isfinal.contiguous() if pred_isfinal is not None else None
    _lib.check(_lib.lib().toist_postprocess(_p(logits), kind(logits, "pred_logits"), _p(boxes), kind(boxes, "pred_boxes"), _p(final),
                                            kind(final, "pred_isfinal") if final is not None else 0, _p(sizes_dev.contiguous(), torch.int64), B, Q, C,
                                            _p(out["scores"], torch.float32), _p(out["boxes"], torch.float32),
                                            _p(out["scores_refexp"], torch.float32) if final is not None else None, _stream()), "toist_postprocess")
    return out


# ---- task sweep (csrc/sweep.hip) ----------------------------------------------------------------------------------------------------------
_SWEEP_STATUS = {}      # device -> int32[1]: max over the launches since the last sweep_check() of (first bad pair + 1)


def sweep_status(device, create=True):
    """The status word of the device's toist_sweep_assemble launches.  Allocated once per device and EAGERLY, like the XCD-resident decoder's control
    words: a word taken from a capturing graph's pool could be handed out again inside that graph.  None while a capture runs and no word exists yet."""
    device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
    st = _SWEEP_STATUS.get(device)
    if st is None and create:
        if torch.cuda.is_current_stream_capturing():
            return None
        st = _SWEEP_STATUS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return st


def sweep_check(raise_on_failure=True):
    """Read (and clear) the status words of the task-sweep launches: one 4-byte read per device, it synchronises.  A set word means that a launch met a
    pair-table entry outside its images / captions; that pair's sequence is zeros, so its results mean nothing.  -> 0, or the first such pair + 1
    (raise_on_failure=False); raises ValueError otherwise.  Called where results are handed out: harness.evaluate_sweep, CapturedSweepStep.step."""
    bad = 0
    for st in _SWEEP_STATUS.values():
        v = int(st.item())
        if v:
            st.zero_()
            bad = bad or v
    if bad and raise_on_failure:
        raise ValueError(f"sweep_assemble: pair {bad - 1} names an image or a caption that does not exist (its sequence was zeroed on the device)")
    return bad


def sweep_assemble(img_tok, img_pos, img_pad, txt_tok, txt_pad, pair_image, pair_caption, out=None, check=True):
    """The cross-modal sequences of P (image, caption) pairs in one launch (include/toist_hip.h: toist_sweep_assemble).  img_tok / img_pos bf16
    [B, HW, D], img_pad bool or uint8 [B, HW], txt_tok bf16 [T, L, D], txt_pad bool or uint8 [T, L], pair_image / pair_caption int32 [P] ON THE DEVICE.
    -> (tokens bf16 [P, S, D], pos bf16 [P, S, D], key_pad uint8 [P, S]), S = HW + L; `out` = such a triple to write into (fixed addresses for a
    captured graph).  check: read the status word right away (synchronises; never during a capture) -- a caller that validated the tables on the host
    passes False and calls sweep_check() where it hands its results out."""
    B, HW, D = img_tok.shape
    T, L = txt_tok.shape[:2]
    P, S, dev = pair_image.numel(), HW + L, img_tok.device
    u8 = lambda t: t.view(torch.uint8) if t.dtype == torch.bool else t
    img_pad, txt_pad = u8(img_pad), u8(txt_pad)
    if tuple(img_pos.shape) != (B, HW, D) or tuple(img_pad.shape) != (B, HW) or tuple(txt_tok.shape) != (T, L, D) or tuple(txt_pad.shape) != (T, L):
        raise ValueError("sweep_assemble: img_tok / img_pos [B, HW, D], img_pad [B, HW], txt_tok [T, L, D] and txt_pad [T, L] must agree")
    if pair_caption.numel() != P or pair_image.dim() != 1 or pair_caption.dim() != 1:
        raise ValueError("sweep_assemble: pair_image and pair_caption are int32 vectors of one length")
    for t in (img_tok, img_pos, img_pad, txt_tok, txt_pad, pair_image, pair_caption):
        if not t.is_contiguous():
            raise ValueError("sweep_assemble: every input must be contiguous")
    status = sweep_status(dev)
    if status is None:
        raise RuntimeError("sweep_assemble: the first launch on a device cannot be captured (its status word is allocated outside any graph)")
    if out is None:
        out = (torch.empty(P, S, D, dtype=torch.bfloat16, device=dev), torch.empty(P, S, D, dtype=torch.bfloat16, device=dev),
               torch.empty(P, S, dtype=torch.uint8, device=dev))
    tokens, pos, key_pad = out
    if tuple(tokens.shape) != (P, S, D) or tuple(pos.shape) != (P, S, D) or tuple(key_pad.shape) != (P, S) or not all(t.is_contiguous() for t in out):
        raise ValueError("sweep_assemble: out = (tokens [P, S, D], pos [P, S, D], key_pad [P, S]), contiguous")
    _lib.check(_lib.lib().toist_sweep_assemble(_p(img_tok, torch.bfloat16), _p(img_pos, torch.bfloat16), _p(img_pad, torch.uint8), B, HW,
                                               _p(txt_tok, torch.bfloat16), _p(txt_pad, torch.uint8), T, L, _p(pair_image, torch.int32),
                                               _p(pair_caption, torch.int32), P, D, _p(tokens, torch.bfloat16), _p(pos, torch.bfloat16),
                                               _p(key_pad, torch.uint8), _p(status, torch.int32), _stream()), "toist_sweep_assemble")
    if check and not torch.cuda.is_current_stream_capturing():
        sweep_check()
    return out


def sweep_assemble_bwd(d_seq, pair_image, pair_caption, B, HW, T, L, want_img=True, want_txt=True, out=None):
    """The gradient of sweep_assemble with respect to its token inputs in one launch (include/toist_hip.h: toist_sweep_assemble_bwd).  d_seq bf16
    [P, HW + L, D], pair_image / pair_caption int32 [P] ON THE DEVICE -> (d_img bf16 [B, HW, D] or None, d_txt bf16 [T, L, D] or None): per element
    the fp32 sum over the image's (caption's) pairs in ascending pair order, rounded to bf16 once.  want_img / want_txt = False skips that half (a
    frozen backbone / text side).  Every element of an output is written; out = (d_img, d_txt) buffers to write into."""
    B, HW, T, L = int(B), int(HW), int(T), int(L)
    if d_seq.dim() != 3 or d_seq.shape[1] != HW + L:
        raise ValueError(f"sweep_assemble_bwd: d_seq must be [P, HW + L, D] with HW + L = {HW + L} (got {tuple(d_seq.shape)})")
    P, S, D = d_seq.shape
    dev = d_seq.device
    if pair_image.dim() != 1 or pair_caption.dim() != 1 or pair_image.numel() != P or pair_caption.numel() != P:
        raise ValueError("sweep_assemble_bwd: pair_image and pair_caption are int32 vectors with one entry per row of d_seq")
    for t in (d_seq, pair_image, pair_caption):
        if not t.is_contiguous():
            raise ValueError("sweep_assemble_bwd: every input must be contiguous")
    d_img, d_txt = out if out is not None else (None, None)
    if want_img and d_img is None:
        d_img = torch.empty(B, HW, D, dtype=torch.bfloat16, device=dev)
    if want_txt and d_txt is None:
        d_txt = torch.empty(T, L, D, dtype=torch.bfloat16, device=dev)
    d_img, d_txt = (d_img if want_img else None), (d_txt if want_txt else None)
    if (d_img is not None and (tuple(d_img.shape) != (B, HW, D) or not d_img.is_contiguous())) or \
            (d_txt is not None and (tuple(d_txt.shape) != (T, L, D) or not d_txt.is_contiguous())):
        raise ValueError("sweep_assemble_bwd: out = (d_img [B, HW, D], d_txt [T, L, D]), contiguous")
    _lib.check(_lib.lib().toist_sweep_assemble_bwd(_p(d_seq, torch.bfloat16), _p(pair_image, torch.int32), _p(pair_caption, torch.int32), P, B, HW, T, L,
                                                   D, _p(d_img, torch.bfloat16), _p(d_txt, torch.bfloat16), _stream()), "toist_sweep_assemble_bwd")
    return d_img, d_txt


# -- the mask head of a sweep: per-image terms found through the pair table (csrc/maskstage.hip, csrc/segm.hip, csrc/sweep.hip).  All three share the
# status word of sweep_assemble (sweep_check reads and clears it) and its rule for a table entry outside [0, n_images): never an index, a zero term
def _pair_table(what, pair_image, pairs):
    if not pair_image.is_cuda or pair_image.dtype != torch.int32 or pair_image.dim() != 1 or pair_image.numel() != pairs or not pair_image.is_contiguous():
        raise ValueError(f"{what}: pair_image is a contiguous int32 vector of {pairs} entries on the device (got {pair_image.dtype} {tuple(pair_image.shape)})")
    status = sweep_status(pair_image.device)
    if status is None:
        raise RuntimeError(f"{what}: the first sweep launch on a device cannot be captured (its status word is allocated outside any graph)")
    return status


def mask_stage_fwd_pairs(src, src_stats, gamma, beta, fpn_conv, w, bias, out, out_stats, N, Q, H, W, c_in, c_out, w_rows, gn_in, up, pair_image, eps=1e-5):
    """mask_stage_fwd for the maps of a sweep's pairs (include/toist_hip.h: toist_mask_stage_fwd_pairs): fpn_conv is [n_images, H, W, c_out] and map n adds
    the term of image pair_image[n // Q] (int32 [N // Q] ON THE DEVICE).  The two `up` stages, (64 -> 32) and (32 -> 16, gn_in); out_lay has no image
    term and keeps mask_stage_fwd.  Shapes and contiguity are checked here, before the launch (ValueError)."""
    what = "mask_stage_fwd_pairs"
    N, Q, H, W = int(N), int(Q), int(H), int(W)
    if not up or (c_in, c_out, bool(gn_in)) not in ((64, 32, False), (32, 16, True)) or w_rows != c_out:
        raise ValueError(f"{what}: the stages with an image term are (64, 32, up) and (32, 16, gn_in, up) (got c_in {c_in}, c_out {c_out}, w_rows {w_rows}, gn_in {gn_in}, up {up})")
    if N <= 0 or Q <= 0 or N % Q or H <= 0 or W <= 0 or H % 2 or W % 2:
        raise ValueError(f"{what}: N = {N} maps of Q = {Q} per pair at {H} x {W}: N % Q == 0 and even sizes")
    if fpn_conv.dim() != 4 or tuple(fpn_conv.shape[1:]) != (H, W, c_out) or fpn_conv.shape[0] < 1:
        raise ValueError(f"{what}: fpn_conv is [n_images, {H}, {W}, {c_out}] (got {tuple(fpn_conv.shape)})")
    if src.numel() != N * (H // 2) * (W // 2) * c_in or out.numel() != N * H * W * c_out or out_stats.numel() != N * 16 or tuple(w.shape) != (c_out, 3, 3, c_in):
        raise ValueError(f"{what}: src [{N}, {H // 2}, {W // 2}, {c_in}], w [{c_out}, 3, 3, {c_in}], out [{N}, {H}, {W}, {c_out}] and out_stats [{N}, 8, 2] "
                         f"(got {tuple(src.shape)}, {tuple(w.shape)}, {tuple(out.shape)}, {tuple(out_stats.shape)})")
    if gn_in and (src_stats is None or src_stats.numel() != N * 16 or gamma is None or gamma.numel() != c_in or beta is None or beta.numel() != c_in):
        raise ValueError(f"{what}: gn_in needs src_stats [{N}, 8, 2] and gamma / beta [{c_in}]")
    if bias is not None and bias.numel() != c_out:
        raise ValueError(f"{what}: bias is [{c_out}]")
    for t in (src, src_stats, gamma, beta, fpn_conv, w, bias, out, out_stats):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{what}: every tensor must be contiguous")
    status = _pair_table(what, pair_image, N // Q)
    _lib.check(_lib.lib().toist_mask_stage_fwd_pairs(_p(src, BF16), _p(src_stats, F32), _p(gamma, F32), _p(beta, F32), _p(fpn_conv, BF16), _p(w, BF16),
                                                     _p(bias, F32), _p(out, BF16), _p(out_stats, F32), N, Q, H, W, c_in, c_out, w_rows, 1 if gn_in else 0,
                                                     1, eps, _p(pair_image, torch.int32), int(fpn_conv.shape[0]), _p(status, torch.int32), _stream()),
               "toist_mask_stage_fwd_pairs")


def resize_add_pairs(inp, fpn, pair_image, n, Q, H, W, OH, OW, C, out):
    """resize_add (rows = None) for the maps of a sweep's pairs (include/toist_hip.h: toist_resize_add_pairs): out [n, OH, OW, C] = fpn[pair_image[map // Q]]
    + nearest-resized inp [n, H, W, C]; fpn holds n_images terms of OH * OW * C elements, pair_image int32 [n // Q] ON THE DEVICE."""
    what = "resize_add_pairs"
    n, Q, H, W, OH, OW, C = (int(v) for v in (n, Q, H, W, OH, OW, C))
    if n <= 0 or Q <= 0 or n % Q or H <= 0 or W <= 0 or OH < H or OW < W or C <= 0 or C % 8:
        raise ValueError(f"{what}: n = {n} maps of Q = {Q} per pair, {H} x {W} -> {OH} x {OW}, C = {C}: n % Q == 0, a target no smaller than the source, C % 8 == 0")
    per = OH * OW * C
    if inp.numel() != n * H * W * C or out.numel() != n * per or fpn.numel() == 0 or fpn.numel() % per:
        raise ValueError(f"{what}: inp [{n}, {H}, {W}, {C}], fpn [n_images, {OH}, {OW}, {C}] and out [{n}, {OH}, {OW}, {C}] "
                         f"(got {tuple(inp.shape)}, {tuple(fpn.shape)}, {tuple(out.shape)})")
    if not (inp.is_contiguous() and fpn.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"{what}: every tensor must be contiguous")
    status = _pair_table(what, pair_image, n // Q)
    _lib.check(_lib.lib().toist_resize_add_pairs(_p(inp, BF16), _p(fpn, BF16), _p(pair_image, torch.int32), fpn.numel() // per, n, Q, H, W, OH, OW, C,
                                                 _p(out, BF16), _p(status, torch.int32), _stream()), "toist_resize_add_pairs")


def resize_add_rows_pairs(inp, fpn, rows, pair_image, n, Q, H, W, OH, OW, C, out):
    """resize_add on a gathered subset of the maps of P pairs (include/toist_hip.h: toist_resize_add_rows_pairs): map i is map rows[i] (int64 [n] ON THE
    DEVICE) of the P * Q maps, out [n, OH, OW, C] = fpn[pair_image[rows[i] // Q]] + nearest-resized inp [n, H, W, C]; n need not be a multiple of Q."""
    what = "resize_add_rows_pairs"
    n, Q, H, W, OH, OW, C = (int(v) for v in (n, Q, H, W, OH, OW, C))
    if n <= 0 or Q <= 0 or H <= 0 or W <= 0 or OH < H or OW < W or C <= 0 or C % 8:
        raise ValueError(f"{what}: n = {n} maps, Q = {Q} per pair, {H} x {W} -> {OH} x {OW}, C = {C}: positive extents, a target no smaller than the source, C % 8 == 0")
    if inp is None or fpn is None or rows is None or out is None or pair_image is None:
        raise ValueError(f"{what}: inp, fpn, rows, pair_image and out are required")
    per = OH * OW * C
    if inp.numel() != n * H * W * C or out.numel() != n * per or fpn.numel() == 0 or fpn.numel() % per:
        raise ValueError(f"{what}: inp [{n}, {H}, {W}, {C}], fpn [n_images, {OH}, {OW}, {C}] and out [{n}, {OH}, {OW}, {C}] "
                         f"(got {tuple(inp.shape)}, {tuple(fpn.shape)}, {tuple(out.shape)})")
    if rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() != n:
        raise ValueError(f"{what}: rows is an int64 vector of {n} entries (got {rows.dtype} {tuple(rows.shape)})")
    if not (inp.is_contiguous() and fpn.is_contiguous() and out.is_contiguous() and rows.is_contiguous()):
        raise ValueError(f"{what}: every tensor must be contiguous")
    P = int(pair_image.numel())
    status = _pair_table(what, pair_image, P)
    if P <= 0:
        raise ValueError(f"{what}: an empty pair table")
    _lib.check(_lib.lib().toist_resize_add_rows_pairs(_p(inp, BF16), _p(fpn, BF16), _p(rows, torch.int64), _p(pair_image, torch.int32), fpn.numel() // per, P,
                                                      n, Q, H, W, OH, OW, C, _p(out, BF16), _p(status, torch.int32), _stream()), "toist_resize_add_rows_pairs")


def sum_maps_by_image(inp, seg, pair_image, Q, n_images, per, out):
    """out [n_images, per] = per image the sum of the maps of its pairs (include/toist_hip.h: toist_sum_maps_by_image): inp bf16 [rows, per]; pair p's
    maps are rows [seg[p], seg[p + 1]) (seg int32 [P + 1] ON THE DEVICE) or [p Q, (p + 1) Q) with seg = None; pair_image int32 [P] ON THE DEVICE.
    fp32 sums in ascending pair and map order, rounded once: the same bits every run."""
    what = "sum_maps_by_image"
    Q, n_images, per = int(Q), int(n_images), int(per)
    if inp is None or out is None or pair_image is None:
        raise ValueError(f"{what}: inp, pair_image and out are required")
    if Q <= 0 or n_images <= 0 or per <= 0 or per % 8:
        raise ValueError(f"{what}: Q = {Q}, n_images = {n_images}, per = {per}: positive extents and per % 8 == 0")
    if inp.numel() == 0 or inp.numel() % per or out.numel() != n_images * per:
        raise ValueError(f"{what}: inp [rows, {per}] and out [{n_images}, {per}] (got {tuple(inp.shape)}, {tuple(out.shape)})")
    if not (inp.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"{what}: every tensor must be contiguous")
    P = int(pair_image.numel())
    if P <= 0:
        raise ValueError(f"{what}: an empty pair table")
    status = _pair_table(what, pair_image, P)
    if seg is not None and (seg.dtype != torch.int32 or seg.dim() != 1 or seg.numel() != P + 1 or not seg.is_contiguous() or not seg.is_cuda):
        raise ValueError(f"{what}: seg is a contiguous int32 vector of {P + 1} entries on the device (got {seg.dtype} {tuple(seg.shape)})")
    _lib.check(_lib.lib().toist_sum_maps_by_image(_p(inp, BF16), _p(seg, torch.int32), _p(pair_image, torch.int32), P, Q, n_images, inp.numel() // per, per,
                                                  _p(out, BF16), _p(status, torch.int32), _stream()), "toist_sum_maps_by_image")
    return out


def sweep_gather(src, pair_image, out=None):
    """out[p] = src[pair_image[p]] in one launch (include/toist_hip.h: toist_sweep_gather): src [n_images, ...] of any dtype, row size and alignment,
    pair_image int32 [P] ON THE DEVICE -> [P, ...]; `out` = such a tensor to write into.  Every output byte is written; a refused pair's row is zeros
    and the status word says so (sweep_check) -- unlike torch.index_select, whose device-side assert aborts the process."""
    what = "sweep_gather"
    if src.dim() < 1 or src.shape[0] < 1 or not src.is_contiguous():
        raise ValueError(f"{what}: src is a contiguous [n_images, ...] tensor (got {tuple(src.shape)})")
    P = int(pair_image.numel())
    shape = (P,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
    if tuple(out.shape) != shape or out.dtype != src.dtype or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"{what}: out is a contiguous {src.dtype} tensor of shape {shape} beside src (got {out.dtype} {tuple(out.shape)})")
    row_bytes = src[0].numel() * src.element_size()
    if row_bytes <= 0:
        raise ValueError(f"{what}: rows of no bytes")
    status = _pair_table(what, pair_image, P)
    _lib.check(_lib.lib().toist_sweep_gather(_p(src), _p(pair_image, torch.int32), int(src.shape[0]), P, row_bytes, _p(out), _p(status, torch.int32),
                                             _stream()), "toist_sweep_gather")
    return out


def mask_pack(dense):
    """[n, h, w] bool / uint8 -> bit planes."""
    n, h, w = dense.shape
    src = dense.contiguous().view(torch.uint8) if dense.dtype == torch.bool else dense.contiguous()
    bits = _plane(n, h, w, dense.device)
    _lib.check(_lib.lib().toist_mask_pack(_p(src, torch.uint8), n, h, w, _p(bits), _stream()), "toist_mask_pack")
    return bits


def mask_unpack(bits, h, w):
    n = bits.shape[0]
    dense = torch.empty(n, h, w, dtype=torch.uint8, device=bits.device)
    _lib.check(_lib.lib().toist_mask_unpack(_p(bits, torch.int64), n, h, w, _p(dense), _stream()), "toist_mask_unpack")
    return dense.view(torch.bool)


def mask_area(bits, h, w):
    area = torch.empty(bits.shape[0], dtype=torch.int32, device=bits.device)
    _lib.check(_lib.lib().toist_mask_area(_p(bits, torch.int64), bits.shape[0], h, w, _p(area), _stream()), "toist_mask_area")
    return area


def mask_iou(dt, gt, iscrowd, area_dt, area_gt, h, w):
    """[n_dt, n_gt] float64 IoU of two sets of bit planes (crowd ground truth: union = detection area)."""
    iou = torch.zeros(dt.shape[0], gt.shape[0], dtype=torch.float64, device=dt.device)
    _lib.check(_lib.lib().toist_mask_iou(_p(dt, torch.int64), dt.shape[0], _p(gt, torch.int64), gt.shape[0], _p(iscrowd, torch.uint8),
                                         _p(area_dt, torch.int32), _p(area_gt, torch.int32), h, w, _p(iou), _stream()), "toist_mask_iou")
    return iou


def mask_rle(bits, h, w):
    """Run lengths of every plane, zeros first (mask_util.encode's counts): (counts int32 [total], first_run int64 [n + 1])."""
    n = bits.shape[0]
    trans = torch.empty(n, w, dtype=torch.int32, device=bits.device)
    _lib.check(_lib.lib().toist_mask_rle_count(_p(bits, torch.int64), n, h, w, _p(trans), _stream()), "toist_mask_rle_count")
    ends = torch.cumsum(trans.view(-1).to(torch.int64), 0)
    col_off = ends - trans.view(-1)
    first_pos = torch.zeros(n + 1, dtype=torch.int64, device=bits.device)
    first_pos[1:] = ends.view(n, w)[:, -1]
    first_run = first_pos + torch.arange(n + 1, device=bits.device)
    total = int(first_pos[-1])                       # the one synchronisation: sizes the output
    pos = torch.empty(max(total, 1), dtype=torch.int32, device=bits.device)
    _lib.check(_lib.lib().toist_mask_rle_emit(_p(bits, torch.int64), n, h, w, _p(col_off), _p(pos), _stream()), "toist_mask_rle_emit")
    counts = torch.empty(total + n, dtype=torch.int32, device=bits.device)
    _lib.check(_lib.lib().toist_mask_rle_counts(_p(pos), _p(first_pos), _p(first_run), n, h, w, _p(counts), _stream()), "toist_mask_rle_counts")
    return counts, first_run


def coco_match(iou, iou_off, dt_area, dt_off, gt_area, gt_ignore, gt_crowd, gt_off, area_rng, thrs):
    """Batched COCOeval.evaluateImg (csrc/evalmask.hip): -> (dt_match int32, dt_ignore uint8) flat [sum_i A*T*D_i],
    gt_range_ignore uint8 flat [sum_i A*G_i]; offsets are int64 device tensors with n_images + 1 entries."""
    n_img, A, T = dt_off.numel() - 1, area_rng.shape[0], thrs.numel()
    n_dt, n_gt = dt_area.numel(), gt_area.numel()
    dev = dt_off.device
    dt_match = torch.empty(A * T * n_dt, dtype=torch.int32, device=dev)
    dt_ignore = torch.empty(A * T * n_dt, dtype=torch.uint8, device=dev)
    gt_flag = torch.empty(A * n_gt, dtype=torch.uint8, device=dev)
    taken = torch.empty(A * T * n_gt, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().toist_coco_match(_p(iou, torch.float64), _p(iou_off, torch.int64), _p(dt_area, torch.float64), _p(dt_off, torch.int64),
                                           _p(gt_area, torch.float64), _p(gt_ignore, torch.uint8), _p(gt_crowd, torch.uint8), _p(gt_off, torch.int64),
                                           n_img, _p(area_rng, torch.float64), A, _p(thrs, torch.float64), T, _p(dt_match), _p(dt_ignore),
                                           _p(gt_flag), _p(taken), _stream()), "toist_coco_match")
    return dt_match, dt_ignore, gt_flag


COCO_BOXES_MAX_Q = _lib.CONSTANTS["TOIST_COCO_BOXES_MAX_Q"]     # queries per row that toist_coco_boxes ranks in LDS


def coco_boxes(scores, boxes, max_det, row_slot, slot_off, gt_xywh, gt_area, gt_crowd, iou_off, gt_off, n_iou, n_gt, out=None):
    """The box side of COCOeval for R PostProcess rows in one launch (include/toist_hip.h: toist_coco_boxes; csrc/evalbox.hip).  scores f32 [R, Q] and
    boxes f32 [R, Q, 4] = kernels.postprocess's buffers (or their first R rows), read in place; row_slot int32 [R]; the staged ground truth slot_off
    int64 [slots + 1], gt_xywh f64 [N, 4], gt_area f64 [N], gt_crowd uint8 [N]; iou_off / gt_off int64 [R + 1]: everything ON THE DEVICE.  n_iou, n_gt:
    host ints, the batch's totals iou_off[R] and gt_off[R] (they size the outputs; nothing is read back).
    -> dict(order int32 [R, D], dt_score f64 [R * D], dt_area f64 [R * D], iou f64 [>= n_iou], gt_area f64 [>= n_gt], gt_crowd uint8 [>= n_gt]),
    D = min(Q, max_det); `out` = such a dict to write into (fixed addresses for a captured graph; iou / gt_area / gt_crowd may be larger: a capacity).
    The tables are the caller's to check on the host (coco_eval.row_tables); the launch writes nothing outside the rows' extents."""
    for name, t in (("scores", scores), ("boxes", boxes), ("row_slot", row_slot), ("slot_off", slot_off), ("gt_xywh", gt_xywh), ("gt_area", gt_area),
                    ("gt_crowd", gt_crowd), ("iou_off", iou_off), ("gt_off", gt_off)):
        if not t.is_cuda:
            raise RuntimeError(f"coco_boxes: {name} is a CPU tensor; the kernel runs on the GPU and there is no CPU path")
        if not t.is_contiguous():
            raise ValueError(f"coco_boxes: {name} must be contiguous")
    if scores.dim() != 2 or tuple(boxes.shape) != (*scores.shape, 4):
        raise ValueError(f"coco_boxes: scores [R, Q] and boxes [R, Q, 4] (got {tuple(scores.shape)} and {tuple(boxes.shape)})")
    R, Q = scores.shape
    max_det, n_iou, n_gt = int(max_det), int(n_iou), int(n_gt)
    if Q > COCO_BOXES_MAX_Q:
        raise ValueError(f"coco_boxes: {Q} queries per row exceed the kernel's capacity of {COCO_BOXES_MAX_Q}")
    if max_det < 0 or n_iou < 0 or n_gt < 0:
        raise ValueError("coco_boxes: max_det, n_iou and n_gt are non-negative")
    D, N, dev = min(Q, max_det), gt_area.numel(), scores.device
    if row_slot.numel() != R or iou_off.numel() != R + 1 or gt_off.numel() != R + 1 or slot_off.numel() < 2:
        raise ValueError("coco_boxes: row_slot [R], iou_off / gt_off [R + 1] and slot_off [slots + 1] must match the rows")
    if tuple(gt_xywh.shape) != (N, 4) or gt_crowd.numel() != N:
        raise ValueError("coco_boxes: the staged ground truth is gt_xywh [N, 4], gt_area [N], gt_crowd [N]")
    if out is None:
        out = {"order": torch.empty(R, D, dtype=torch.int32, device=dev), "dt_score": torch.empty(R * D, dtype=torch.float64, device=dev),
               "dt_area": torch.empty(R * D, dtype=torch.float64, device=dev), "iou": torch.empty(n_iou, dtype=torch.float64, device=dev),
               "gt_area": torch.empty(n_gt, dtype=torch.float64, device=dev), "gt_crowd": torch.empty(n_gt, dtype=torch.uint8, device=dev)}
    if any(not out[name].is_contiguous() for name in ("order", "dt_score", "dt_area", "iou", "gt_area", "gt_crowd")):
        raise ValueError("coco_boxes: every output must be contiguous")
    if out["order"].numel() != R * D or out["dt_score"].numel() != R * D or out["dt_area"].numel() != R * D:
        raise ValueError(f"coco_boxes: order, dt_score and dt_area hold R * D = {R * D} elements")
    if out["iou"].numel() < n_iou or out["gt_area"].numel() < n_gt or out["gt_crowd"].numel() != out["gt_area"].numel():
        raise ValueError(f"coco_boxes: iou holds at least {n_iou} elements, gt_area and gt_crowd at least {n_gt} (and as many as each other)")
    ptr = lambda t, dtype: _p(t, dtype) if t.numel() else None
    _lib.check(_lib.lib().toist_coco_boxes(ptr(scores, torch.float32), ptr(boxes, torch.float32), R, Q, max_det, ptr(row_slot, torch.int32),
                                           _p(slot_off, torch.int64), slot_off.numel() - 1, ptr(gt_xywh, torch.float64), ptr(gt_area, torch.float64),
                                           ptr(gt_crowd, torch.uint8), N, _p(iou_off, torch.int64), _p(gt_off, torch.int64), out["iou"].numel(),
                                           out["gt_area"].numel(), ptr(out["order"], torch.int32), ptr(out["dt_score"], torch.float64),
                                           ptr(out["dt_area"], torch.float64), ptr(out["iou"], torch.float64), ptr(out["gt_area"], torch.float64),
                                           ptr(out["gt_crowd"], torch.uint8), _stream()), "toist_coco_boxes")
    return out


COCO_MASKS_CHUNK_WORDS = _lib.CONSTANTS["TOIST_COCO_MASKS_CHUNK_WORDS"]     # words of a detection plane toist_coco_masks holds in LDS at a time


def coco_masks(bits, capacity_words, row_hw, Q, order, row_slot, slot_off, gt_bits, gt_plane_off, slot_hw, gt_parea, gt_crowd, iou_off, n_iou, out=None):
    """The mask side of COCOeval for R rows in one launch (include/toist_hip.h: toist_coco_masks; csrc/evalrows.hip).  bits int64 [>= R *
    capacity_words]: row r's Q planes [Q, w_r, ceil(h_r/64)] from word r * capacity_words (CapturedEvalStep's buffer); row_hw int64 [R, 2] = (h, w);
    order int32 [R, D] = coco_boxes' ranking; row_slot int32 [R]; slot_off int64 [slots + 1]; the staged planes gt_bits int64 [words], gt_plane_off int64
    [N + 1], slot_hw int32 [slots, 2], gt_parea int32 [N] (popcounts), gt_crowd uint8 [N]; iou_off int64 [R + 1]: everything ON THE DEVICE.  n_iou: the
    host int iou_off[R] (it sizes the output; nothing is read back).
    -> dict(dt_area f64 [R * D], iou f64 [>= n_iou]); `out` = such a dict to write into (fixed addresses for a captured graph; iou may be larger).
    The tables are the caller's to check on the host (coco_eval.mask_row_tables); the launch writes nothing outside the rows' extents."""
    for name, t in (("bits", bits), ("row_hw", row_hw), ("order", order), ("row_slot", row_slot), ("slot_off", slot_off), ("gt_bits", gt_bits),
                    ("gt_plane_off", gt_plane_off), ("slot_hw", slot_hw), ("gt_parea", gt_parea), ("gt_crowd", gt_crowd), ("iou_off", iou_off)):
        if not t.is_cuda:
            raise RuntimeError(f"coco_masks: {name} is a CPU tensor; the kernel runs on the GPU and there is no CPU path")
        if not t.is_contiguous():
            raise ValueError(f"coco_masks: {name} must be contiguous")
    if order.dim() != 2 or row_hw.dim() != 2 or tuple(row_hw.shape) != (order.shape[0], 2):
        raise ValueError(f"coco_masks: order [R, D] and row_hw [R, 2] (got {tuple(order.shape)} and {tuple(row_hw.shape)})")
    R, D = order.shape
    Q, capacity_words, n_iou = int(Q), int(capacity_words), int(n_iou)
    N, S, dev = gt_crowd.numel(), slot_off.numel() - 1, bits.device
    if Q < D or capacity_words < 0 or n_iou < 0:
        raise ValueError(f"coco_masks: {D} kept detections of {Q} queries, capacity_words = {capacity_words}, n_iou = {n_iou}")
    if bits.numel() < R * capacity_words:
        raise ValueError(f"coco_masks: bits holds {bits.numel()} words, {R} x {capacity_words} are needed")
    if row_slot.numel() != R or iou_off.numel() != R + 1 or S < 1 or tuple(slot_hw.shape) != (S, 2):
        raise ValueError("coco_masks: row_slot [R], iou_off [R + 1], slot_off [slots + 1] and slot_hw [slots, 2] must match the rows and each other")
    if gt_plane_off.numel() != N + 1 or gt_parea.numel() != N:
        raise ValueError("coco_masks: the staged planes are gt_plane_off [N + 1], gt_parea [N], gt_crowd [N]")
    if out is None:
        out = {"dt_area": torch.empty(R * D, dtype=torch.float64, device=dev), "iou": torch.empty(n_iou, dtype=torch.float64, device=dev)}
    if not out["dt_area"].is_contiguous() or not out["iou"].is_contiguous() or out["dt_area"].numel() != R * D or out["iou"].numel() < n_iou:
        raise ValueError(f"coco_masks: contiguous outputs, dt_area of R * D = {R * D} elements and iou of at least {n_iou}")
    ptr = lambda t, dtype: _p(t, dtype) if t.numel() else None
    _lib.check(_lib.lib().toist_coco_masks(ptr(bits, torch.int64), capacity_words, ptr(row_hw, torch.int64), R, Q, D, ptr(order, torch.int32),
                                           ptr(row_slot, torch.int32), _p(slot_off, torch.int64), S, ptr(gt_bits, torch.int64), gt_bits.numel(),
                                           ptr(gt_plane_off, torch.int64), _p(slot_hw, torch.int32), ptr(gt_parea, torch.int32), ptr(gt_crowd, torch.uint8),
                                           N, _p(iou_off, torch.int64), out["iou"].numel(), ptr(out["dt_area"], torch.float64),
                                           ptr(out["iou"], torch.float64), _stream()), "toist_coco_masks")
    return out
