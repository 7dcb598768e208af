"""Plain fp64 restatement of the post-norm decoder layer stack that `toist_xdec_desc` (include/toist_hip.h) describes: test infrastructure,
CPU torch, written from the descriptor's comments and oracle/model_ref.py decoder_layer -- not from the kernels' code.

Inputs are the descriptor's: x0 / qpos [B*Q, 256], the pre-projected memory kv [B*S, >= L*512] (layer l: K at columns l*512, V at l*512 + 256),
key_pad [B, S] (non-zero = padding) and per layer a dict with the 18 parameter tensors under the descriptor's names plus "seed" (6 ints: self-attention,
norm1 branch, cross-attention, norm3 branch, hidden, norm4 branch).  Every tensor the launch saves comes back under the descriptor's field name,
stacked over the layers.  Row statistics of the attentions are (maximum of the raw dot products over live keys, 1 / sum exp(scale (s - max))).

Dropout masks are the kernels' two counter hashes restated in integer torch ops: `pair_hash` (csrc/common.h: one 32-bit value per two adjacent keys
of a score row, pair index (row * round8(Sk) + key) >> 1) and `hash_u32` (csrc/common.h: element m * 256 + n of a [M, 256] tensor, m * 2048 + n of
the hidden activations).

  layer_stages   teacher-forced: every stage in fp64 from GIVEN (already rounded) inputs of that stage
  forward        free-running fp64, differentiable: torch.autograd gives every gradient the backward launch exports (`taps`)
  forward(..., round_stores=True)   the rounding model: the same graph with a straight-through bf16 rounding wherever the launches store bf16 --
                 the saved tensors, the probabilities entering P v, the 32 partial sums of linear2 (one per 64 hidden units), and in the backward
                 direction the exported gradients, the partial sums of dh W1, the dq shares of the 128-key splits and the score gradients.
                 It only sizes tolerances: e_model = relF(forward(round_stores=True), forward()).
  backward_stages   teacher-forced backward chain at p = 0 from given exports
"""
import math

import torch

D, H, DH, FF = 256, 8, 32, 2048
SCALE = 1.0 / math.sqrt(DH)
EPS = 1e-5
M32 = 0xFFFFFFFF
F64 = torch.float64
SAVED = ("qkv", "ctx_s", "lse_s", "z1", "mean1", "rstd1", "y1", "y1e", "qc", "ctx_c", "lse_c", "z3", "mean3", "rstd3", "y3", "h", "z4", "mean4", "rstd4",
         "y4", "y4e")
PARAMS = ("w_in", "b_in", "w_os", "b_os", "g1", "be1", "w_q", "b_q", "w_oc", "b_oc", "g3", "be3", "w1", "b1", "w2", "b2", "g4", "be4")


# ------------------------------------------------------------------------------------------------------------------ dropout hashes
def pair_hash(pair, seed):
    """csrc/common.h pair_hash in int64 arithmetic (values kept below 2^32)"""
    s0 = seed & M32
    s1 = ((seed >> 32) ^ ((seed & M32) * 0x9E3779B9)) & M32
    a = (pair ^ s0) & M32
    a = a ^ (a >> 12)
    h = ((a & 0xFFFFFF) * 0x9E3779 + s1) & M32
    h = h ^ (h >> 15)
    h = ((h & 0xFFFFFF) * 0x85EBCB + (a >> 8)) & M32
    h = h ^ (h >> 13)
    return h


def attn_keep(BH, Sq, Sk, p, seed):
    """keep mask [BH, Sq, Sk] of the attention probabilities: 16-bit field (key parity) of the pair hash >= round(p * 2^16)"""
    ldp = (Sk + 7) // 8 * 8
    row = torch.arange(BH * Sq, dtype=torch.int64).view(BH, Sq, 1)
    key = torch.arange(Sk, dtype=torch.int64).view(1, 1, Sk)
    idx = row * ldp + key
    h = pair_hash(idx >> 1, seed)
    field = torch.where((key & 1) == 1, h >> 16, h & 0xFFFF)
    return field >= int(p * 65536.0 + 0.5)


def _mul32(x, c):
    """(x * c) mod 2^32 for 0 <= x, c < 2^32 without leaving int64"""
    return ((x & 0xFFFF) * c + ((((x >> 16) * c) & 0xFFFF) << 16)) & M32


def hash_u32(seed, idx):
    """csrc/common.h hash_u32 for element indices below 2^32 (int64 tensor) and a 64-bit seed (Python int)"""
    x = (idx ^ (seed & M32)) & M32
    key = ((seed >> 32) ^ ((seed & M32) * 0x9E3779B9)) & M32
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ key
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    x = x ^ (x >> 16)
    return x


def elem_keep(M, N, p, seed):
    """keep mask [M, N] of a row-major tensor: hash of element m * N + n >= (unsigned)(p * 2^32), p a C float"""
    thresh = int(float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0)
    idx = torch.arange(M * N, dtype=torch.int64).view(M, N)
    return hash_u32(seed, idx) >= thresh


# ------------------------------------------------------------------------------------------------------------------ rounding model
class _Ste(torch.autograd.Function):
    """bf16 rounding of a stored value, straight-through gradient"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """identity whose gradient is rounded to bf16: a gradient the backward launch stores"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _same(x):
    return x


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


# ------------------------------------------------------------------------------------------------------------------ stages
def _heads(t, B, S):
    return t.view(B, S, H, DH).permute(0, 2, 1, 3)


def st_qkv(x, xe, P):
    """q | k = (x + query_pos) W_in[:512]^T, v = x W_in[512:]^T, + bias"""
    return torch.cat([xe @ P["w_in"][:2 * D].t(), x @ P["w_in"][2 * D:].t()], dim=1) + P["b_in"]


def st_attn(q, k, v, dead, B, Sq, Sk, p, seed, rnd=_same, rg=None):
    """softmax(scale q k^T, padded keys at -inf) -> dropout -> P v per head.  q [B*Sq, 256], k / v [B*Sk, 256], dead [B, Sk] bool or None.
    Returns the context [B*Sq, 256] and the statistics [B*8, Sq, 2]."""
    qh, kh, vh = _heads(q, B, Sq), _heads(k, B, Sk), _heads(v, B, Sk)
    if rg is None:
        raw = qh @ kh.transpose(-1, -2)
    else:        # the backward launch forms dq as one bf16 share per 128-key split, and rounds the score gradients
        raw = rg(torch.cat([rg(qh) @ kh[:, :, c:c + 128].transpose(-1, -2) for c in range(0, Sk, 128)], dim=-1))
    if dead is not None:
        raw = raw.masked_fill(dead.view(B, 1, 1, Sk), float("-inf"))
    m = raw.detach().amax(-1, keepdim=True)
    e = torch.exp((raw - m) * SCALE)
    l = e.sum(-1, keepdim=True)
    if p > 0:
        e = e * attn_keep(B * H, Sq, Sk, p, seed).view(B, H, Sq, Sk)
    ctx = (rnd(e) @ vh) / l / (1.0 - p)
    lse = torch.cat([m, 1.0 / l.detach()], dim=-1).reshape(B * H, Sq, 2)
    return ctx.permute(0, 2, 1, 3).reshape(B * Sq, D), lse


def st_drop(t, p, seed, rgf=_same):
    """dropout of a [M, 256] sub-layer branch (rgf: the branch gradient gb4 / go3 / go1 is a bf16 store of the backward launch)"""
    t = rgf(t)
    return t * elem_keep(t.shape[0], D, p, seed) / (1.0 - p) if p > 0 else t


def st_branch(a, w, b, p, seed, rgf=_same):
    """dropout(a W^T + b); returns (pre-dropout, post-dropout)"""
    t = a @ w.t() + b
    return t, st_drop(t, p, seed, rgf)


def st_stats(z):
    mean = z.mean(1)
    rstd = ((z - mean[:, None]) ** 2).mean(1).add(EPS).rsqrt()
    return mean, rstd


def st_norm(z, mean, rstd, gamma, beta):
    return (z - mean[:, None]) * rstd[:, None] * gamma + beta


def st_hidden(y3, P, p, seed, rg=None):
    """dropout(relu(y3 W1^T + b1)); returns (pre-activation, h)"""
    if rg is None:
        a = y3 @ P["w1"].t() + P["b1"]
    else:        # the backward launch folds 32 bf16 partial sums of dh W1, one per 64 hidden units
        a = rg(torch.cat([rg(y3) @ P["w1"][c:c + 64].t() for c in range(0, FF, 64)], dim=1) + P["b1"])
    h = torch.relu(a)
    if p > 0:
        h = h * elem_keep(h.shape[0], FF, p, seed) / (1.0 - p)
    return a, h


def st_linear2(h, P, rnd=_same, partials=False):
    """h W2^T; partials: as the sum of 32 bf16-rounded partial sums (64 hidden units each), the launch's `part` scratch"""
    if not partials:
        return h @ P["w2"].t()
    return sum(rnd(h[:, c:c + 64] @ P["w2"][:, c:c + 64].t()) for c in range(0, FF, 64))


def st_linear2_bounds(h, P):
    """(lo, hi) around st_linear2(partials=True) for ANY fp32 accumulation order: a 64-term partial sum formed in fp32 lies within 64 * 2^-24 * sum |h w| of the
    exact one, so where that interval straddles a bf16 rounding boundary the stored partial may be either neighbour (one partial ulp, up to 2e-3 here: more
    than the stage's absolute tolerance).  bf16 rounding is monotone, so rounding the interval's ends brackets every admissible stored value."""
    lo = hi = 0.0
    for c in range(0, FF, 64):
        s = h[:, c:c + 64] @ P["w2"][:, c:c + 64].t()
        d = (h[:, c:c + 64].abs() @ P["w2"][:, c:c + 64].abs().t()) * (64.0 * 2.0 ** -24)
        lo, hi = lo + bf16(s - d), hi + bf16(s + d)
    return lo, hi


def _dead(key_pad):
    return None if key_pad is None else key_pad.bool()


def layer_stages(sv, x_in, xe_in, qpos, kv_l, key_pad, P, p, B, Q, S, last, round_partials=False, round_probs=False):
    """Teacher-forced expectations of one layer.  sv: the launch's saved tensors of this layer (fp64), x_in / xe_in: the rows entering the layer
    (x0 / qpos for layer 0, y4 / y4e of the layer below otherwise), kv_l = (K, V) [B*S, 256] of this layer.  Every stage reads the GIVEN tensors of
    the stage before it; statistics are those of the given (rounded) pre-norm rows.  round_partials / round_probs: the two bf16 roundings INSIDE a stage (the 32 partial sums of linear2, the
    probabilities entering P v) as the rounding model has them; round_partials="bounds": z4 comes back as (lo, hi), see st_linear2_bounds.  y4e is absent for the last layer, as in the launch."""
    seed = P["seed"]
    rp = bf16 if round_probs else _same
    dead = _dead(key_pad)
    o = {}
    o["qkv"] = st_qkv(x_in, xe_in, P)
    o["ctx_s"], o["lse_s"] = st_attn(sv["qkv"][:, :D], sv["qkv"][:, D:2 * D], sv["qkv"][:, 2 * D:], None, B, Q, Q, p, seed[0], rp)
    o["z1"] = st_branch(sv["ctx_s"], P["w_os"], P["b_os"], p, seed[1])[1] + x_in
    o["mean1"], o["rstd1"] = st_stats(sv["z1"])
    o["y1"] = st_norm(sv["z1"], o["mean1"], o["rstd1"], P["g1"], P["be1"])
    o["y1e"] = sv["y1"] + qpos
    o["qc"] = sv["y1e"] @ P["w_q"].t() + P["b_q"]
    o["ctx_c"], o["lse_c"] = st_attn(sv["qc"], kv_l[0], kv_l[1], dead, B, Q, S, p, seed[2], rp)
    o["z3"] = st_branch(sv["ctx_c"], P["w_oc"], P["b_oc"], p, seed[3])[1] + sv["y1"]
    o["mean3"], o["rstd3"] = st_stats(sv["z3"])
    o["y3"] = st_norm(sv["z3"], o["mean3"], o["rstd3"], P["g3"], P["be3"])
    o["h"] = st_hidden(sv["y3"], P, p, seed[4])[1]
    if round_partials == "bounds":        # z4 as an interval (lo, hi): dropout scales by a non-negative factor, bias and residual shift both ends
        o["z4"] = tuple(st_drop(t + P["b2"], p, seed[5]) + sv["y3"] for t in st_linear2_bounds(sv["h"], P))
    else:
        o["z4"] = st_drop(st_linear2(sv["h"], P, bf16, round_partials) + P["b2"], p, seed[5]) + sv["y3"]
    o["mean4"], o["rstd4"] = st_stats(sv["z4"])
    o["y4"] = st_norm(sv["z4"], o["mean4"], o["rstd4"], P["g4"], P["be4"])
    if not last:
        o["y4e"] = sv["y4"] + qpos
    return o


def forward(x0, qpos, kv, key_pad, layers, p, B, Q, S, round_stores=False):
    """Free-running fp64 stack.  Returns (out, taps): out[name] = [L, ...] stacked saved tensors (y4e of the last layer is absent from the
    launch: it is returned as y4 + qpos all the same), taps[name][l] = the graph tensors whose autograd gradients are the backward launch's exports
    (t4 -> gb4, a1 -> dh, t3 -> go3, t1 -> go1, qkv -> sink[:, :768], qc -> sink[:, 768:]).  x0 enters twice in `taps`: "x_proj" (the in_proj path
    of layer 0) and "x_res" (the residual path)."""
    rnd = _Ste.apply if round_stores else _same
    rg = _RoundGrad.apply if round_stores else None
    rgf = rg if round_stores else _same
    dead = _dead(key_pad)
    out = {n: [] for n in SAVED}
    taps = {n: [] for n in ("t4", "a1", "t3", "t1", "qkv", "qc")}
    x_proj, x_res = x0.view_as(x0), x0.view_as(x0)
    taps["x_proj"], taps["x_res"] = x_proj, x_res
    x_p, x, xe = x_proj, x_res, rnd(x_proj + qpos)          # xe0 of the descriptor: a bf16 tensor of the caller
    for li, P in enumerate(layers):
        seed = P["seed"]
        col = li * 2 * D
        kmat, vmat = rgf(kv[:, col:col + D]), rgf(kv[:, col + D:col + 2 * D])
        qkv_t = st_qkv(x_p, xe, P)
        qkv = rgf(rnd(qkv_t))
        ctx_s, lse_s = st_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], None, B, Q, Q, p, seed[0], rnd, rg)
        ctx_s = rgf(rnd(ctx_s))
        t1, t1d = st_branch(ctx_s, P["w_os"], P["b_os"], p, seed[1], rgf)
        z1 = rgf(rnd(t1d + x))
        mean1, rstd1 = st_stats(z1)
        y1 = rnd(st_norm(z1, mean1, rstd1, P["g1"], P["be1"]))
        y1e = rnd(y1 + qpos)
        qc_t = y1e @ P["w_q"].t() + P["b_q"]
        qc = rgf(rnd(qc_t))
        ctx_c, lse_c = st_attn(qc, kmat, vmat, dead, B, Q, S, p, seed[2], rnd, rg)
        ctx_c = rgf(rnd(ctx_c))
        t3, t3d = st_branch(ctx_c, P["w_oc"], P["b_oc"], p, seed[3], rgf)
        z3 = rgf(rnd(t3d + y1))
        mean3, rstd3 = st_stats(z3)
        y3 = rnd(st_norm(z3, mean3, rstd3, P["g3"], P["be3"]))
        a1, h = st_hidden(y3, P, p, seed[4], rg)
        h = rnd(h)
        t4 = st_linear2(h, P, rnd, round_stores) + P["b2"]
        t4d = st_drop(t4, p, seed[5], rgf)
        z4 = rgf(rnd(t4d + y3))
        mean4, rstd4 = st_stats(z4)
        y4 = rnd(st_norm(z4, mean4, rstd4, P["g4"], P["be4"]))
        y4e = rnd(y4 + qpos)
        for n, t in (("qkv", qkv), ("ctx_s", ctx_s), ("lse_s", lse_s), ("z1", z1), ("mean1", mean1), ("rstd1", rstd1), ("y1", y1), ("y1e", y1e), ("qc", qc),
                     ("ctx_c", ctx_c), ("lse_c", lse_c), ("z3", z3), ("mean3", mean3), ("rstd3", rstd3), ("y3", y3), ("h", h), ("z4", z4), ("mean4", mean4),
                     ("rstd4", rstd4), ("y4", y4), ("y4e", y4e)):
            out[n].append(t)
        for n, t in (("t4", t4), ("a1", a1), ("t3", t3), ("t1", t1), ("qkv", qkv_t), ("qc", qc_t)):
            taps[n].append(t)
        x_p, x, xe = y4, y4, y4e
    return {n: torch.stack(v) for n, v in out.items()}, taps


# ------------------------------------------------------------------------------------------------------------------ backward, teacher-forced (p = 0)
def ln_bwd(v, z, mean, rstd, gamma):
    """input gradient of y = (z - mean) rstd gamma + beta for the output gradient v"""
    xh = (z - mean[:, None]) * rstd[:, None]
    gg = v * gamma
    return rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))


def attn_bwd(q, k, v, dctx, dead, B, Sq, Sk):
    """(dq, dk, dv) of st_attn at p = 0 by autograd on fp64 leaves"""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ctx, _ = st_attn(q, k, v, dead, B, Sq, Sk, 0.0, 0)
    ctx.backward(dctx)
    return q.grad, k.grad, v.grad


def backward_stages(sv, ex, gy, kv_l, key_pad, P, B, Q, S, round_partials=False):
    """Teacher-forced expectations of one layer of the backward launch at p = 0.  sv: the forward launch's saved tensors of the layer, ex: the
    backward launch's exports of the layer (gb4, dh, go3, go1, sink [M, 1024], all fp64), gy: the gradient of the layer's output y4 (g_out[l] plus the
    layer above's input gradient, rebuilt by the caller from that layer's exports).  round_partials: dh W1 as the sum of the launch's 32 bf16 partial sums."""
    dead = _dead(key_pad)
    o = {}
    o["gb4"] = ln_bwd(gy, sv["z4"], sv["mean4"], sv["rstd4"], P["g4"])
    o["dh"] = (ex["gb4"] @ P["w2"]) * (sv["h"] > 0)
    dy3 = sum(bf16(ex["dh"][:, c:c + 64] @ P["w1"][c:c + 64]) for c in range(0, FF, 64)) if round_partials else ex["dh"] @ P["w1"]
    o["go3"] = ln_bwd(ex["gb4"] + dy3, sv["z3"], sv["mean3"], sv["rstd3"], P["g3"])
    dq, dk, dv = attn_bwd(sv["qc"], kv_l[0], kv_l[1], ex["go3"] @ P["w_oc"], dead, B, Q, S)
    o["dq_c"], o["dk_c"], o["dv_c"] = dq, dk, dv
    o["go1"] = ln_bwd(ex["sink"][:, 3 * D:] @ P["w_q"] + ex["go3"], sv["z1"], sv["mean1"], sv["rstd1"], P["g1"])
    dq, dk, dv = attn_bwd(sv["qkv"][:, :D], sv["qkv"][:, D:2 * D], sv["qkv"][:, 2 * D:], ex["go1"] @ P["w_os"], None, B, Q, Q)
    o["dqkv_s"] = torch.cat([dq, dk, dv], dim=1)
    return o


def input_grad(ex, P):
    """gradient of the rows entering a layer at p = 0, from the layer's exports: [dq | dk | dv] W_in + the residual gradient (go1 = norm1's input gradient)"""
    return ex["sink"][:, :3 * D] @ P["w_in"] + ex["go1"]


def relF(a, b, floor=0.0):
    """relative Frobenius error |a - b| / |b|.  floor: only for a reference that is ZERO up to fp64 cancellation (rms below 1e-12: the dq / dk of a softmax
    over a single key, of value rows that are all the same) -- its norm is then taken as `floor` per element, since fp32 kernels leave such a gradient
    as cancellation noise; every other tensor is divided by its own norm alone."""
    nb = float(b.norm())
    if floor > 0 and nb < 1e-12 * math.sqrt(b.numel()):
        nb = floor * math.sqrt(b.numel())
    return float((a - b).norm()) / (nb + 1e-300)


# ------------------------------------------------------------------------------------------------------------------ synthetic cases
# The smallest shapes at which each mechanism of the launches can go wrong (tests/test_gpu_xdec_reference.py runs them on the device,
# tests/test_cpu_xdec_reference.py pins the reference on them).  pad: none | tail | tail+mid (tail + one middle key; the LAST image keeps a single
# live key) | middle (a run of keys in the middle).
CASES = {
    "a": dict(B=1, Q=1, S=1, L=1, p=0.0, pad="none"),            # one live row, one key, 31 idle row owners, 7 empty XCD groups
    "b": dict(B=3, Q=30, S=17, L=2, p=0.1, pad="tail+mid"),      # ragged 4-row block, S not a multiple of 8 (round8(S) in the pair index)
    "c": dict(B=2, Q=128, S=64, L=1, p=0.0, pad="none"),         # every row owner full, exactly one key block
    "d": dict(B=2, Q=125, S=65, L=2, p=0.1, pad="tail"),         # last owner has 1 row; one key past a block
    "e128": dict(B=8, Q=100, S=128, L=1, p=0.1, pad="tail"),     # cross-attention backward key splits 1 ...
    "e129": dict(B=8, Q=100, S=129, L=1, p=0.1, pad="tail"),     # ... -> 2 (dq_part fold)
    "f256": dict(B=2, Q=100, S=256, L=1, p=0.0, pad="middle"),   # splits 2
    "f257": dict(B=2, Q=100, S=257, L=1, p=0.0, pad="middle"),   # 3
    "f384": dict(B=2, Q=100, S=384, L=1, p=0.0, pad="middle"),   # 3
    "f385": dict(B=2, Q=100, S=385, L=1, p=0.0, pad="middle"),   # 4
    "g": dict(B=2, Q=128, S=512, L=2, p=0.1, pad="tail"),        # both limits; 4 splits; the 128-row slabs of `part` full
    "h": dict(B=10, Q=100, S=224, L=2, p=0.1, pad="tail"),       # second image of an XCD (b = xcc + 8), padded differently from the first
    "i": dict(B=17, Q=7, S=40, L=1, p=0.0, pad="tail"),          # three images on XCD 0; control words reused
    "j": dict(B=2, Q=100, S=224, L=8, p=0.1, pad="tail", last_only=True),      # TOIST_XDEC_MAX_LAYERS; g_out of layers 0 .. L-2 zero (aux_loss = False)
    "k": dict(B=8, Q=100, S=416, L=6, p=0.1, pad="none", x0_zero=True),        # the benchmark's shape, x0 = 0 as in the model
    "l": dict(B=2, Q=30, S=40, L=2, p=0.0, pad="tail"),          # p = 0 with two layers: the stage-level check of the layer-to-layer gradient hand-off
}


def make_key_pad(B, S, pad):
    if pad == "none":
        return None
    kp = torch.zeros(B, S, dtype=torch.uint8)
    for b in range(B):
        if pad in ("tail", "tail+mid"):
            n = 1 + (b * 41) % max(1, S // 3)          # 41: coprime to S // 3 of every case, so images b and b + 8 differ
            kp[b, S - n:] = 1
            if pad == "tail+mid":
                kp[b, (b * 11 + 3) % max(1, S - n)] = 1
        else:
            lo = S // 3 + b
            kp[b, lo:lo + S // 5] = 1
    if pad == "tail+mid":
        kp[B - 1] = 1
        kp[B - 1, S // 2] = 0
    return kp


def make_case(name):
    """Synthetic inputs of case `name` as the launches take them (CPU tensors): bf16 weights scaled 1 / sqrt(fan_in), gammas in [0.5, 1.5], non-zero
    biases and betas, kv a column slice of a wider tensor (ldkv = L*512 + 64)."""
    c = dict(CASES[name])
    B, Q, S, L = c["B"], c["Q"], c["S"], c["L"]
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    bf = torch.bfloat16
    M = B * Q
    rn = lambda *s: torch.randn(*s, generator=g)
    c["x0"] = torch.zeros(M, D, dtype=bf) if c.get("x0_zero") else rn(M, D).to(bf)
    c["qpos"] = rn(Q, D).to(bf).unsqueeze(0).expand(B, Q, D).reshape(M, D).contiguous()
    c["kv_wide"] = rn(B * S, L * 2 * D + 64).to(bf)
    c["kv"] = c["kv_wide"][:, 32:32 + L * 2 * D]            # what the launches are given: row stride L*512 + 64, 64 bytes into the row
    c["key_pad"] = make_key_pad(B, S, c["pad"])
    layers = []
    for _ in range(L):
        P = {}
        for w, (n_out, n_in) in (("w_in", (3 * D, D)), ("w_os", (D, D)), ("w_q", (D, D)), ("w_oc", (D, D)), ("w1", (FF, D)), ("w2", (D, FF))):
            P[w] = (rn(n_out, n_in) / math.sqrt(n_in)).to(bf)
        for b_, n in (("b_in", 3 * D), ("b_os", D), ("b_q", D), ("b_oc", D), ("b1", FF), ("b2", D), ("be1", D), ("be3", D), ("be4", D)):
            P[b_] = rn(n) * 0.1
        for g_ in ("g1", "g3", "g4"):
            P[g_] = torch.rand(D, generator=g) + 0.5
        P["seed"] = [int(torch.randint(1, 2 ** 62, (1,), generator=g)) for _ in range(6)] if c["p"] > 0 else [0] * 6
        layers.append(P)
    c["layers"] = layers
    g_out = rn(L, M, D).to(bf)
    if c.get("last_only"):
        g_out[:L - 1] = 0
    c["g_out"] = g_out
    return c


GRADS = ("gb4", "dh", "go3", "go1", "dq_s", "dk_s", "dv_s", "dq_c", "dk_c", "dv_c", "dg1", "dbe1", "dg3", "dbe3", "dg4", "dbe4")


def run_reference(c, round_stores=False):
    """forward + autograd of case `c` (make_case).  Returns (out, grads): out[name] [L, ...] detached, grads[name] = list over the layers of the
    gradients the backward launch exports (GRADS; the LayerNorm parameter gradients are ln_part summed over the row blocks) + "gx_proj" / "gx_res":
    the gradient of x0 through layer 0's in_proj and through the residual connection."""
    B, Q, S, L, p = c["B"], c["Q"], c["S"], c["L"], c["p"]
    x0 = c["x0"].double().requires_grad_(True)
    kv = c["kv"].double().requires_grad_(True)
    layers = [{n: (v if n == "seed" else v.double().requires_grad_(n in ("g1", "be1", "g3", "be3", "g4", "be4"))) for n, v in P.items()} for P in c["layers"]]
    out, taps = forward(x0, c["qpos"].double(), kv, c["key_pad"], layers, p, B, Q, S, round_stores=round_stores)
    for n in ("t4", "a1", "t3", "t1", "qkv", "qc"):
        for t in taps[n]:
            t.retain_grad()
    taps["x_proj"].retain_grad()
    taps["x_res"].retain_grad()
    (out["y4"] * c["g_out"].double()).sum().backward()
    gr = {n: [] for n in GRADS}
    for l in range(L):
        gr["gb4"].append(taps["t4"][l].grad)
        gr["dh"].append(taps["a1"][l].grad)
        gr["go3"].append(taps["t3"][l].grad)
        gr["go1"].append(taps["t1"][l].grad)
        gq = taps["qkv"][l].grad
        gr["dq_s"].append(gq[:, :D])
        gr["dk_s"].append(gq[:, D:2 * D])
        gr["dv_s"].append(gq[:, 2 * D:])
        gr["dq_c"].append(taps["qc"][l].grad)
        gr["dk_c"].append(kv.grad[:, l * 2 * D:l * 2 * D + D])
        gr["dv_c"].append(kv.grad[:, l * 2 * D + D:(l + 1) * 2 * D])
        for n in ("g1", "be1", "g3", "be3", "g4", "be4"):
            gr["d" + n].append(layers[l][n].grad)
    gr["gx_proj"], gr["gx_res"] = [taps["x_proj"].grad], [taps["x_res"].grad]
    return {n: v.detach() for n, v in out.items()}, gr


def e_model(ref, model, floor=0.0):
    """per tensor and layer: relF(forward(round_stores=True), forward()) -- ref / model = (out, grads) of run_reference"""
    e = {"y4": [relF(model[0]["y4"][l], ref[0]["y4"][l], floor) for l in range(ref[0]["y4"].shape[0])]}
    for n, v in ref[1].items():
        e[n] = [relF(a, b, floor) for a, b in zip(model[1][n], v)]
    return e
