"""fp64 references with a derived per-element error bound for the attention cores -- attn2_fwd_kernel (csrc/attn2.hip), the key-owning backward
(csrc/attn2_bwd_body.h, also a phase of the decoder's backward launch) and the whole-head text kernels (csrc/attn_small.hip) -- in the manner of
tests/rounding_bounds.py and tests/row_bounds.py, whose U, UB, round_bf16, acc_term, ratio, record and check they use.  Shared by
tests/test_cpu_attn_bounds.py (f32 torch emulations with the kernels' block structure inside every bound, named mutants outside it) and
tests/test_gpu_attn_cores.py.  Not a conftest and not a test.

A kernel is right when |got - ref| <= bound for EVERY element; no share of the elements is excused.  The terms (u = 2^-24, ub = 2^-8), none tuned:

  scores        an f32 dot of dh products of two bf16 values (exact in f32; MFMA in attn2, FMA loops in attn_small):
                |s - s*| <= e_s = (dh + 2) u sum|q||k|.
  argument      the kernels form exp2((s - m) c), c = scale * log2(e) (attn_small: __expf((s - m)), scale folded into s).  The row maximum m carries
                e_m = max_j e_s; the f32 subtraction, the product with c and c itself (two f32 constants and their product) cost a few u |x| on the
                argument x; the argument's error delta_x carries through exp2 as a RELATIVE ln 2 * delta_x on the probability.
  exponential   hardware exp2 / __expf: the relative allowance the project already uses for __expf, E_EXP = 2^-14 (rounding_bounds.attnmap_fwd_ref) --
                borrowed, not fitted; 64 times below the bf16 storage term, so it cannot hide a wrong element of a bf16 output.  A result below
                2^-126 may be flushed: an ABSOLUTE 2^-126 per probability (FLUSH, doubled for a subnormal bf16 rounding).
  bf16 operand  where a kernel rounds a score-shaped value to bf16 before an MFMA (attn2: the dropped-out probabilities before P V; dS and Pd in the
                backward) the reference does NOT imitate the rounding -- so there are no tie cases -- and charges ub * sum_j |t_j| |w_j| instead, from the
                same fp64 operator run on absolute values.
  accumulation  acc_term(n, sum|t_i|) = (n + 2) u sum|t_i| for a sum of n terms in any order (ACC_WIDEN in force under the four keys of WIDEN_KEYS).
  storage       ub |ref| for a bf16 output; none for the f32 row statistics.

Fully masked rows are outside the kernels' contract (the reference's own result there is NaN) and get no case.  Measured figures go to
attn_core_parity.json beside rounding_bounds.RECORD (committed as profiles/attn_core_parity.json)."""
import math

import torch

import rounding_bounds as rb
from oracle.train_ref import small_attn_keep
from oracle.xdec_ref import pair_hash
from rounding_bounds import BF, F32, F64, U, UB, acc_term, round_bf16

FILE = "attn_core_parity.json"
WIDEN_KEYS = ["attn2_fwd", "attn2_bwd", "attn_small_fwd", "attn_small_bwd"]      # the names the references below widen under
E_EXP = 2.0 ** -14                # relative error allowed to exp2 / __expf: the constant of rounding_bounds.attnmap_fwd_ref
FLUSH = 2.0 ** -125               # 2 * 2^-126: a flushed exponential, and the rounding of a subnormal bf16
LN2 = math.log(2.0)
LOG2E = float(torch.tensor(1.4426950408889634, dtype=F32))


def widen_of(kernel):
    """the ACC_WIDEN factor in force for a RECORDED kernel name ('attn2_bwd.dq_part': the reference's key is its prefix; the longest key first)"""
    for key in sorted(WIDEN_KEYS, key=len, reverse=True):
        if kernel.startswith(key):
            return rb.ACC_WIDEN.get(key, 1.0)
    return 1.0


def check(kernel, case, got, ref, bound):
    rb.check(kernel, case, got, ref, bound, file=FILE, widen=widen_of(kernel))


def record(kernel, case, value, extra=None):
    return rb.record(kernel, case, value, widen=widen_of(kernel), file=FILE, extra=extra)


def check_parts(kernel, case, gots, refs, bounds):
    """several tensors under ONE record (the shares of dq_part): each is held separately, the largest ratio is recorded before any is asserted"""
    rs = [rb.ratio(g, r, b) for g, r, b in zip(gots, refs, bounds)]
    record(kernel, case, max(rs), extra={"parts": len(rs)})
    for i, r in enumerate(rs):
        assert r <= 1.0, f"{kernel} [{case}] part {i} of {len(rs)}: max err/bound {r}"


def f32v(x):
    """a Python float as the f32 the C interface receives"""
    return float(torch.tensor(x, dtype=F32))


def drop_scale(p):
    """1 / (1 - p) of the f32 p, in fp64 (the kernels' f32 subtraction and division are charged in the bounds)"""
    return 1.0 / (1.0 - f32v(p)) if p > 0 else 1.0


def round8(n):
    return (n + 7) // 8 * 8


def heads(t, B, S, H, dh):
    """rows [B * S, H * dh] -> [B, H, S, dh]"""
    return t.reshape(B, S, H, dh).permute(0, 2, 1, 3)


def rows(t):
    """[B, H, S, dh] -> rows [B * S, H * dh]"""
    B, H, S, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * dh)


def to_bf16(v):
    """fp64 -> bf16 with ONE rounding"""
    return round_bf16(v).to(BF)


# ---------------------------------------------------------------------------------------------------------------- attn2: cases and inputs
A2_B, A2_H, A2_DH = 2, 3, 32                  # d = 96: bh / H with an H that is no power of two
A2_D = A2_H * A2_DH
# Sq on 16 / 32 / 64 and n_tiles = 1, 2, 3, 4, 6 (n_iter odd and even); Sk on 32 / 128 / 512, odd and no multiple of 8; 1, 2, 5, 6 key splits with
# nw = 1 and nw = 4 active waves in the last
A2_SHAPES = [(1, 1), (17, 17), (64, 33), (65, 127), (33, 128), (97, 129), (32, 161), (1, 512), (64, 513), (65, 641), (161, 97)]
A2_DROPS = [0.0, 0.1, 0.5]
A2_PADS = ["none", "first", "last", "block2_first", "tail", "first_block", "first_stage", "all_but_last_block", "per_image"]


def a2_pads(Sk):
    """the patterns that leave a live key in every image at this key count"""
    out = ["none"]
    if Sk > 1:
        out += ["first", "last", "tail"]
    if Sk > 2:
        out += ["per_image"]
    if Sk > 128:
        out += ["block2_first", "first_block", "all_but_last_block"]
    if Sk > 512:
        out += ["first_stage"]
    return [p for p in A2_PADS if p in out]


def a2_key_pad(Sk, pad):
    """[B, Sk] u8 (1 = padded) or None; never a whole image"""
    if pad == "none":
        return None
    kp = torch.zeros(A2_B, Sk, dtype=torch.uint8)
    last_block = (Sk - 1) // 128 * 128
    if pad == "first":
        kp[:, 0] = 1
    elif pad == "last":
        kp[:, Sk - 1] = 1
    elif pad == "block2_first":
        kp[:, 128] = 1
    elif pad == "tail":
        kp[:, Sk - max(1, Sk // 3):] = 1
    elif pad == "first_block":
        kp[:, :128] = 1
    elif pad == "first_stage":
        kp[:, :512] = 1
    elif pad == "all_but_last_block":
        kp[:, :last_block] = 1
    elif pad == "per_image":
        kp[0, 0] = 1
        kp[0, Sk - max(1, Sk // 4):] = 1
        kp[1, Sk // 3:Sk // 3 + max(1, Sk // 2)] = 1
    else:
        raise ValueError(pad)
    assert pad in a2_pads(Sk) and int(kp.sum(1).max()) < Sk, (Sk, pad)
    return kp


def a2_cases():
    """(Sq, Sk, p, pad): every shape with every padding pattern it admits; the dropout value rotates, so that every shape and every pattern meets all of
    0, 0.1 and 0.5 (Sk = 1 admits one pattern, and only two shapes admit a masked first stage: those take the three values each)"""
    for i, (Sq, Sk) in enumerate(A2_SHAPES):
        pads = a2_pads(Sk)
        for j, pad in enumerate(pads):
            for p in (A2_DROPS if len(pads) < 3 or pad == "first_stage" else [A2_DROPS[(i + j) % 3]]):
                yield Sq, Sk, p, pad


def a2_name(Sq, Sk, p, pad):
    return f"{Sq}x{Sk} p={p:g} pad={pad}"


def a2_inputs(Sq, Sk, p, pad):
    """q, k (randn * 1.5: scaled scores of spread 2.25, a peaked softmax -- one key carries a row, so one wrong key shows), v, dctx as rows
    [B * S, 96] bf16; a seed with bits above 2^32"""
    g = torch.Generator().manual_seed(7919 * Sq + 13 * Sk + A2_PADS.index(pad))
    B, d = A2_B, A2_D
    return dict(q=(torch.randn(B * Sq, d, generator=g) * 1.5).to(BF), k=(torch.randn(B * Sk, d, generator=g) * 1.5).to(BF),
                v=torch.randn(B * Sk, d, generator=g).to(BF), dctx=torch.randn(B * Sq, d, generator=g).to(BF), key_pad=a2_key_pad(Sk, pad),
                Sq=Sq, Sk=Sk, p=p, pad=pad, scale=1.0 / math.sqrt(A2_DH), seed=0x5EED0BADC0DE + 1000 * Sq + Sk, B=B, H=A2_H, dh=A2_DH)


def a2_keep(BH, Sq, Sk, p, seed, ld=None):
    """keep mask [BH, Sq, Sk] of csrc/attn2.hip from oracle.xdec_ref.pair_hash (csrc/common.h pair_hash): element row * round8(Sk) + key, one hash per element pair, the 16-bit
    field of the element's parity >= round(p * 2^16).  ld: another row pitch (a mutant of the emulation)"""
    if p <= 0:
        return torch.ones(BH, Sq, Sk, dtype=torch.bool)
    ld = round8(Sk) if ld is None else ld
    idx = torch.arange(BH * Sq, dtype=torch.int64).view(BH, Sq, 1) * ld + torch.arange(Sk, dtype=torch.int64).view(1, 1, Sk)
    h = pair_hash(idx >> 1, seed)
    return torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF) >= int(p * 65536.0 + 0.5)


def _a2_common(t):
    B, H, dh, Sq, Sk = t["B"], t["H"], t["dh"], t["Sq"], t["Sk"]
    q, k, v = (heads(t[n].to(F64), B, S, H, dh) for n, S in (("q", Sq), ("k", Sk), ("v", Sk)))
    dead = torch.zeros(B, 1, 1, Sk, dtype=torch.bool) if t["key_pad"] is None else t["key_pad"].bool().view(B, 1, 1, Sk)
    keep = a2_keep(B * H, Sq, Sk, t["p"], t["seed"]).view(B, H, Sq, Sk)
    s = q @ k.transpose(-1, -2)
    e_s = (dh + 2) * U * (q.abs() @ k.abs().transpose(-1, -2))
    return B, H, dh, Sq, Sk, q, k, v, dead.expand(B, H, Sq, Sk), keep, s, e_s


def a2_fwd_ref(t):
    """attn2_fwd_kernel: dict name -> (ref, bound) for ctx [B * Sq, 96] (bf16), lse_max and lse_rsum [B * H, Sq] (f32), and `host`: the (ctx bf16,
    lse f32 [B * H, Sq, 2]) a correct forward hands to the backward, built here -- m the fp64 maximum rounded to f32, rs the f32 reciprocal of the fp64
    sum, ctx the bf16 rounding of the fp64 context.
      m      = max over live keys of the raw dots               |m^ - m| <= e_m = max_j e_s                      (lse_max: held to exactly this)
      x_j    = (s_j - m) c, c = scale log2(e)                   delta_x = c (e_s + e_m) + 8 u |x|: the kernel reaches exp2(x_j) as exp2 of (s_j - m_blk) c
               times one alpha = exp2((m_old - m_new) c) per later 128-key block; the arguments of that chain add up to x_j and their magnitudes to
               |x_j|, each with a subtraction, c (three roundings) and a product: 5 u, and 3 to spare
      pe_j   = exp2(x_j)                                        relative e_rel = ln 2 delta_x + (1 + nb) E_EXP + nb u    (nb blocks: one exp2 and one
               product per rescale); absolute FLUSH
      l      = sum_j pe_j over live keys, BEFORE dropout        relative d_l = sum pe e_rel / l + (Sk + 2) u + Sk FLUSH / l     (positive terms)
      rs     = 1 / l                                            relative e_rs = d_l / (1 - d_l) + 3 u                          (lse_rsum: held to this)
      ctx    = sum_j Pd_j v_j, Pd = keep pe rs / (1 - p)        ub A (each Pd_j is rounded to bf16 before P V; A = sum_j |Pd_j v_j|)
                                                                + sum_j Pd_j e_rel_j |v_j| + e_rs A + acc_term(Sk, A) + 6 u A (1 - p, the division,
                                                                the product with the accumulator) + FLUSH rs / (1 - p) sum_j |v_j|; storage ub |ctx|
    A dropped or padded key contributes exactly nothing to ref and to every term of the bound."""
    B, H, dh, Sq, Sk, q, k, v, dead, keep, s, e_s = _a2_common(t)
    c = f32v(t["scale"]) * LOG2E
    m = s.masked_fill(dead, float("-inf")).amax(-1, keepdim=True)
    e_m = e_s.masked_fill(dead, 0.0).amax(-1, keepdim=True)
    x = torch.where(dead, torch.zeros_like(s), (s - m) * c)
    pe = torch.where(dead, torch.zeros_like(s), torch.exp2(x))
    nb = (Sk + 127) // 128
    e_rel = LN2 * (c * (e_s + e_m) + 8 * U * x.abs()) + (1 + nb) * E_EXP + nb * U
    l = pe.sum(-1, keepdim=True)
    d_l = (pe * e_rel).sum(-1, keepdim=True) / l + acc_term(Sk, 1.0, "attn2_fwd") + Sk * FLUSH / l
    rs = 1.0 / l
    e_rs = d_l / (1 - d_l) + 3 * U
    sc = drop_scale(t["p"])
    Pd = pe * rs * keep.to(F64) * sc
    va = v.abs()
    ref, A = Pd @ v, Pd @ va
    ev = UB * A + (Pd * e_rel) @ va + e_rs * A + acc_term(Sk, A, "attn2_fwd") + 6 * U * A + FLUSH * rs * sc * va.sum(-2, keepdim=True)
    lse = torch.stack([m[..., 0].to(F32), rs[..., 0].to(F32)], -1).reshape(B * H, Sq, 2)
    return dict(ctx=(rows(ref), rows(UB * ref.abs() + ev * (1 + UB))), lse_max=(m.reshape(B * H, Sq), e_m.reshape(B * H, Sq)),
                lse_rsum=(rs.reshape(B * H, Sq), (rs * e_rs).reshape(B * H, Sq)), host=(to_bf16(rows(ref)), lse))


def a2_splits(Sk):
    return ((Sk + 31) // 32 + 3) // 4


def a2_bwd_ref(t, ctx, lse):
    """the key-owning backward as a function of ITS inputs (q, k, v, ctx, dctx, lse): what the kernel evaluates from the given m = lse[..., 0] and
    rs = lse[..., 1], taken as exact.  dict name -> (ref, bound) for dk, dv [B * Sk, 96] and dq: a LIST with one (ref, bound) [B * Sq, 96] per 128-key
    split, each the fp64 sum over that split's keys alone (one split: dq itself).
      P    = exp2((s - m) c) rs             relative e_P = ln 2 (c e_s + 6 u |x|) + E_EXP + 2 u; absolute FLUSH rs; exactly 0 at a padded key
      D    = sum_e dO O                     e_D = acc_term(dh, sum|dO O|)
      dP   = dO . v                         e_dP = (dh + 2) u sum|dO||v|
      dp   = keep dP / (1 - p)              e_dp = keep (e_dP / (1 - p) + 5 u |dp|)               (1 - p, the division, the product)
      Pd   = keep P / (1 - p)               e_Pd = |Pd| (e_P + 5 u) + keep FLUSH rs / (1 - p)
      dS   = P (dp - D)                     e_dS = (P e_P + FLUSH rs) T + P (e_dp + e_D + u T) + u |dS|,  T = |dp| + |D|
      dv_j = sum_i Pd_ij dO_i               ub Av (Pd is rounded to bf16 before the MFMA; Av = sum_i |Pd||dO|) + sum_i e_Pd |dO| + acc_term(Sq, Av)
      dk_j = scale sum_i dS_ij q_i          ub Ak + scale sum_i e_dS |q| + acc_term(Sq, Ak) + 2 u Ak,  Ak = scale sum_i |dS||q|
      dq_i = scale sum_{j in split} dS_ij k_j   the same with the split's keys: acc_term(128, Aq)
    and the storage term ub |ref| on each.  Every term carries the live-key mask: rows of dk and dv at padded keys have ref = 0 and bound = 0 --
    exactly nothing -- and so has a whole dq share whose 128 keys are padded."""
    B, H, dh, Sq, Sk, q, k, v, dead, keep, s, e_s = _a2_common(t)
    dO, O = heads(t["dctx"].to(F64), B, Sq, H, dh), heads(ctx.to(F64), B, Sq, H, dh)
    scale = f32v(t["scale"])
    c = scale * LOG2E
    ls = lse.to(F64).view(B, H, Sq, 2)
    m, rs = ls[..., :1], ls[..., 1:]
    live = (~dead).to(F64)
    x = torch.where(dead, torch.zeros_like(s), (s - m) * c)
    P = torch.exp2(x) * rs * live
    e_P = LN2 * (c * e_s + 6 * U * x.abs()) + E_EXP + 2 * U
    fl = FLUSH * rs * live
    D = (dO * O).sum(-1, keepdim=True)
    e_D = acc_term(dh, (dO * O).abs().sum(-1, keepdim=True), "attn2_bwd")
    dP = dO @ v.transpose(-1, -2)
    e_dP = (dh + 2) * U * (dO.abs() @ v.abs().transpose(-1, -2))
    sc = drop_scale(t["p"])
    kf = keep.to(F64) * live
    dp = kf * dP * sc
    e_dp = kf * e_dP * sc + 5 * U * dp.abs()
    Pd = P * kf * sc
    e_Pd = Pd * (e_P + 5 * U) + fl * kf * sc
    T = dp.abs() + D.abs()
    dS = P * (dp - D)
    e_dS = (P * e_P + fl) * T + P * (e_dp + e_D + U * T) + U * dS.abs()

    def out(ref, A, e, n):
        ev = UB * A + e + acc_term(n, A, "attn2_bwd")
        return rows(ref), rows(UB * ref.abs() + ev * (1 + UB))
    tr = lambda a: a.transpose(-1, -2)
    dv = out(tr(Pd) @ dO, tr(Pd) @ dO.abs(), tr(e_Pd) @ dO.abs(), Sq)
    Ak = scale * (tr(dS.abs()) @ q.abs())
    dk = out(scale * (tr(dS) @ q), Ak, scale * (tr(e_dS) @ q.abs()) + 2 * U * Ak, Sq)
    dq = []
    for sp in range(a2_splits(Sk)):
        sl = slice(128 * sp, min(Sk, 128 * sp + 128))
        Aq = scale * (dS[..., sl].abs() @ k[..., sl, :].abs())
        dq.append(out(scale * (dS[..., sl] @ k[..., sl, :]), Aq, scale * (e_dS[..., sl] @ k[..., sl, :].abs()) + 2 * U * Aq, 128))
    return dict(dk=dk, dv=dv, dq=dq)


# ---------------------------------------------------------------------------------------------------------------- attn_small: cases and inputs
AS_B, AS_H = 3, 3
AS_S = [1, 7, 16, 17, 32, 33, 64]             # the 16 / 32 / 64-lane row groups and their edges
AS_DH = [8, 16, 40, 64]
AS_DROPS = [0.0, 0.1, 0.5]
AS_PADS = ["none", "first", "last", "middle"]
AS_SEED_WORD = (0xFFFFFFF0, 0x25)             # host seed + device word: the sum carries past 2^32


def as_cases():
    """(S, dh, p, bias, pad): every S with every dh; p, the biases and the padding pattern rotate with the case index, so that every S meets all three
    dropout values, both bias settings and -- from S = 7 on -- all four patterns (one key cannot be padded)"""
    for i, S in enumerate(AS_S):
        for j, dh in enumerate(AS_DH):
            n = i + j
            yield S, dh, AS_DROPS[n % 3], (i + j // 2) % 2 == 0, AS_PADS[(2 * i + j) % 4] if S > 1 else "none"


def as_name(S, dh, p, bias, pad):
    return f"S={S} dh={dh} p={p:g} bias={'yes' if bias else 'no'} pad={pad}"


def as_inputs(S, dh, p, bias, pad):
    """q, k, v, dctx rows [B * S, H * dh] bf16; the three projection biases f32 [H * dh] or None; key_pad [B, S] u8 or None"""
    g = torch.Generator().manual_seed(131 * S + dh + 7 * AS_PADS.index(pad) + (3 if bias else 0))
    B, d = AS_B, AS_H * dh
    rn = lambda n, sd: (torch.randn(n, d, generator=g) * sd).to(BF)
    t = dict(q=rn(B * S, 1.5 * (32.0 / dh) ** 0.25), k=rn(B * S, 1.5 * (32.0 / dh) ** 0.25), v=rn(B * S, 1.0), dctx=rn(B * S, 1.0),
             bq=None, bk=None, bv=None, key_pad=None, S=S, dh=dh, p=p, pad=pad, scale=1.0 / math.sqrt(dh), seed=0xABCDEF0123 + 17 * S + dh, B=B, H=AS_H)
    if bias:
        t["bq"], t["bk"], t["bv"] = (0.5 * torch.randn(d, generator=g) for _ in range(3))
    if pad != "none":
        assert S > 1
        kp = torch.zeros(B, S, dtype=torch.uint8)
        if pad == "first":
            kp[:, 0] = 1
        elif pad == "last":
            kp[:, S - 1] = 1
        else:
            for b in range(B):
                kp[b, (S // 2 + b) % S] = 1
        t["key_pad"] = kp
    return t


def _as_common(t, keep):
    """the biased operands (one f32 add each: relative u, charged as 2 u of sum|q'||k'| in e_s), the scaled scores and P from GIVEN statistics or its own"""
    B, H, dh, S = t["B"], t["H"], t["dh"], t["S"]
    bias = lambda n: 0.0 if t[n] is None else t[n].to(F64).view(1, H, 1, dh)
    q, k, v = (heads(t[n].to(F64), B, S, H, dh) + bias(b) for n, b in (("q", "bq"), ("k", "bk"), ("v", "bv")))
    dead = (torch.zeros(B, 1, 1, S, dtype=torch.bool) if t["key_pad"] is None else t["key_pad"].bool().view(B, 1, 1, S)).expand(B, H, S, S)
    scale = f32v(t["scale"])
    s = (q @ k.transpose(-1, -2)) * scale
    e_s = (dh + 8) * U * scale * (q.abs() @ k.abs().transpose(-1, -2))
    if keep is None:
        keep = small_attn_keep(B, H, S, t["p"], t["seed"]) if t["p"] > 0 else torch.ones(B, H, S, S, dtype=torch.bool)
    return B, H, dh, S, q, k, v, dead, keep.view(B, H, S, S), s, e_s


def as_fwd_ref(t, keep=None):
    """attn_small_fwd_kernel, all f32: dict name -> (ref, bound) for ctx [B * S, H dh] (bf16), stat_max and stat_rsum [B * H, S] (f32), and `host`: the
    statistics f32 [B * H, S, 2] a correct forward hands to the backward (m the fp64 maximum rounded to f32, rs the f32 reciprocal of the fp64 sum).
      q' = q + bq (k, v alike)           one f32 add; with it, both roundings of a product that may or may not be fused and the scale (an f32 constant
                                         and its product): e_s = (dh + 8) u scale sum|q'||k'| for the SCALED score s = scale q'.k'
      m  = max_j s_j                     e_m = max_j e_s                                                      (stat_max)
      pe = __expf(s - m)                 relative e_rel = e_s + e_m + 3 u |s - m| + E_EXP (natural units: no ln 2); absolute FLUSH
      rs = 1 / sum_j pe_j                relative e_rs = d / (1 - d) + 3 u, d = sum pe e_rel / sum + (S + 2) u + S FLUSH / sum       (stat_rsum)
      Pd = keep pe rs / (1 - p)          relative e_rel + e_rs + 6 u  (two products; 1 - p and its division)
      ctx = sum_j Pd_j v'_j              f32 FMA loop over unrounded Pd: sum_j Pd (e_rel + e_rs + 8 u) |v'| (v' and the product: 2 u) + acc_term(S, A)
                                         + FLUSH rs / (1 - p) sum|v'|; storage ub |ctx|
    keep: the mask [B, H, S, S] to use instead of small_attn_keep(seed) (the device seed word case passes the mask of seed + word)."""
    B, H, dh, S, q, k, v, dead, keep, s, e_s = _as_common(t, keep)
    m = s.masked_fill(dead, float("-inf")).amax(-1, keepdim=True)
    e_m = e_s.masked_fill(dead, 0.0).amax(-1, keepdim=True)
    x = torch.where(dead, torch.zeros_like(s), s - m)
    pe = torch.where(dead, torch.zeros_like(s), torch.exp(x))
    e_rel = e_s + e_m + 3 * U * x.abs() + E_EXP
    l = pe.sum(-1, keepdim=True)
    d_l = (pe * e_rel).sum(-1, keepdim=True) / l + acc_term(S, 1.0, "attn_small_fwd") + S * FLUSH / l
    rs = 1.0 / l
    e_rs = d_l / (1 - d_l) + 3 * U
    sc = drop_scale(t["p"])
    Pd = pe * rs * keep.to(F64) * sc
    va = v.abs()
    ref, A = Pd @ v, Pd @ va
    ev = (Pd * (e_rel + e_rs + 8 * U)) @ va + acc_term(S, A, "attn_small_fwd") + FLUSH * rs * sc * va.sum(-2, keepdim=True)
    stats = torch.stack([m[..., 0].to(F32), rs[..., 0].to(F32)], -1).reshape(B * H, S, 2)
    return dict(ctx=(rows(ref), rows(UB * ref.abs() + ev * (1 + UB))), stat_max=(m.reshape(B * H, S), e_m.reshape(B * H, S)),
                stat_rsum=(rs.reshape(B * H, S), (rs * e_rs).reshape(B * H, S)), host=stats)


def as_bwd_ref(t, stats, keep=None):
    """attn_small_bwd_kernel as a function of its inputs (q, k, v, the biases, stats, dctx), all f32 with FMA loops; m, rs = the GIVEN statistics.
      P    = __expf(s - m) rs             relative e_P = e_s + 3 u |s - m| + E_EXP + u; absolute FLUSH rs; exactly 0 at a padded key
      Pd   = keep P / (1 - p)             e_Pd = Pd (e_P + 5 u) + keep FLUSH rs / (1 - p)
      dv_j = sum_i Pd_ij dO_i             sum_i e_Pd |dO| + acc_term(S, sum_i |Pd||dO|)
      dp   = keep (dO . v') / (1 - p)     e_dp = keep (dh + 8) u sum|dO||v'| / (1 - p) + 5 u |dp|
      r_i  = sum_j P_ij dp_ij             e_r = acc_term(S, sum_j |P dp|) + sum_j (P e_dp + (P e_P + FLUSH rs) |dp|)
      dS   = P (dp - r) scale             e_dS = scale [(P e_P + FLUSH rs) T + P (e_dp + e_r + u T)] + 3 u |dS|,  T = |dp| + |r|
      dq_i = sum_j dS_ij k'_j             sum_j (e_dS + 3 u |dS|) |k'| (k' and the product) + acc_term(S, sum_j |dS||k'|);   dk_j = sum_i dS_ij q'_i alike
    and the storage term ub |ref| on each.  Every term carries the live-key mask."""
    B, H, dh, S, q, k, v, dead, keep, s, e_s = _as_common(t, keep)
    dO = heads(t["dctx"].to(F64), B, S, H, dh)
    scale = f32v(t["scale"])
    st = stats.to(F64).view(B, H, S, 2)
    m, rs = st[..., :1], st[..., 1:]
    live = (~dead).to(F64)
    x = torch.where(dead, torch.zeros_like(s), s - m)
    P = torch.exp(x) * rs * live
    e_P = e_s + 3 * U * x.abs() + E_EXP + U
    fl = FLUSH * rs * live
    sc = drop_scale(t["p"])
    kf = keep.to(F64) * live
    Pd = P * kf * sc
    e_Pd = Pd * (e_P + 5 * U) + fl * kf * sc
    dp = kf * (dO @ v.transpose(-1, -2)) * sc
    e_dp = kf * (dh + 8) * U * (dO.abs() @ v.abs().transpose(-1, -2)) * sc + 5 * U * dp.abs()
    r = (P * dp).sum(-1, keepdim=True)
    e_r = acc_term(S, (P * dp).abs().sum(-1, keepdim=True), "attn_small_bwd") + (P * e_dp + (P * e_P + fl) * dp.abs()).sum(-1, keepdim=True)
    T = dp.abs() + r.abs()
    dS = P * (dp - r) * scale
    e_dS = scale * ((P * e_P + fl) * T + P * (e_dp + e_r + U * T)) + 3 * U * dS.abs()

    def out(ref, A, e):
        ev = e + acc_term(S, A, "attn_small_bwd")
        return rows(ref), rows(UB * ref.abs() + ev * (1 + UB))
    tr = lambda a: a.transpose(-1, -2)
    e3 = e_dS + 3 * U * dS.abs()
    return dict(dv=out(tr(Pd) @ dO, tr(Pd) @ dO.abs(), tr(e_Pd) @ dO.abs()),
                dq=out(dS @ k, dS.abs() @ k.abs(), e3 @ k.abs()), dk=out(tr(dS) @ q, tr(dS.abs()) @ q.abs(), tr(e3) @ q.abs()))
