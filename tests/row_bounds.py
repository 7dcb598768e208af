"""fp64 references with a derived per-element error bound for the row, elementwise and embedding kernels (csrc/rows.hip, csrc/elem.hip, the two
l2norm launches of csrc/contrastive.hip), in the manner of tests/rounding_bounds.py, whose U, UB, acc_term, ratio, record and check they use.
Shared by tests/test_cpu_row_bounds.py (f32 torch emulations that stay inside every bound, mutants that leave it) and the GPU tests
tests/test_gpu_row_kernels.py / tests/test_gpu_elem.py.  Not a conftest and not a test.

Every reference takes the bf16 / f32 tensors the kernel takes, on the CPU, and returns fp64 (ref, bound); a kernel is right when
|got - ref| <= bound for EVERY element -- no element is excluded, there is no flippable set.  Conventions (u = 2^-24), those of gn_coeffs:
an f32 add, subtract or multiply is within u, a division within 3u, rsqrtf / sqrtf within 2u; rows.hip and elem.hip are built with FMA
contraction allowed and without fast-math, so where a product feeds a sum the bound charges BOTH roundings (the unfused form; the fused one
has one of them).  A sum of n terms in ANY order is within acc_term(n, sum|t_i|) = (n + 2) u sum|t_i| of the exact sum; the two spare units
are spent, where noted, on the rounding of the terms themselves.  Measured figures go to row_kernel_parity.json beside rounding_bounds.RECORD
(committed as profiles/row_kernel_parity.json)."""
import math

import torch

import rounding_bounds as rb
from rounding_bounds import BF, F32, F64, U, UB, acc_term

FILE = "row_kernel_parity.json"


WIDEN_KEYS = ["layernorm_fwd", "layernorm_bwd", "softmax_fwd", "softmax_bwd", "colsum", "embed_type_bwd", "l2norm"]       # the names the references below widen under


def widen_of(kernel):
    """the ACC_WIDEN factor in force for a RECORDED kernel name ('layernorm_bwd.dgamma (atomic)', 'colsum (narrow)', 'l2norm_fwd': the reference's key is
    its prefix); the bit-for-bit kernels have none: 1"""
    for key in WIDEN_KEYS:
        if kernel.startswith(key):
            return rb.ACC_WIDEN.get(key, 1.0)
    return 1.0


def check(kernel, case, got, ref, bound):
    rb.check(kernel, case, got, ref, bound, file=FILE, widen=widen_of(kernel))


def record(kernel, case, value, extra=None):
    return rb.record(kernel, case, value, widen=widen_of(kernel), file=FILE, extra=extra)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def check_exact(kernel, case, got, want):
    """bit-for-bit (bound 0): records 0 or inf before it asserts; NaN in `got` (an unwritten element) never equals"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (kernel, case, got.dtype, want.dtype, got.shape, want.shape)
    bad = int((bits(got) != bits(want)).sum())
    record(kernel, case, 0.0 if bad == 0 else float("inf"))
    assert bad == 0, f"{kernel} [{case}]: {bad} of {got.numel()} elements differ"


def _inv_half(e):
    """relative error of v^-1/2 when v carries relative error e: (1 - e)^-1/2 <= 1 + e / (2 (1 - e))"""
    return torch.where(e < 1, 0.5 * e / (1 - e).clamp(min=1e-300), torch.full_like(e, float("inf")))


def f32_scale(p):
    """1.f / (1.f - p) as the kernels form it, as an f32 scalar tensor"""
    one = torch.tensor(1.0, dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm (rows.hip)
LN_D = [8, 256, 512, 520, 768, 1024]          # one live lane, one full chunk, the chunk boundary and one step past it, the product's, the limit
LN_ROWS = [1, 5, 17, 130]
LN_EPS = [1e-5, 1e-12]
LN_BIG = [(2051, 256), (4099, 256)]           # the atomic grid at its cap of 128 blocks, the deferred grid at its cap of 512


LN_DROP = (17, 1e-5, 0.1, 0x5EED1234)         # rows, eps, p, seed of the dx_drop case of every D (atomic path)


def ln_inputs(rows, D, offset=0.0):
    g = torch.Generator().manual_seed(11 * rows + D + (5 if offset else 0))
    return dict(x=(torch.randn(rows, D, generator=g) + offset).to(BF), dy=torch.randn(rows, D, generator=g).to(BF),
                add=torch.randn(rows, D, generator=g).to(BF), gamma=1.0 + 0.2 * torch.randn(D, generator=g), beta=0.3 * torch.randn(D, generator=g),
                dg0=torch.randn(D, generator=g), db0=torch.randn(D, generator=g))


def ln_fwd_ref(x, gamma, beta, eps):
    """layernorm_fwd_kernel against the fp64 LayerNorm of the bf16 input: dict name -> (ref, bound) for mean [rows], rstd [rows] (f32 outputs: no
    storage term) and y [rows, D] (bf16: storage + evaluation).  The kernel is two-pass, so nothing cancels:
      mean = (sum x) / D                  d_mean = acc_term(D, sum|x|) / D + 3u |mean|            (bf16 terms are exact in f32)
      dh   = x - mean (f32)               |dh - d| <= e = d_mean (1 + u) + u |d|                  with d = x - the TRUE mean
      var  = (sum dh^2) / D               d_var = [acc_term(D, sum (|d| + e)^2) + sum (2 |d| e + e^2)] / D + 3u var
                                          (the first term: D - 1 additions and the rounding of each square; the second: dh^2 - d^2 = 2 d e' + e'^2)
      rstd = rsqrtf(var + eps)            e_v = d_var / (var + eps) + 2u (the add, and eps as an f32), e_rs = e_v / (2 (1 - e_v)) + 2u
      y    = ((dh rstd) gamma) + beta     delta = |rstd gamma| e + |A| (e_rs + 2u) + u |y|,  A = d rstd gamma    (two products, one sum)
    A row of zero variance with a tiny eps has e_v >= 1 (bound inf): the constant row is checked apart, exactly."""
    xd, gm, bt = x.to(F64), gamma.to(F64), beta.to(F64)
    D = xd.shape[1]
    mean = xd.mean(1, keepdim=True)
    d = xd - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    d_mean = acc_term(D, xd.abs().sum(1, keepdim=True), "layernorm_fwd") / D + 3 * U * mean.abs()
    e = d_mean * (1 + U) + U * d.abs()
    d_var = (acc_term(D, ((d.abs() + e) ** 2).sum(1, keepdim=True), "layernorm_fwd") + (2 * d.abs() * e + e * e).sum(1, keepdim=True)) / D + 3 * U * var
    e_rs = _inv_half(d_var / (var + eps) + 2 * U) + 2 * U
    A = d * rstd * gm
    y = A + bt
    delta = (rstd * gm).abs() * e + A.abs() * (e_rs + 2 * U) + U * y.abs()
    return dict(mean=(mean[:, 0], d_mean[:, 0]), rstd=(rstd[:, 0], (e_rs * rstd)[:, 0]), y=(y, UB * y.abs() + delta * (1 + UB)))


def ln_y2_ref(y, add):
    """y2 = bf16(bf16(y) + add) from the DEVICE's own y, one f32 add and one rounding: bit for bit"""
    return (y.to(F32) + add.to(F32)).to(BF)


def ln_bwd_ref(dy, x, mean, rstd, gamma, dg0, db0, keep=None, p=0.0):
    """layernorm_bwd_kernel from the kernel's own mean / rstd (f32 [rows], taken as exact inputs).  With g = dy gamma, xh = (x - mean) rstd:
      xh                                  d_xh = 2u |xh|                                          (a subtraction and a product)
      m1 = (sum g) / D                    d_m1 = acc_term(D, sum|g|) / D + 3u |m1|                (the spare units: g's own rounding)
      m2 = (sum g xh) / D                 d_m2 = acc_term(D + 2, sum|g xh|) / D + 3u |m2|         (each term: u + 2u + the product's u)
      dx = rstd ((g - m1) - xh m2)        d_dx = rstd (d_m1 + |xh| d_m2 + 6u T) + u |dx|,  T = |g| + |m1| + |xh m2|
                                          (6u T: g, xh m2 with d_xh, its product, two subtractions, one to spare)       bf16: storage + d_dx
      dgamma = dg0 + sum_rows dy xh       acc_term(rows + 1, sum|dy xh| + |dg0|): rows additions in any order (wave walk, LDS fold, atomics or
                                          partial blocks + fold) and 3u for each term (d_xh, the product)
      dbeta  = db0 + sum_rows dy          acc_term(rows + 1, sum|dy| + |db0|)
      dx_drop (keep [rows, D] bool, p)    bf16(dx_f32 * sc), sc = 1.f / (1.f - p): storage + (d_dx sc + u |dx sc|); exactly 0 where dropped
    Returns dict name -> (ref, bound)."""
    xd, dyd, gm = x.to(F64), dy.to(F64), gamma.to(F64)
    rows, D = xd.shape
    mu, rs = mean.to(F64).view(rows, 1), rstd.to(F64).view(rows, 1)
    xh = (xd - mu) * rs
    g = dyd * gm
    m1 = g.sum(1, keepdim=True) / D
    d_m1 = acc_term(D, g.abs().sum(1, keepdim=True), "layernorm_bwd") / D + 3 * U * m1.abs()
    m2 = (g * xh).sum(1, keepdim=True) / D
    d_m2 = acc_term(D + 2, (g * xh).abs().sum(1, keepdim=True), "layernorm_bwd") / D + 3 * U * m2.abs()
    dx = rs * (g - m1 - xh * m2)
    T = g.abs() + m1.abs() + (xh * m2).abs()
    d_dx = rs * (d_m1 + xh.abs() * d_m2 + 6 * U * T) + U * dx.abs()
    out = dict(dx=(dx, UB * dx.abs() + d_dx * (1 + UB)),
               dgamma=(dg0.to(F64) + (dyd * xh).sum(0), acc_term(rows + 1, (dyd * xh).abs().sum(0) + dg0.to(F64).abs(), "layernorm_bwd")),
               dbeta=(db0.to(F64) + dyd.sum(0), acc_term(rows + 1, dyd.abs().sum(0) + db0.to(F64).abs(), "layernorm_bwd")))
    if keep is not None:
        sc = float(f32_scale(p))
        k = keep.to(F64)
        ref = dx * sc * k
        out["dx_drop"] = (ref, k * (UB * ref.abs() + (d_dx * sc + U * ref.abs()) * (1 + UB)))
    return out


# ---------------------------------------------------------------------------------------------------------------- masked softmax (rows.hip)
SM_SK = [1, 7, 8, 9, 63, 65, 511, 512, 513, 1066, 2048]       # around one 8-wide chunk, one wave pass, the register-chunk boundary (512), the evaluation shape, the limit
SM_PADS = ["none", "first", "last", "middle"]
SM_NB, SM_H, SM_SQ = 2, 3, 5                                  # 30 rows: not a multiple of the 4 rows of a block; b = row / (H * Sq) matters


def round8(n):
    return (n + 7) // 8 * 8


def sm_pads(Sk):
    """one key cannot be padded (the row would be padded away whole): Sk = 1 runs without key_pad only"""
    return SM_PADS if Sk > 1 else ["none"]


def sm_lds(Sk):
    return [ld for ld in (round8(Sk), round8(Sk) + 8) if ld <= 2048]


def sm_inputs(Sk, ld, pad):
    """scores [rows, ld] bf16, randn * 6 clamped to +-30 (|v - max| <= 64), columns [Sk, ld) = 1e4; key_pad [nbatch, Sk] u8 or None, never a whole row;
    dp [rows, ld] bf16 with NaN-free garbage past Sk"""
    g = torch.Generator().manual_seed(23 * Sk + ld + SM_PADS.index(pad))
    rows = SM_NB * SM_H * SM_SQ
    s = (torch.randn(rows, ld, generator=g) * 6).clamp(-30, 30)
    s[:, Sk:] = 1e4
    dp = torch.randn(rows, ld, generator=g)
    dp[:, Sk:] = 1e4
    kp = None
    assert pad in sm_pads(Sk)
    if pad != "none":
        kp = torch.zeros(SM_NB, Sk, dtype=torch.uint8)
        if pad == "first":
            kp[:, 0] = 1
        elif pad == "last":
            kp[:, Sk - 1] = 1
        else:
            kp[0, Sk // 3:Sk // 3 + max(1, Sk // 4)] = 1
            kp[1, Sk // 2:Sk // 2 + max(1, Sk // 5)] = 1
        assert int(kp.sum(1).max()) < Sk            # no row is padded away whole (its softmax would be NaN by construction)
    return dict(scores=s.to(BF), dp=dp.to(BF), key_pad=kp, Sk=Sk, ld=ld, rows=rows)


def sm_fwd_ref(t):
    """softmax_fwd_kernel: p [rows, ld] bf16; dead keys (key_pad of image row / (H Sq), or k >= Sk) and columns [Sk, ld) exactly 0 (bound 0).
    Live keys, for |v - max| <= 64 (v - max of two bf16 values within u):
      e = __expf(v - max) = exp2((v - max) log2e)   relative e_exp = (3 * 64 + 2) u: the subtraction, the f32 constant and the product each move
                                                    the argument by <= 64 u (absolute, in natural units), the hardware exponent is within 2u
      sum of Sk terms                               relative (Sk + 2) u   (all terms positive: sum|t| is the sum)
      p = e * (1 / sum)                             3u + u
    so relative e_p = 2 e_exp + (Sk + 2) u + 4u, and bound = 2^-8 p + e_p p (1 + 2^-8): at Sk = 2048 e_p is 2^-12.7, 20 times below the storage term."""
    Sk, ld, rows = t["Sk"], t["ld"], t["rows"]
    s = t["scores"].to(F64)[:, :Sk]
    if t["key_pad"] is not None:
        img = torch.arange(rows) // (SM_H * SM_SQ)
        s = s.masked_fill(t["key_pad"].bool()[img], float("-inf"))
    p = torch.softmax(s, -1)
    e_p = (2 * (3 * 64 + 2) + Sk + 2 + 4) * U * rb.ACC_WIDEN.get("softmax_fwd", 1.0)
    z = torch.zeros(rows, ld - Sk, dtype=F64)
    return torch.cat([p, z], 1), torch.cat([UB * p + e_p * p * (1 + UB), z], 1)


def sm_bwd_ref(p, dp, Sk):
    """softmax_bwd_kernel from the probabilities handed to it (the device's own, [rows, ld] bf16): ds = p (dp - dot), dot = sum_{k < Sk} p dp
    (products of two bf16 values: exact); columns [Sk, ld) exactly 0 whatever p and dp hold there.
    bound = storage + |p| acc_term(Sk, sum|p dp|) + 2u |p| (|dp| + |dot|)   (the subtraction and the product)"""
    ld = p.shape[1]
    P, dP = p.to(F64)[:, :Sk], dp.to(F64)[:, :Sk]
    dot = (P * dP).sum(1, keepdim=True)
    ref = P * (dP - dot)
    ev = P.abs() * acc_term(Sk, (P * dP).abs().sum(1, keepdim=True), "softmax_bwd") + 2 * U * P.abs() * (dP.abs() + dot.abs())
    z = torch.zeros(p.shape[0], ld - Sk, dtype=F64)
    return torch.cat([ref, z], 1), torch.cat([UB * ref.abs() + ev * (1 + UB), z], 1)


# ---------------------------------------------------------------------------------------------------------------- column sum (rows.hip)
CS_M = [1, 255, 256, 257, 1000]
CS_N = [1, 7, 8, 9, 255, 256, 257, 264]
CS_LD = ["N", "N+8", "N+3", "unaligned"]      # unaligned: a column slice [:, 1:] of an [M, N + 1] tensor -- ld = N + 1, base one element off 16 bytes
CS_NARROW_N = [8, 16, 32, 64, 128]
CS_NARROW_M = [32768, 32768 + 8192 + 37]      # the first M that takes the narrow kernel; a last block of 37 rows (no multiple of any rows-per-pass)
CS_ROWS = 8192                                # rows per block of the narrow kernel; 256 / (N / 8) rows per pass


CS_TALL = 32768                               # from here on the inputs are sparse (below)


def cs_tall_rows(M, gen):
    """the rows of a tall matrix that hold values: of every 8192-row block of the narrow kernel the first three rows, three around its middle, its
    last two and three anywhere; and the last 37 rows of the matrix (the ragged last block, and in it the ragged last pass of every rows-per-pass)"""
    rows = set(range(max(0, M - 37), M))
    for b in range(0, M, 8192):
        end = min(b + 8192, M)
        rows.update(r for r in (b, b + 1, b + 2, b + 4095, b + 4096, b + 4097, end - 2, end - 1) if r < end)
        rows.update(b + int(r) for r in torch.randint(0, end - b, (3,), generator=gen))
    return torch.tensor(sorted(rows))


def cs_inputs(M, N, ld_kind):
    """-> (storage [M, ld] bf16, view g = storage[:, off:off + N], ld, out0 [N] f32 non-zero).
    Below CS_TALL rows: randn.  A tall randn matrix would make the bound vacuous for what matters there -- acc_term(M + 1, sum|g|) grows like M^1.5 u,
    tens of units at M = 40997, more than a whole missing block of 37 rows -- so a tall matrix is zero except for the ~90 rows of cs_tall_rows, whose
    values are +-[1, 2) in steps of 2^-7 (out0 likewise, in [-4, 4)): sum|g| + |out0| < 200 and the bound is below 0.5, less than ANY one missing,
    doubled or misplaced element (>= 1); and every partial sum is a multiple of 2^-7 below 2^9, exact in f32, so the result is the same bits in
    every order of the atomics."""
    g = torch.Generator().manual_seed(7 * M + 13 * N + CS_LD.index(ld_kind))
    ld = {"N": N, "N+8": N + 8, "N+3": N + 3, "unaligned": N + 1}[ld_kind]
    off = 1 if ld_kind == "unaligned" else 0
    if M < CS_TALL:
        store = torch.randn(M, ld, generator=g).to(BF)
        return store, store[:, off:off + N], ld, torch.randn(N, generator=g) + 2.0
    rows = cs_tall_rows(M, g)
    grid = lambda shape, lo, hi: torch.randint(lo, hi, shape, generator=g).to(F32) / 128
    sign = torch.randint(0, 2, (len(rows), ld), generator=g).to(F32) * 2 - 1
    store = torch.zeros(M, ld, dtype=BF)
    store[rows] = (sign * grid((len(rows), ld), 128, 256)).to(BF)
    return store, store[:, off:off + N], ld, (torch.randint(0, 2, (N,), generator=g).to(F32) * 2 - 1) * grid((N,), 128, 512)


def colsum_ref(g, out0):
    """out [N] f32 = out0 + sum_m g[m, n]: M + 1 terms in any order (row lanes, LDS fold, one atomic per block); no storage term"""
    gd, o = g.to(F64), out0.to(F64)
    return o + gd.sum(0), acc_term(g.shape[0] + 1, gd.abs().sum(0) + o.abs(), "colsum")


# ---------------------------------------------------------------------------------------------------------------- add / dropout (rows.hip)
STRIDE_N = 2048 * 256 * 8 + 8 * 37            # the 2048-block grid of add / dropout strides once and leaves a ragged second pass


ADD_CASES = [(8, None), (4096, None), (4096, 8), (3 * 2048, 2048), (STRIDE_N, None), (STRIDE_N, 8)]       # (n, b_period)
DROP_N = [8, 4096, STRIDE_N]
DROP_P = [0.0, 0.1, 0.5]


def add_inputs(n, period):
    g = torch.Generator().manual_seed(5 + n + (period or 0))
    return torch.randn(n, generator=g).to(BF), torch.randn(n if period is None else period, generator=g).to(BF)


def drop_inputs(n, p):
    """-> (x bf16 [n], seed)"""
    return (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3).to(BF), 0xABCDEF12345 + int(p * 10)


def pack_inputs(N, C, H, W):
    return torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C + H)) * 3


def unpack_inputs(N, HW, C):
    return torch.randn(N, HW, C, generator=torch.Generator().manual_seed(HW + C)).to(BF)


def pool_inputs(N, H, W, C, negative=False):
    g = torch.Generator().manual_seed(C + H + W)
    return (-torch.rand(N, H, W, C, generator=g) - 0.5).to(BF) if negative else torch.randn(N, H, W, C, generator=g).to(BF)


def add_ref(a, b, b_period=None):
    """bf16(f32(a) + f32(b[i % b_period])): one add, one rounding, bit for bit"""
    bf = b.to(F32).reshape(-1)
    if b_period is not None:
        bf = bf[:b_period].repeat(a.numel() // b_period)
    return (a.to(F32).reshape(-1) + bf).to(BF).view(a.shape)


def dropout_ref(x, keep, p):
    """bf16(x * sc) where kept, sc = 1.f / (1.f - p) and the product in f32: bit for bit; +0 where dropped"""
    return torch.where(keep.view(x.shape), (x.to(F32) * f32_scale(p)).to(BF), torch.zeros((), dtype=BF))


# ---------------------------------------------------------------------------------------------------------------- embeddings (rows.hip)
EMB_D = [2, 64, 130, 768]
EMB_BL = [(1, 1), (1, 5), (5, 14)]            # n = B * L tokens: 1, 5, 70
TYPE_D = [1, 31, 32, 33, 768]
TYPE_N = [1, 7, 8, 9, 70]
PAD_ID = 1


def position_ids(ids, pad_id=PAD_ID):
    keep = ids.ne(pad_id).long()
    return torch.cumsum(keep, 1) * keep + pad_id


def emb_inputs(B, L, D, vocab=40):
    """ragged captions (pad behind them), repeated ids; tables f32"""
    g = torch.Generator().manual_seed(1000 * B + 10 * L + D)
    ids = torch.randint(3, 9, (B, L), generator=g)                     # 6 distinct words: repeats from L = 5 on
    lens = torch.randint(1, L + 1, (B,), generator=g)
    att = (torch.arange(L)[None, :] < lens[:, None]).long()
    ids = torch.where(att.bool(), ids, torch.full_like(ids, PAD_ID))
    return dict(ids=ids, att=att, word=torch.randn(vocab, D, generator=g), pos=torch.randn(L + 2, D, generator=g), type=torch.randn(2, D, generator=g))


def embed_fwd_ref(ids, pos_ids, word, pos, type0):
    """bf16((word[id] + type0) + pos[pos_id]), both sums in f32 in that order: bit for bit"""
    return ((word[ids.reshape(-1)] + type0) + pos[pos_ids.reshape(-1)]).to(BF)


def embed_type_ref(g, dtype0):
    """dtype0 [D] f32 += sum_t g[t]: n + 1 terms (8 token lanes folded in a fixed order, then the initial contents)"""
    gd, o = g.to(F64), dtype0.to(F64)
    return o + gd.sum(0), acc_term(g.shape[0] + 1, gd.abs().sum(0) + o.abs(), "embed_type_bwd")


# ---------------------------------------------------------------------------------------------------------------- elem.hip: exact kernels
PACK_C = [1, 3, 8]
PACK_NHW = [(1, 1, 1), (2, 5, 7)]
PACK_BIG = (1, 3, 1030, 1030)                 # 1 060 900 pixels > 4096 * 256: the grid strides
UNPACK = [(1, 1, 1), (2, 31, 33), (3, 32, 32), (2, 65, 264), (1, 1000, 8)]       # (N, HW, C): both tails of the 32 x 32 tile, exactly one tile, many tiles
POOL_C = [8, 64]
POOL_NHW = [(1, 1, 1), (2, 2, 2), (2, 7, 9), (3, 40, 24)]
POOL_BIG = (1, 2100, 2100, 8)                 # 1050 * 1050 outputs > 4096 * 256


def pack_ref(x):
    """f32 NCHW -> bf16 NHWC with 8 channels: bf16(x) in channels 0..C-1, exactly 0 in C..7"""
    N, C, H, W = x.shape
    out = torch.zeros(N, H, W, 8, dtype=BF)
    out[..., :C] = x.permute(0, 2, 3, 1).to(BF)
    return out


def unpack_ref(x):
    """bf16 [N, HW, C] -> f32 [N, C, HW], exact"""
    return x.to(F32).permute(0, 2, 1).contiguous()


def maxpool_ref(x):
    """bf16 NHWC -> 3x3 / s2 / p1 max pool (padding never wins: -inf), exact on the bf16 values"""
    return torch.nn.functional.max_pool2d(x.to(F32).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(BF)


# ---------------------------------------------------------------------------------------------------------------- sine position (elem.hip)
SINE_F, SINE_T = 128, 10000.0
SINE_BHW = [(1, 1, 1), (2, 5, 7), (2, 25, 42)]
SINE_BIG = (2, 96, 96)                        # 2 * 9216 * 64 threads' worth > 4096 * 256
SINE_MASKS = ["none", "random", "column", "row", "right_bottom"]
# The ROCm device library's documentation is not at hand for the error of powf / sinf / cosf, so that part of the evaluation term is MEASURED, not
# guessed: SINE_MEASURED is the largest |f32 output - fp64 reference| of toist_sine_position's NCHW output over every case of the GPU grid (MI355X,
# recorded per case as measured_sine_abs_err in row_kernel_parity.json), and the library term is 4x that maximum.
SINE_MEASURED = 8.62e-07           # 8.613e-07 at 2 x 96 x 96 with the random mask; 4.6e-07 .. 8.3e-07 on the other cases
SINE_LIB = 4 * SINE_MEASURED


def sine_mask(B, H, W, kind):
    g = torch.Generator().manual_seed(100 * H + W + SINE_MASKS.index(kind))
    m = torch.zeros(B, H, W, dtype=torch.bool)
    if kind == "random":
        m = torch.rand(B, H, W, generator=g) < 0.3
        m[:, 0, 0] = False
    elif kind == "column":
        m[:, :, W // 2] = True                # yt = 0 there: 0 / 1e-6
    elif kind == "row":
        m[:, H // 2, :] = True
    elif kind == "right_bottom":
        for b in range(B):
            m[b, H - (b + 1) * H // 4:, :] = True
            m[b, :, W - (b + 1) * W // 3:] = True
    return m


def sine_ref(mask, nf=SINE_F, temperature=SINE_T):
    """PositionEmbeddingSine(normalize=True, scale=2 pi) of toist_amd/position_encoding.py (the reference's position_encoding.py:30-49) in fp64:
    cumulative sums over unpadded cells, / (total + 1e-6) * 2 pi, / temperature ** (2 j / F), interleaved sin / cos, y half then x half.
    -> (ref, ev), both [B, H, W, 2F]: the value and the bound of the f32 evaluation (an f32 output's whole bound; a bf16 one adds storage).
      a  = cnt / (tot + 1e-6f) * 2pi_f     relative 7u: the add u (counts are exact; 1e-6 as an f32 moves tot >= 1 by far less), the division 3u,
                                           the product u, the f32 constant u, one to spare.  tot = 0 gives cnt = 0 and a = 0 exactly.
      ex = 2 j / F                         relative 3u;  dim_t = powf(T, ex) moves by relative ln(T) ex 3u, plus powf's own error (in SINE_LIB)
      th = a / dim_t                       relative 3u
    The errors of powf, sinf and cosf themselves are not derived but MEASURED (SINE_LIB above: 4x the largest error seen on the MI355X).
      sinf / cosf(th)                      |d sin| <= |d th| = |th| (13 + 3 ln(T) ex) u (7 + 3 + 3 ln(T) ex, and 3 to spare), plus the library's own error (in SINE_LIB)"""
    nm = (~mask.bool()).to(F64)
    ye, xe = nm.cumsum(1), nm.cumsum(2)
    ay = ye / (ye[:, -1:, :] + 1e-6) * (2 * math.pi)
    ax = xe / (xe[:, :, -1:] + 1e-6) * (2 * math.pi)
    ex = 2 * torch.arange(nf // 2, dtype=F64) / nf
    dim_t = temperature ** ex
    e_th = (13 + 3 * math.log(temperature) * ex) * U

    def half(a):
        th = a[..., None] / dim_t
        v = torch.stack([th.sin(), th.cos()], -1).flatten(3)
        d = (th.abs() * e_th)[..., None].expand(*th.shape, 2).flatten(3)
        return v, d
    (vy, dy), (vx, dx) = half(ay), half(ax)
    return torch.cat([vy, vx], 3), torch.cat([dy, dx], 3) + SINE_LIB


def sine_tok_ref(mask, tail=0):
    """the token output bf16 [B, H W + tail, 2F]: storage + evaluation; the tail rows exactly 0"""
    v, ev = sine_ref(mask)
    B, H, W, C = v.shape
    v, ev = v.reshape(B, H * W, C), ev.reshape(B, H * W, C)
    bound = UB * v.abs() + ev * (1 + UB)
    z = torch.zeros(B, tail, C, dtype=F64)
    return torch.cat([v, z], 1), torch.cat([bound, z], 1)


def sine_nchw_ref(mask):
    """the NCHW output f32 [B, 2F, H, W]: the evaluation term only"""
    v, ev = sine_ref(mask)
    return v.permute(0, 3, 1, 2).contiguous(), ev.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- l2norm (contrastive.hip)
L2_D = [1, 63, 64, 65, 256]
L2_ROWS = [1, 5, 130]
L2_EPS = float(torch.tensor(1e-12, dtype=F32))


def l2_inputs(rows, D):
    """f32 rows; from 5 rows on, row 2 is all zero"""
    g = torch.Generator().manual_seed(97 * rows + D)
    x, dy = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    if rows >= 5:
        x[2] = 0
    return dict(x=x, dy=dy)


def _l2_inv(xd, D):
    """inv = 1 / max(sqrtf(sum x^2), eps) and its relative error: the sum of D squares is relative (D + 2) u (positive terms; each square's rounding
    in the spare units), the square root halves it and adds 2u, the division adds 3u.  A clamped row has inv = 1 / eps: 3u."""
    ss = (xd * xd).sum(1, keepdim=True)
    e_ss = torch.full_like(ss, rb.ACC_WIDEN.get("l2norm", 1.0) * (D + 2) * U)
    nrm = ss.sqrt()
    e_inv = torch.where(nrm > L2_EPS, _inv_half(e_ss) + 5 * U, torch.full_like(ss, 3 * U))
    return 1.0 / nrm.clamp(min=L2_EPS), e_inv


def l2norm_fwd_ref(x):
    """y = x * inv: relative e_inv + u (f32 out: no storage term); an all-zero row gives exactly 0"""
    xd = x.to(F64)
    inv, e_inv = _l2_inv(xd, xd.shape[1])
    y = xd * inv
    return y, y.abs() * (e_inv + U)


def l2norm_bwd_ref(x, dy):
    """dx = (dy - y (y . dy)) inv with y = x inv re-formed per use (relative e_y = e_inv + u):
      dot = sum y dy            d_dot = acc_term(D, sum|y dy|) + (e_y + u) sum|y dy|
      dx                        inv [|y| d_dot + |y dot| (e_y + u) + u (|dy| + |y dot|)] + |dx| (e_inv + u)"""
    xd, gd = x.to(F64), dy.to(F64)
    D = xd.shape[1]
    inv, e_inv = _l2_inv(xd, D)
    y = xd * inv
    e_y = e_inv + U
    S = (y * gd).abs().sum(1, keepdim=True)
    dot = (y * gd).sum(1, keepdim=True)
    d_dot = acc_term(D, S, "l2norm") + (e_y + U) * S
    dx = (gd - y * dot) * inv
    bound = inv * (y.abs() * d_dot + (y * dot).abs() * (e_y + U) + U * (gd.abs() + (y * dot).abs())) + dx.abs() * (e_inv + U)
    return dx, bound
