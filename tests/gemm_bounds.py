"""fp64 references with a derived per-element error bound for the bf16 GEMM / implicit-convolution family (csrc/gemm.hip: the generic tiles, the
3x3 halo kernel, the panel kernels, gemm128, gemm128w, gemm256w and the three split-K finishes) and the fused stem (csrc/stem.hip), in the manner of
tests/rounding_bounds.py, whose U, UB, acc_term, ratio, record, check and round_bf16 they use.  Shared by tests/test_cpu_gemm_bounds.py (f32 torch
emulations with the kernels' block structure inside every bound, named mutants outside it) and tests/test_gpu_gemm_kernels.py.  Not a conftest and
not a test.

Every reference takes the CPU bf16 / f32 tensors the kernel takes and returns (ref, bound), fp64, shaped like the output; a kernel is right when
|got - ref| <= bound for EVERY element.  No element is excused and there is no flip rule: ReLU is 1-Lipschitz, and MASK_POS, the *_BWD activations
and dropout decide from exact bf16 / hashed inputs.  The terms follow epilogue_row8 (csrc/gemm.hip) line by line, none tuned (u = 2^-24, ub = 2^-8):

  accumulation  acc = sum_k A[m][k] B[n][k] over n real products (exact in f32; a tap outside the plane is an exact zero and adds nothing to the
                magnitude), then e f32 operations of the epilogue: one unit each for v *= alpha [* rscale[m]] (two with rscale: the product
                alpha * rscale[m] is formed first), * scale[n], + shift[n], + res, += out0, and three for a dropout (1 - p, 1 / that, the product).
                For ANY summation order the term is acc_term(n + e, S): S is the same fp64 operator on |A|, |B|, carried through
                |alpha rscale[m] scale[n]| (and the dropout factor), plus |shift[n]| + |res| + |out0|.  One formula therefore covers MFMA blocking, the
                32-deep halves of gemm128, the cross-wave k-fold, k-slice partials in every finish, and the f32 atomics of a_colsum.
  storage       ub |ref| for a bf16 output or pre_out (times 1 + ub on the rest: the f32 value, not ref, was rounded); none for an f32 output.
  activation    ReLU and MASK_POS add nothing.  GELU, SIGMOID and the two *_BWD carry the pre-activation bound b through the function's Lipschitz
                constant ON [v - b, v + b] (computed in fp64, not a global constant) and add a library term: relative E_EXP = 2^-14 for __expf (the
                allowance of rounding_bounds.attnmap_fwd_ref and tests/attn_bounds.py), ERF_LIB = 4 * ERF_MEASURED for erff (below).
  dropout       the keep mask of oracle.xdec_ref.elem_keep (element m * N + n): a dropped element is exactly 0 (drop_where = 2) or exactly the
                residual (drop_where = 1; bound 0 under no activation / ReLU / MASK_POS, else the activation's own terms).
  a_colsum      out0[m] + sum_k A[m][k]: acc_term(K + 1, |out0| + sum|A|).

ACC_WIDEN (rounding_bounds) holds a factor on the accumulation term alone under the kernel names of WIDEN_KEYS; none is in force."""
import math
import zlib

import torch

import rounding_bounds as rb
from oracle.xdec_ref import elem_keep
from rounding_bounds import BF, F32, F64, U, UB, acc_term, check, ratio, record, round_bf16  # noqa: F401  (the contract's names)
from row_bounds import pack_ref

F = torch.nn.functional
FILE = "gemm_kernel_parity.json"
WIDEN_KEYS = ["gemm_tiles", "gemm_conv3", "gemm_panel", "gemm128", "gemm128w", "gemm256w", "stem_fwd"]
E_EXP = 2.0 ** -14
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_MASK_POS, ACT_GELU_BWD, ACT_SIGMOID_BWD = range(7)        # TOIST_ACT_* (include/toist_hip.h)

# MEASURED: the largest |f32 output - fp64 reference| / max(1, |v|) of the GELU cases, and / |v| of the GELU_BWD
# cases, of tests/test_gpu_gemm_kernels.py::test_erff_measurement on an MI355X (recorded per case as measured_erf_err in gemm_kernel_parity.json).  Those cases have K = 8 and operands on a 2^-4
# grid, alpha = 1 and a shift on a 2^-8 grid, so the pre-activation value v is EXACT in f32: the propagated part is 0 and all of the error is erff /
# __expf and the three or four f32 operations around them.  The library term is 4x the maximum.
ERF_MEASURED = 1.656e-07          # 1.6559e-07 on GELU_BWD at 259 x 136 (tile 64); 1.29e-07 .. 1.59e-07 on its other cases, 9.30e-08 on every GELU case
ERF_LIB = 4 * ERF_MEASURED


def widen_of(kernel):
    for key in sorted(WIDEN_KEYS, key=len, reverse=True):
        if kernel.startswith(key):
            return rb.ACC_WIDEN.get(key, 1.0)
    return 1.0


def hold(kernel, case, got, ref, bound):
    """record, then assert: every element inside its bound, none NaN"""
    g = got.detach().cpu().to(F64)
    r = rb.record(kernel, case, ratio(g, ref, bound), widen=widen_of(kernel), file=FILE)
    assert not bool(torch.isnan(g).any()), f"{kernel} [{case}]: NaN in the output"
    assert r <= 1.0, f"{kernel} [{case}]: max err/bound {r}"
    return r


def f32v(x):
    """a Python float as the f32 the C interface receives"""
    return float(torch.tensor(x, dtype=F32))


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------------- activations in fp64
R2, RPI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / R2))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / R2)) + x * torch.exp(-0.5 * x * x) / RPI


def gelu_lip(lo, hi):
    """max |gelu'| on [lo, hi]: gelu'' = phi(x) (2 - x^2) vanishes at +-sqrt 2 only, so the extrema are the end points and those two"""
    m = torch.maximum(gelu_grad(lo).abs(), gelu_grad(hi).abs())
    for x0 in (R2, -R2):
        g0 = float(gelu_grad(torch.tensor(x0, dtype=F64)).abs())
        m = torch.where((lo <= x0) & (x0 <= hi), m.clamp(min=g0), m)
    return m


def sigmoid_lip(lo, hi):
    d = lambda x: torch.sigmoid(x) * (1 - torch.sigmoid(x))
    return torch.where((lo <= 0) & (0 <= hi), torch.full_like(lo, 0.25), torch.maximum(d(lo), d(hi)))


# ---------------------------------------------------------------------------------------------------------------- the epilogue
def epilogue(acc, S, n, e):
    """acc, S [M,N] fp64 (the sum and the sum of magnitudes), n = real products per element (int or [M,1] / [M,N] tensor), e = dict of the
    epilogue's operands (CPU tensors / floats; absent = NULL): alpha, rscale [M], scale [N], shift [N], res [M,N], aux [M,N], act, drop_where,
    drop_p, drop_seed, out0 [M,N] (accumulate), out_f32, pre_out (bool), kernel (the ACC_WIDEN key).
    Returns {"out": (ref, bound)[, "pre_out": (ref, bound)]}."""
    g = lambda k, d=None: e.get(k, d)
    M, N = acc.shape
    kern, act = g("kernel"), g("act", ACT_NONE)
    f = torch.full((M, 1), f32v(g("alpha", 1.0)), dtype=F64)
    ops = 1
    if g("rscale") is not None:
        f, ops = f * g("rscale").to(F64).view(M, 1), ops + 1
    if g("scale") is not None:
        f, ops = f * g("scale").to(F64).view(1, N), ops + 1
    v, S = acc * f, S * f.abs()
    if g("shift") is not None:
        v, S, ops = v + g("shift").to(F64).view(1, N), S + g("shift").to(F64).abs().view(1, N), ops + 1
    keep, sc = None, 1.0
    if g("drop_where", 0):
        keep = elem_keep(M, N, g("drop_p"), g("drop_seed"))
        sc = 1.0 / (1.0 - f32v(g("drop_p")))
    exact = torch.zeros(M, N, dtype=torch.bool)           # elements whose pre-activation value is exact: dropped before the residual
    if g("drop_where", 0) == 1:
        v, S, ops = torch.where(keep, v * sc, 0 * v), torch.where(keep, S * sc, 0 * S), ops + 3
        exact = ~keep
    if g("res") is not None:
        v, S, ops = v + g("res").to(F64), S + g("res").to(F64).abs(), ops + 1
    late = act == ACT_NONE and g("drop_where", 0) != 2
    if g("out0") is not None and late:                    # C += v with nothing in between: one more term of the same sum
        pre_v, pre_S, pre_ops = v, S, ops
        v, S, ops = v + g("out0").to(F64), S + g("out0").to(F64).abs(), ops + 1
    else:
        pre_v, pre_S, pre_ops = v, S, ops
    b = torch.where(exact & (g("out0") is None), 0 * S, acc_term(n + ops, S, kern))
    res = {}
    if g("pre_out"):
        bp = torch.where(exact, 0 * S, acc_term(n + pre_ops, pre_S, kern))
        res["pre_out"] = (pre_v, torch.where(exact, 0 * S, UB * pre_v.abs() + bp * (1 + UB)))
    aux = g("aux").to(F64) if g("aux") is not None else None
    if act == ACT_RELU:
        y = v.clamp(min=0)
    elif act == ACT_GELU:           # 0.5 v (1 + erff(v c)): erff's error times |v| / 2, and the products' roundings, relative to max(1, |v|)
        y, b = gelu(v), gelu_lip(v - b, v + b) * b + ERF_LIB * v.abs().clamp(min=1)
    elif act == ACT_SIGMOID:        # 1 / (1 + __expf(-v)): d s / d t = -s^2, t E_EXP -> s (1 - s) E_EXP; the sum and the quotient 4u s
        y = torch.sigmoid(v)
        b = sigmoid_lip(v - b, v + b) * b + y * (1 - y) * E_EXP + 4 * U * y
    elif act == ACT_MASK_POS:
        y, b = torch.where(aux > 0, v, 0 * v), torch.where(aux > 0, b, 0 * b)
    elif act == ACT_GELU_BWD:       # v * gelu'(aux), aux exact: the factor's own error (erff, __expf, five f32 operations) times |v|
        y = v * gelu_grad(aux)
        b = gelu_grad(aux).abs() * b + ERF_LIB * v.abs() + (aux * torch.exp(-0.5 * aux * aux) / RPI).abs() * E_EXP * v.abs() + 2 * U * y.abs()
    elif act == ACT_SIGMOID_BWD:    # v * (aux * (1 - aux)): three f32 operations
        y = v * aux * (1 - aux)
        b = (aux * (1 - aux)).abs() * b + 4 * U * y.abs()
    else:
        y = v
    if g("drop_where", 0) == 2:
        y, b = torch.where(keep, y * sc, 0 * y), torch.where(keep, b * sc + 3 * U * (y * sc).abs(), 0 * b)
    if g("out0") is not None and not late:                # C += act(v): one f32 sum behind the activation
        y = y + g("out0").to(F64)
        b = b + U * y.abs()
    if not g("out_f32"):
        plain = act in (ACT_NONE, ACT_RELU, ACT_MASK_POS) and g("drop_where", 0) != 2
        b = torch.where(exact & plain, 0 * b, UB * y.abs() + b * (1 + UB))      # a dropped element is the bf16 residual itself
    res["out"] = (y, b)
    return res


# ---------------------------------------------------------------------------------------------------------------- operators
def plain_ref(A, B, e):
    """A [M,K], B [N,K] (bf16, the LOGICAL matrices of any of A_ROWK / A_KROW x B_ROWK / B_KROW): C = epilogue(A B^T), n = K"""
    Ad, Bd = A.to(F64), B.to(F64)
    return epilogue(Ad @ Bd.t(), Ad.abs() @ Bd.abs().t(), A.shape[1], e)


def colsum_ref(A, out0):
    """a_colsum [M] = out0[m] + sum_k A[m][k] (f32, atomics or per-slice rows folded in slice order)"""
    Ad = A.to(F64)
    ref, S = out0.to(F64) + Ad.sum(1), out0.to(F64).abs() + Ad.abs().sum(1)
    return ref, acc_term(A.shape[1] + 1, S, "a_colsum")


def out_hw(H, W, R, S, stride, pad, dil=1):
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (S - 1) - 1) // stride + 1


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv_fwd_ref(x, w, e, stride=1, pad=0, dil=1):
    """A_CONV x B_ROWK: x [Nb,H,W,C], w [Co,R,S,C] -> [Nb*OH*OW, Co]; n = (taps inside the plane) * C per pixel"""
    run = lambda a, b: F.conv2d(_nchw(a), _nchw(b), stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1)
    xd, wd = x.to(F64), w.to(F64)
    Co, C = w.shape[0], x.shape[-1]
    acc, S = run(xd, wd).reshape(-1, Co), run(xd.abs(), wd.abs()).reshape(-1, Co)
    n = run(torch.ones_like(xd[..., :1]), torch.ones_like(wd[:1, :, :, :1])).reshape(-1, 1) * C
    return epilogue(acc, S, n, e)


def conv_dgrad_ref(dy, w, in_hw, e, stride=1, pad=0, dil=1):
    """A_CONVT x B_KROW (and the parity classes / the row scatter of the strided ones): dy [Nb,OH,OW,Co], w [Co,R,S,C] -> dx [Nb*H*W, C].
    A pixel no tap reaches has n = 0: its value is the epilogue of an exact zero."""
    H, W = in_hw
    Nb, OH, OW, Co = dy.shape
    R, S_, C = w.shape[1], w.shape[2], w.shape[3]
    op = (H - ((OH - 1) * stride - 2 * pad + dil * (R - 1) + 1), W - ((OW - 1) * stride - 2 * pad + dil * (S_ - 1) + 1))
    run = lambda a, b: F.conv_transpose2d(_nchw(a), _nchw(b), stride=stride, padding=pad, dilation=dil, output_padding=op).permute(0, 2, 3, 1)
    dd, wd = dy.to(F64), w.to(F64)
    acc, S = run(dd, wd).reshape(-1, C), run(dd.abs(), wd.abs()).reshape(-1, C)
    n = run(torch.ones_like(dd[..., :1]), torch.ones_like(wd[:1, :, :, :1])).reshape(-1, 1) * Co
    return epilogue(acc, S, n, e)


def conv_wgrad_ref(dy, x, w_shape, e, stride=1, pad=0, dil=1):
    """A_KROW x B_CONVX (B_KROW for 1x1): dw [Co, R*S*C] = sum over the P output pixels of dy (x) gathered x; n = P"""
    Co, R, S_, C = w_shape
    run = lambda a, b: torch.nn.grad.conv2d_weight(_nchw(b), (Co, C, R, S_), _nchw(a), stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1)
    dd, xd = dy.to(F64), x.to(F64)
    P = dy.shape[0] * dy.shape[1] * dy.shape[2]
    return epilogue(run(dd, xd).reshape(Co, -1), run(dd.abs(), xd.abs()).reshape(Co, -1), P, e)


def stem_ref(img, w8, shift):
    """toist_stem_fwd: the image rounded by pack_ref, conv 7x7 / 2 / pad 3, + shift, ReLU, max-pool 3x3 / 2 / pad 1 -> [N,PH,PW,64] bf16.  Max and
    ReLU are 1-Lipschitz: a pooled element's bound is the largest conv-element bound of its window (n = 147 products + the shift) plus storage."""
    x = pack_ref(img)
    r = conv_fwd_ref(x[..., :3].contiguous(), w8[..., :3].contiguous(), dict(shift=shift, out_f32=1, kernel="stem_fwd"), stride=2, pad=3)["out"]
    N, H, W = img.shape[0], img.shape[2], img.shape[3]
    OH, OW = out_hw(H, W, 7, 7, 2, 3)
    pool = lambda t: F.max_pool2d(_nchw(t.reshape(N, OH, OW, 64)), 3, 2, 1).permute(0, 2, 3, 1)
    ref, b = pool(r[0].clamp(min=0)), pool(r[1])
    return ref, UB * ref.abs() + b * (1 + UB)


# ---------------------------------------------------------------------------------------------------------------- inputs
def plain_inputs(name, M, N, K, exact=False):
    """A [M,K], B [N,K] bf16 (B scaled by (2 / K)^0.5: outputs O(1)) and every epilogue operand, seeded by the case's name.  exact: operands on a 2^-4
    grid and a shift on a 2^-8 grid (test_erff_measurement: the pre-activation value is exact in f32)."""
    g = torch.Generator().manual_seed(seed_of(name))
    rn = lambda *s: torch.randn(*s, generator=g)
    if exact:
        A, B = (torch.round(rn(M, K) * 8).clamp(-24, 24) / 16).to(BF), (torch.round(rn(N, K) * 8).clamp(-24, 24) / 16).to(BF)
        shift = torch.round(rn(N) * 128) / 256
    else:
        A, B, shift = rn(M, K).to(BF), (rn(N, K) * (2.0 / K) ** 0.5).to(BF), rn(N)
    return dict(A=A, B=B, shift=shift, scale=torch.rand(N, generator=g) + 0.5, rscale=torch.rand(M, generator=g) + 0.5, res=rn(M, N).to(BF),
                aux=rn(M, N).to(BF), out0=rn(M, N), colsum0=rn(M))


def conv_inputs(name, Nb, H, W, C, Co, R, stride, pad, dil=1):
    """x [Nb,H,W,C], w [Co,R,R,C] scaled by (2 / (R R C))^0.5, dy [Nb,OH,OW,Co], and epilogue operands for the forward ([.., Co]) and the data
    gradient ([.., C])"""
    g = torch.Generator().manual_seed(seed_of(name))
    rn = lambda *s: torch.randn(*s, generator=g)
    OH, OW = out_hw(H, W, R, R, stride, pad, dil)
    return dict(x=rn(Nb, H, W, C).to(BF), w=(rn(Co, R, R, C) * (2.0 / (R * R * C)) ** 0.5).to(BF), dy=rn(Nb, OH, OW, Co).to(BF),
                scale=torch.rand(Co, generator=g) + 0.5, shift=rn(Co), res=rn(Nb, OH, OW, Co).to(BF), dscale=torch.rand(C, generator=g) + 0.5,
                dres=rn(Nb, H, W, C).to(BF), daux=rn(Nb, H, W, C).to(BF), rscale=torch.rand(Co, generator=g) + 0.5, out0=rn(Co, R, R, C), OH=OH, OW=OW)


TILES = {64: (64, 64, 32), 65: (64, 64, 64), 128: (128, 128, 32), 129: (128, 128, 64), 130: (128, 64, 64), 132: (128, 32, 64), 133: (32, 128, 64),
         134: (64, 128, 64)}            # tile code -> BM, BN, BK (include/toist_hip.h)


# the epilogues the grids rotate through: every switch with non-trivial operands; (switches, needs the general epilogue)
E_LEAN = dict(alpha=0.75, scale=1, shift=1, res=1, act=ACT_RELU)
E_GEN = dict(alpha=1.25, rscale=1, shift=1, res=1, pre_out=1, act=ACT_GELU)
E_ACC = dict(alpha=0.5, rscale=1, out_f32=1, accumulate=1)
E_MASK = dict(alpha=-1.5, scale=1, res=1, act=ACT_MASK_POS)
E_SIG = dict(alpha=1.0, scale=1, shift=1, out_f32=1, act=ACT_SIGMOID)
E_DROP1 = dict(alpha=0.75, shift=1, res=1, drop_where=1, drop_p=0.25, drop_seed=0x1234567890)
E_DROP2 = dict(alpha=1.0, scale=1, shift=1, res=1, act=ACT_RELU, drop_where=2, drop_p=0.1, drop_seed=77)
ROTATE = [E_LEAN, E_GEN, E_ACC, E_MASK, E_SIG, E_DROP1, E_DROP2]


def seams(tile):
    """four (M, N, K) per tile code: every seam of M {1, BM - 1, BM + 1, 2 BM + 3}, N {8, BN - 8, BN + 8} and one N % 8 == 4, K {8, BK - 8, BK, 2 BK + 8}"""
    BM, BN, BK = TILES[tile]
    return [(1, BN + 8, BK - 8), (BM - 1, 8, 2 * BK + 8), (BM + 1, BN - 8, 8), (2 * BM + 3, BN + 4, BK)]


# (name, Nb, H, W, C, Co, R, stride, pad, dil): planes as small as n = 2, 5 x 7; channel counts 8, 64, 72, 128
CONVS = [("3x3s1", 2, 5, 7, 8, 72, 3, 1, 1, 1), ("3x3s2", 2, 5, 7, 64, 8, 3, 2, 1, 1), ("3x3d2", 1, 9, 11, 72, 64, 3, 1, 2, 2), ("1x1s2", 2, 5, 7, 128, 64, 1, 2, 0, 1),
         ("3x3s2even", 3, 8, 6, 72, 128, 3, 2, 1, 1)]
