"""fp64 references with a derived per-element error bound for the mask-head kernels (csrc/maskstage.hip, csrc/smallconv.hip, csrc/segm.hip),
shared by tests/test_cpu_mask_head_bounds.py (torch emulations of the kernels' arithmetic, and mutants of them) and the GPU tests
tests/test_gpu_mask_head_kernels.py / tests/test_gpu_attnmap.py.  Not a conftest and not a test.

Every reference takes the bf16 / f32 tensors the kernel takes (on the CPU) and returns (ref, bound), both fp64 and shaped like the kernel's
output; a kernel is right when |got - ref| <= bound for EVERY element.  `bound` is a sum of at most three terms, none of them tuned:

  storage        a bf16 output is the round-to-nearest of the f32 value v the kernel formed: |bf16(v) - v| <= u/(1+u) |v| with u = 2^-8 (p = 8
                 significand bits), so the term is 2^-8 |ref|.  The slack u^2/(1+u) |ref| it leaves absorbs that v, not ref, was rounded.  An f32
                 output has no such term.
  accumulation   v is a sum of n terms t_i (products of two bf16 values are exact in f32), summed in f32 in an order the kernel chooses (MFMA
                 blocks, lanes, waves, atomics).  For ANY order |v - sum t_i| <= (n-1) 2^-24 sum|t_i| to first order; the term is
                 (n + 2) 2^-24 S with S = sum|t_i| obtained by running the SAME fp64 operator on absolute values (|w|, |x|, + |bias| + |res|).
                 The three spare units cover the second-order part and the (1 + 2^-8) factor of the storage argument above.
  flippable      where a kernel rounds an INTERMEDIATE to bf16 before using it (the GroupNorm + ReLU input of the gn_in stages: ms_pack8v in
                 maskstage.hip), the reference rounds the fp64 value the same way; the two roundings can only differ when the fp64 value lies
                 within the f32 evaluation error `delta` of a rounding tie (the result moves by one bf16 ulp) or of the ReLU kink (it moves by at
                 most 2 delta).  Those inputs are marked and the term is sum ulp(a_i) |w_i| over them: the same convolution applied to the
                 (mask * ulp) tensor with |w|.  See gn_coeffs for delta.

ACC_WIDEN holds, per kernel, a factor on the accumulation term alone (1 = as derived); a GPU run that needs another value states it there."""
import json
import os

import torch

F = torch.nn.functional
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24            # unit roundoff of f32
UB = 2.0 ** -8            # unit roundoff of bf16
EPS = 1e-5
G = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured figures go to $TOIST_PARITY_OUT (default: parity_out/ in the tree, ignored by git); the committed copy is profiles/mask_head_kernel_parity.json
RECORD = os.path.join(os.environ.get("TOIST_PARITY_OUT") or os.path.join(ROOT, "parity_out"), "mask_head_kernel_parity.json")

ACC_WIDEN = {}            # kernel name -> factor on the accumulation term (none needed so far)


# ---------------------------------------------------------------------------------------------------------------- number formats
def round_bf16(v):
    """fp64 -> nearest bf16 value (ties to even), as fp64.  Exact: no detour through f32 (which would round twice)."""
    _, e = torch.frexp(v)                                 # |v| = m 2^e, m in [0.5, 1): 8 significand bits -> ulp 2^(e-8)
    q = torch.ldexp(torch.ones_like(v), e - 8)
    return torch.round(v / q) * q                         # torch.round is half-to-even; v / q is exact (a power of two)


def bf16_ulp(v):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 8)


def tie_distance(v):
    """distance from v to the nearest bf16 rounding tie (the midpoints of v's own binade; v = 0 has none: inf)"""
    q = bf16_ulp(v)
    frac = v.abs() / q
    d = (frac - torch.floor(frac) - 0.5).abs() * q
    return torch.where(v == 0, torch.full_like(v, float("inf")), d)


def acc_term(n, S, kernel=None):
    return ACC_WIDEN.get(kernel, 1.0) * (n + 2) * U * S


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0, x / 0 as inf)"""
    err = (got.detach().cpu().to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def record(kernel, case, value, widen=None, file=None, extra=None):
    """{kernel, case, max err/bound, widening factor} into RECORD (one entry per kernel and case), BEFORE the assertion.
    file: another file name beside RECORD (tests/row_bounds.py: row_kernel_parity.json); extra: further fields of the entry (a measured constant)"""
    path = RECORD if file is None else os.path.join(os.path.dirname(RECORD), file)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    rows = {}
    if os.path.exists(path):
        try:
            with open(path) as f:
                rows = {(r["kernel"], r["case"]): r for r in json.load(f)}
        except (ValueError, KeyError):
            rows = {}
    rows[(kernel, case)] = {"kernel": kernel, "case": case, "max_err_over_bound": round(value, 4) if value == value and value != float("inf") else str(value),
                            "acc_widen": widen if widen is not None else ACC_WIDEN.get(kernel, 1.0)}
    if extra:
        rows[(kernel, case)].update(extra)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(rows[k]) for k in sorted(rows)) + "\n]\n")
    return value


def check(kernel, case, got, ref, bound, file=None, widen=None):
    r = record(kernel, case, ratio(got, ref, bound), widen=widen, file=file)
    assert r <= 1.0, f"{kernel} [{case}]: max err/bound {r}"


def rel(a, b):
    a, b = a.detach().cpu().to(F64), b.detach().cpu().to(F64)
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------- GroupNorm (csrc/segm.hip)
def gn_stats_ref(x, C):
    """x [N,HW,C] -> ({sum, sum of squares} [N,G,2], bound).  n = HW * C/G terms each (v * v of a bf16 v is exact in f32): accumulation term only."""
    N, HW = x.shape[0], x.shape[1]
    xd = x.to(F64).reshape(N, HW, G, C // G)
    ref = torch.stack([xd.sum((1, 3)), (xd * xd).sum((1, 3))], -1)
    S = torch.stack([xd.abs().sum((1, 3)), (xd * xd).sum((1, 3))], -1)
    return ref, acc_term(HW * (C // G), S, "groupnorm_stats")


def gn_coeffs(stats, gamma, beta, HW, C, eps=EPS):
    """The affine form y = x * a + b the kernels evaluate (gn_apply_kernel, mask_stage_kernel) from stats [N,G,2], in fp64, per (n, c), with
    the error of the f32 evaluation.  With u = 2^-24, a division within 3u and rsqrtf within 2u:
      mean = s0 / cnt                      rel 3u
      var  = max(s1 / cnt - mean^2, 0)     abs u (3 E2 + 7 mean^2) + u var       (E2 = s1 / cnt; mean * mean carries 2 * 3u + u)
           -> rel e_v of (var + eps) = u (3 E2 + 7 mean^2) / (var + eps) + 2u  -- the cancellation factor: (E2 + mean^2) / var = 1 + 2 mean^2 / var
      rs   = rsqrtf(var + eps)             rel e_rs = e_v / (2 (1 - e_v)) + 2u   ((1-x)^-1/2 <= 1 + x / (2 (1-x)))
      a    = rs * gamma                    rel e_a = e_rs + u
      b    = beta - mean * a               abs d_b = |mean a| (e_a + 4u) + u |b|
    Returns a dict of [N,C] fp64 tensors (mean, rs, a, b, e_rs, e_a, d_b)."""
    Cg = C // G
    cnt = float(HW * Cg)
    s = stats.to(F64)
    mean, e2 = s[..., 0] / cnt, s[..., 1] / cnt
    var = (e2 - mean * mean).clamp(min=0)
    e_v = U * (3 * e2.abs() + 7 * mean * mean) / (var + eps) + 2 * U
    e_rs = torch.where(e_v < 1, 0.5 * e_v / (1 - e_v).clamp(min=1e-300), torch.full_like(e_v, float("inf"))) + 2 * U
    rs = (var + eps).rsqrt()
    ch = torch.arange(C) // Cg
    mean, var, rs, e_rs = mean[:, ch], var[:, ch], rs[:, ch], e_rs[:, ch]
    a = rs * gamma.to(F64)
    e_a = e_rs + U
    b = beta.to(F64) - mean * a
    d_b = (mean * a).abs() * (e_a + 4 * U) + U * b.abs()
    return dict(mean=mean, var=var, rs=rs, a=a, b=b, e_rs=e_rs, e_a=e_a, d_b=d_b)


def gn_affine(x, co):
    """x [N,...,C] -> (v, delta): the pre-ReLU value x * a + b in fp64 and the bound of its f32 evaluation, delta = |x a| (e_a + u) + d_b + u |v|
    (product -- or one fused multiply-add -- and sum)"""
    shp = (x.shape[0],) + (1,) * (x.dim() - 2) + (x.shape[-1],)
    xa = x.to(F64) * co["a"].view(shp)
    v = xa + co["b"].view(shp)
    return v, xa.abs() * (co["e_a"].view(shp) + U) + co["d_b"].view(shp) + U * v.abs()


def gn_apply_ref(x, stats, gamma, beta, relu, eps=EPS):
    """groupnorm_apply / the second pass of groupnorm_fwd from GIVEN statistics (the kernel's own): y [N,HW,C] bf16.
    storage + the evaluation error delta (ReLU is 1-Lipschitz).  Also returns (v, delta) for the ReLU-ambiguity condition."""
    co = gn_coeffs(stats, gamma, beta, x.shape[1], x.shape[2], eps)
    v, delta = gn_affine(x, co)
    y = v.clamp(min=0) if relu else v
    return y, UB * y.abs() + delta * (1 + UB), (v, delta)


def gn_true_ref(x, gamma, beta, relu, eps=EPS):
    """y against the TRUE fp64 GroupNorm of x alone (the offset case: |mean| ~ 4 std, where E[x^2] - mean^2 cancels).  The kernel's statistics
    are within B0, B1 (gn_stats_ref) of the true sums, so mean moves by d_m <= B0 / cnt and var by d_v <= B1 / cnt + 2 |mean| d_m + d_m^2;
    y = (x - mean) r gamma + beta with r = (var + eps)^-1/2 has dy/dmean = -r gamma and dy/dvar = -(x - mean) gamma r^3 / 2, hence
    bound = storage + [delta + |r gamma| d_m + |x - mean| |gamma| r^3 d_v / 2] (first order in d_m, d_v)."""
    N, HW, C = x.shape
    sums, sb = gn_stats_ref(x, C)
    co = gn_coeffs(sums, gamma, beta, HW, C, eps)
    v, delta = gn_affine(x, co)
    cnt = float(HW * (C // G))
    ch = torch.arange(C) // (C // G)
    d_m = (sb[..., 0] / cnt)[:, ch]
    d_v = (sb[..., 1] / cnt)[:, ch] + 2 * co["mean"].abs() * d_m + d_m * d_m
    gm = gamma.to(F64).abs()
    prop = (co["rs"] * gm * d_m).unsqueeze(1) + 0.5 * (x.to(F64) - co["mean"].unsqueeze(1)).abs() * (gm * co["rs"] ** 3 * d_v).unsqueeze(1)
    y = v.clamp(min=0) if relu else v
    return y, UB * y.abs() + (delta + prop) * (1 + UB)


def gn_bwd_ref(dy, x, stats, gamma, beta, relu, y=None, bstats=None, dgamma0=None, dbeta0=None, eps=EPS):
    """groupnorm_bwd from the kernel's own statistics.  With g = dy * mask, xh = (x - mean) rs:
      bstats[n][grp] = {sum g gamma, sum g gamma xh}   dgamma[c] += sum g xh   dbeta[c] += sum g   dx = rs (g gamma - m1 - xh m2), m = bstats / cnt
    mask: y > 0 of the GIVEN y (exact), or -- y None -- x * a + b > 0 re-derived in f32: an element with |v| <= delta may take either side
    (`flip`), which moves dx by rs |dy gamma| and each sum by that element's term.
    f32 evaluation: d_xh = rs 4u (|x| + |mean|) + |xh| (e_rs + u);  dx: rs (|m2| d_xh + 6u T) + (e_rs + u) |dx| with T = |g gamma| + |m1| + |xh m2|.
    dx is evaluated from `bstats` when given (the kernel's own), so it is checked apart from the sums.
    Returns dict name -> (ref, bound) for dx, bstats, dgamma, dbeta, and n_flip."""
    N, HW, C = x.shape
    Cg = C // G
    cnt = float(HW * Cg)
    co = gn_coeffs(stats, gamma, beta if beta is not None else torch.zeros(C), HW, C, eps)
    xd, dyd, gm = x.to(F64), dy.to(F64), gamma.to(F64)
    u1 = lambda t: t.unsqueeze(1)
    flip = torch.zeros_like(xd, dtype=torch.bool)
    if not relu:
        m = torch.ones_like(xd)
    elif y is not None:
        m = (y.to(F64) > 0).to(F64)
    else:
        v, delta = gn_affine(x, co)
        m = (v > 0).to(F64)
        flip = v.abs() <= delta
    g = dyd * m
    fl = flip.to(F64) * dyd.abs()                         # what a flipped mask adds or removes
    xh = (xd - u1(co["mean"])) * u1(co["rs"])
    d_xh = u1(co["rs"]) * 4 * U * (xd.abs() + u1(co["mean"]).abs()) + xh.abs() * (u1(co["e_rs"]) + U)
    grp = lambda t: t.reshape(N, HW, G, Cg).sum((1, 3))
    t0, t1 = g * gm, g * gm * xh
    bs_ref = torch.stack([grp(t0), grp(t1)], -1)
    n = HW * Cg
    bs_bound = torch.stack([acc_term(n + 2, grp(t0.abs()), "groupnorm_bwd") + grp(fl * gm.abs()),
                            acc_term(n + 2, grp(t1.abs()), "groupnorm_bwd") + grp((g * gm).abs() * d_xh) + grp(fl * (gm * xh).abs())], -1)
    dg0 = dgamma0.to(F64) if dgamma0 is not None else torch.zeros(C, dtype=F64)
    db0 = dbeta0.to(F64) if dbeta0 is not None else torch.zeros(C, dtype=F64)
    dg_ref, db_ref = dg0 + (g * xh).sum((0, 1)), db0 + g.sum((0, 1))
    dg_bound = acc_term(N * HW + 1, (g * xh).abs().sum((0, 1)) + dg0.abs(), "groupnorm_bwd") + (g.abs() * d_xh).sum((0, 1)) + (fl * xh.abs()).sum((0, 1))
    db_bound = acc_term(N * HW + 1, g.abs().sum((0, 1)) + db0.abs(), "groupnorm_bwd") + fl.sum((0, 1))
    bs = bstats.to(F64) if bstats is not None else bs_ref
    ch = torch.arange(C) // Cg
    m1, m2 = u1((bs[..., 0] / cnt)[:, ch]), u1((bs[..., 1] / cnt)[:, ch])
    rs = u1(co["rs"])
    dx = rs * (g * gm - m1 - xh * m2)
    T = (g * gm).abs() + m1.abs() + (xh * m2).abs()
    d_dx = rs * (m2.abs() * d_xh + 6 * U * T) + (u1(co["e_rs"]) + U) * dx.abs()
    dx_bound = UB * dx.abs() + d_dx * (1 + UB) + rs * fl * gm.abs()
    return dict(dx=(dx, dx_bound), bstats=(bs_ref, bs_bound), dgamma=(dg_ref, dg_bound), dbeta=(db_ref, db_bound), n_flip=int(flip.sum()))


def gn_inputs(C, HW, N=3, offset=0.0, seed=None):
    g = torch.Generator().manual_seed(GN_SEEDS.get((C, HW), 7000 + 13 * C + HW) if seed is None else seed)
    x = (torch.randn(N, HW, C, generator=g) + offset).to(BF)
    dy = torch.randn(N, HW, C, generator=g).to(BF)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, dg0=dg0, db0=db0)


GN_C = [16, 32, 64, 128, 264]
GN_HW = [1, 7, 130, 513, 1601]
GN_SEEDS = {(16, 1601): 9000}             # (C, HW) -> seed, where the default seed leaves a pre-ReLU value within delta of zero (tests/test_cpu_mask_head_bounds.py checks)


# ---------------------------------------------------------------------------------------------------------------- 3x3 convolutions
def conv3x3(x, w, dgrad=False):
    """x [N,H,W,Cs], w [Co,3,3,Ci] (fp64) -> 3x3 / s1 / p1 convolution [N,H,W,Co], or its data gradient [N,H,W,Ci] (x = dy [N,H,W,Co])"""
    xn, wn = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    y = F.conv_transpose2d(xn, wn, padding=1) if dgrad else F.conv2d(xn, wn, padding=1)
    return y.permute(0, 2, 3, 1)


def small_conv_ref(src, w, shift, res, dgrad):
    """conv3x3_small: out bf16 = conv(src, w) [+ shift per channel] [+ res].  n = 9 * c_src products + shift + res; storage + accumulation."""
    sd, wd = src.to(F64), w.to(F64)
    ref, S = conv3x3(sd, wd, dgrad), conv3x3(sd.abs(), wd.abs(), dgrad)
    if shift is not None:
        ref, S = ref + shift.to(F64), S + shift.to(F64).abs()
    if res is not None:
        ref, S = ref + res.to(F64), S + res.to(F64).abs()
    return ref, UB * ref.abs() + acc_term(9 * src.shape[-1] + 2, S, "conv3x3_small")


def wgrad_ref(dy, x, out0):
    """wgrad3x3_small with accumulate: out [Co,3,3,C] f32 = out0 + sum over the P pixels of dy[p, co] x[p + tap, ci].  n = P + 1; no storage term."""
    dd, xd = dy.to(F64), x.to(F64)
    N, H, W, C = x.shape

    def run(a, b):
        bp = F.pad(b, (0, 0, 1, 1, 1, 1))
        return torch.stack([torch.stack([torch.einsum("nhwo,nhwc->oc", a, bp[:, r:r + H, s:s + W]) for s in range(3)], 1) for r in range(3)], 1)
    ref, S = run(dd, xd) + out0.to(F64), run(dd.abs(), xd.abs()) + out0.to(F64).abs()
    return ref, acc_term(N * H * W + 1, S, "wgrad3x3_small")


SMALL_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 7, 16), (2, 4, 33), (1, 20, 17)]
SMALL_FWD = [(32, 16), (16, 8), (32, 32), (8, 16), (16, 4)]
SMALL_DGRAD = [(16, 32), (8, 16), (32, 32)]             # (c_src = Co of w, c_out = Ci of w)
WGRAD_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 6, 32), (3, 9, 11), (2, 20, 17)]
WGRAD_CH = [(16, 8), (16, 16), (32, 8), (32, 16)]


def small_inputs(shape, c_src, c_out, dgrad):
    n, H, W = shape
    g = torch.Generator().manual_seed(100000 * n + 1000 * H + 10 * W + c_src + 3 * c_out + (7 if dgrad else 0))
    src = torch.randn(n, H, W, c_src, generator=g).to(BF)
    wshape = (c_src, 3, 3, c_out) if dgrad else (c_out, 3, 3, c_src)
    w = (torch.randn(wshape, generator=g) * (2.0 / (9 * c_src)) ** 0.5).to(BF)
    return dict(src=src, w=w, shift=torch.randn(c_out, generator=g), res=torch.randn(n, H, W, c_out, generator=g).to(BF))


def wgrad_inputs(shape, C, Co):
    n, H, W = shape
    g = torch.Generator().manual_seed(200000 * n + 1000 * H + 10 * W + C + 3 * Co)
    return dict(dy=torch.randn(n, H, W, Co, generator=g).to(BF), x=torch.randn(n, H, W, C, generator=g).to(BF), out0=torch.randn(Co, 3, 3, C, generator=g))


# ---------------------------------------------------------------------------------------------------------------- fused stages (csrc/maskstage.hip)
STAGES = {"lay4": (64, 32, False, True), "lay5": (32, 16, True, True), "out_lay": (16, 1, True, False)}      # c_in, c_out, gn_in, up
STAGE_SHAPES = {"lay4": [(2, 2), (16, 16), (18, 34), (30, 14), (4, 66)], "lay5": [(2, 2), (16, 16), (18, 34), (30, 14), (4, 66)],
                "out_lay": [(1, 1), (16, 16), (17, 33), (5, 50), (33, 3)]}
STAGE_SEEDS = {("out_lay", 1, 1): 9000}          # (stage, H, W) -> seed, as GN_SEEDS


def stage_inputs(stage, H, W, B=2, Q=3, seed=None):
    cin, cout, gn_in, up = STAGES[stage]
    default = 500 + 1000 * list(STAGES).index(stage) + 37 * H + W
    g = torch.Generator().manual_seed(STAGE_SEEDS.get((stage, H, W), default) if seed is None else seed)
    N = B * Q
    SH, SW = (H // 2, W // 2) if up else (H, W)
    src = (torch.randn(N, SH, SW, cin, generator=g) * 1.5 + 0.3).to(BF)
    if not gn_in:
        src = src.clamp(min=0)
    t = dict(src=src, w=(torch.randn(cout, 3, 3, cin, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(BF), Q=Q, stage=stage, H=H, W=W,
             bias=None if up else torch.randn(cout, generator=g) * 0.1, gamma=None, beta=None, stats=None,
             fpn_conv=torch.randn(B, H, W, cout, generator=g).to(BF) if up else None)       # one FPN term per IMAGE, all different
    if gn_in:
        t["gamma"], t["beta"] = 1 + 0.2 * torch.randn(cin, generator=g), 0.2 * torch.randn(cin, generator=g)
        t["stats"] = gn_stats_ref(src.reshape(N, SH * SW, cin), cin)[0].to(F32)             # host fp64 sums, handed over as f32
    return t


def up2(a):
    return a.repeat_interleave(2, 1).repeat_interleave(2, 2)


def mask_stage_ref(t, stats=None, rounding=True, src64=None):
    """mask_stage_fwd: [GroupNorm + ReLU of src from `stats`, rounded to bf16] -> [nearest 2x] -> 3x3 conv [+ bias] [+ fpn_conv of image n // Q].
    ref [N,H,W,c_out] fp64 (the raw value: a bf16 output's storage term is in `bound`; c_out == 1 is the f32 output: no storage term).
    n = 9 c_in + 2 terms.  rounding=False (and src64, an fp64 source) is the same chain with no bf16 rounding anywhere, for the storage floor
    measured in test_cpu_mask_head_bounds.py.  Returns (ref, bound, info) with info = {flippable fraction, outputs with a zero flippable term,
    n_ambiguous: inputs whose pre-ReLU value is within delta of zero}."""
    cin, cout, gn_in, up = STAGES[t["stage"]]
    x = src64 if src64 is not None else t["src"].to(F64)
    N, SH, SW, _ = x.shape
    wd = t["w"].to(F64)
    info = dict(flippable=0.0, zero_flip_outputs=1.0, n_ambiguous=0)
    flipmag = torch.zeros_like(x)
    if gn_in:
        co = gn_coeffs(stats if stats is not None else t["stats"], t["gamma"], t["beta"], SH * SW, cin)
        v, delta = gn_affine(x, co)
        r = v.clamp(min=0)
        if rounding:
            kink = v.abs() <= delta
            tie = (tie_distance(r) <= delta) & (r > 0)
            flipmag = tie.to(F64) * bf16_ulp(r) + kink.to(F64) * 2 * delta
            info.update(flippable=float((kink | tie).double().mean()), n_ambiguous=int(kink.sum()))
            r = round_bf16(r)
        x = r
    if up:
        x, flipmag = up2(x), up2(flipmag)
    ref, S, fterm = conv3x3(x, wd), conv3x3(x.abs(), wd.abs()), conv3x3(flipmag, wd.abs())
    if t["bias"] is not None:
        ref, S = ref + t["bias"].to(F64), S + t["bias"].to(F64).abs()
    if up:
        f = t["fpn_conv"].to(F64).repeat_interleave(t["Q"], 0)
        ref, S = ref + f, S + f.abs()
    info["zero_flip_outputs"] = float((fterm == 0).double().mean())
    bound = acc_term(9 * cin + 2, S, "mask_stage_fwd") + fterm
    if cout != 1:
        bound = bound + UB * ref.abs()
    return ref, bound, info


def stage_stats_ref(out):
    """out_stats of a stage against the fp64 sums of the ROUNDED output the kernel wrote, out [N,H,W,c_out] bf16: n 2^-24 sum|v| (and v^2), n = H W c_out/8"""
    N, H, W, C = out.shape
    o = out.to(F64).reshape(N, H * W, G, C // G)
    ref = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
    S = torch.stack([o.abs().sum((1, 3)), (o * o).sum((1, 3))], -1)
    return ref, ACC_WIDEN.get("mask_stage_stats", 1.0) * (H * W * (C // G)) * U * S


# ---------------------------------------------------------------------------------------------------------------- resample and sum kernels
UPS_HW = [(1, 1), (3, 5), (8, 9)]
UPS_C = [8, 16, 64, 264]
SUMQ_Q = [1, 3, 100]


def ups_inputs(H, W, C, BQ=6, Q=3):
    g = torch.Generator().manual_seed(31 * H + 7 * W + C)
    return dict(inp=torch.randn(BQ, H, W, C, generator=g).to(BF), fpn=torch.randn(BQ // Q, 2 * H, 2 * W, C, generator=g).to(BF),
                dout=torch.randn(BQ, 2 * H, 2 * W, C, generator=g).to(BF))


def upsample_add_ref(inp, fpn, Q):
    """one add and one rounding: bf16(f32(fpn[n // Q]) + f32(up2(in))), bit for bit (bound 0); formed in f32, as specified"""
    ref = (up2(inp.to(F32)) + fpn.to(F32).repeat_interleave(Q, 0)).to(BF).to(F64)
    return ref, torch.zeros_like(ref)


def upsample_add_bwd_ref(dout):
    """din = the sum of the 2 x 2 output pixels that read it: n = 4; storage + accumulation"""
    d = dout.to(F64)
    N, OH, OW, C = d.shape
    fold = lambda a: a.reshape(N, OH // 2, 2, OW // 2, 2, C).sum((2, 4))
    ref = fold(d)
    return ref, UB * ref.abs() + acc_term(4, fold(d.abs()), "upsample_add_bwd")


def sum_queries_ref(inp, B, Q):
    d = inp.to(F64).reshape(B, Q, -1)
    ref = d.sum(1)
    return ref, UB * ref.abs() + acc_term(Q, d.abs().sum(1), "sum_queries")


# ---------------------------------------------------------------------------------------------------------------- attention-map softmax
ATT_HW = [1, 63, 64, 65, 130, 300]
ATT_PADS = ["none", "first", "last", "middle"]


def attnmap_inputs(HW, extra_ld, pad, B=2, Q=3, H=8):
    """scores [B,Q,H,ld] bf16 with |v - max| <= 64 per row, ld = HW rounded up to 8 (+ extra_ld); key_pad [B,HW] u8 or None (never a whole image)"""
    g = torch.Generator().manual_seed(17 * HW + extra_ld + ATT_PADS.index(pad))
    ld = (HW + 7) // 8 * 8 + extra_ld
    s = (torch.randn(B, Q, H, ld, generator=g) * 6).clamp(-30, 30).to(BF)
    kp = None
    if pad != "none" and HW > 1:
        kp = torch.zeros(B, HW, dtype=torch.uint8)
        if pad == "first":
            kp[:, 0] = 1
        elif pad == "last":
            kp[:, HW - 1] = 1
        else:
            kp[0, HW // 3:HW // 3 + max(1, HW // 4)] = 1
            kp[1, HW // 2:HW // 2 + max(1, HW // 5)] = 1
        assert int(kp.sum(1).max()) < HW
    return dict(scores=s, key_pad=kp, ld=ld, HW=HW, B=B, Q=Q, H=H, dprob=torch.randn(B * Q, HW, H, generator=g).to(BF))


def attnmap_fwd_ref(t):
    """softmax over the HW keys of each (b, q, head); output channels-last [BQ,HW,H] bf16; padded keys exactly 0 (bound 0 there).
    bound = 2^-8 ref (1 + 2^-6): storage, plus a relative 2^-14 for __expf (argument scaling <= 64 * 2^-24 for |v - max| <= 64, a few ulp of the
    hardware exponent) and the HW-term sum -- 64 times smaller than the storage term, so it cannot hide a wrong element."""
    B, Q, H, HW = t["B"], t["Q"], t["H"], t["HW"]
    s = t["scores"].to(F64)[..., :HW]
    if t["key_pad"] is not None:
        s = s.masked_fill(t["key_pad"].bool()[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1).reshape(B * Q, H, HW).permute(0, 2, 1).contiguous()
    return p, UB * p * (1 + 2.0 ** -6)


def attnmap_bwd_ref(prob, dprob, ld):
    """dscores [BQ,H,ld] = P (dP - sum_p P dP) from the DEVICE's probabilities [BQ,HW,H]; columns [HW, ld) exactly zero.
    storage + |P| (HW + 2) 2^-24 sum|P dP| (the dot product's accumulation, carried through the factor P)"""
    P, dP = prob.to(F64).permute(0, 2, 1), dprob.to(F64).permute(0, 2, 1)          # [BQ,H,HW]
    HW = P.shape[-1]
    dot = (P * dP).sum(-1, keepdim=True)
    ref = P * (dP - dot)
    bound = UB * ref.abs() + P.abs() * ACC_WIDEN.get("attnmap_softmax_bwd", 1.0) * (HW + 2) * U * (P * dP).abs().sum(-1, keepdim=True)
    padc = torch.zeros(P.shape[0], P.shape[1], ld - HW, dtype=F64)
    return torch.cat([ref, padc], -1), torch.cat([bound, padc], -1)
