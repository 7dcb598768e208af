"""Every kernel family behind toist_gemm_bf16 (csrc/gemm.hip: the eight generic tiles, the 3x3 halo kernel, the panel kernels, gemm128, gemm128w,
gemm256w, the three split-K finishes) and the fused stem (csrc/stem.hip) against the fp64 references of tests/gemm_bounds.py: EVERY output element
within the derived bound, no element excused, at the smallest shapes that sit on each family's seams (one row, a tile less or more one row / eight
columns, a k-tail, a plane of 5 x 7 pixels, a 128-row block across an image boundary, a k-slice that clamps).

Every case
  * asserts its route: the (tile, a_kind, b_kind) of every launch is read back through kernels.PROFILE; a case that ran on another family fails;
  * keeps its outputs in a wider, NaN-free, pre-filled buffer (row pitch > N where the call takes a pitch, rows before and after): everything outside
    [M, N] must come back bit-identical;
  * poisons the operands' padding with NaN where the layout admits it (columns beyond K / N inside the pitch, rows beyond M / K), and keeps the gathered
    planes of the convolutions between NaN guard rows: no output may be NaN;
  * records its worst err / bound in gemm_kernel_parity.json (gemm_bounds.hold) BEFORE asserting; the committed copy is profiles/gemm_kernel_parity.json.

Plain products are driven through kernels.gemm (the pitches, rscale, aux, a2, res_bcast and batch strides have no handle in ops) and through
ops.linear / linear_dgrad / linear_wgrad; the convolutions through ops.conv2d / conv2d_dgrad / conv2d_wgrad(_group).
tests/test_cpu_gemm_bounds.py shows that the bounds hold for a correct implementation and catch the usual mistakes."""
import contextlib

import pytest
import torch

import gemm_bounds as gb
import rounding_bounds as rb
from gemm_bounds import BF, F32, F64, TILES

pytestmark = pytest.mark.gpu
NAN = float("nan")
GR = 128                 # guard rows before and behind a gathered plane / a convolution's output (a 3x3 tap at dilation 2 reaches 2 * 47 + 2 rows)


@pytest.fixture(scope="module")
def kern():
    from toist_amd import kernels as k
    seed_dev = k.SEED_DEV
    k.SEED_DEV = None
    yield k
    k.SEED_DEV = seed_dev


def up8(n):
    return (n + 7) // 8 * 8


class Guard:
    """an output [rows, cols] inside a pre-filled NaN-free buffer [lead + rows + tail, ld]"""

    def __init__(self, dev, rows, cols, dtype, ld=None, lead=2, tail=2, seed=1, init=None):
        ld = cols if ld is None else ld
        g = torch.Generator().manual_seed(seed)
        host = torch.randn(lead + rows + tail, ld, generator=g).to(dtype)
        if init is not None:
            host[lead:lead + rows, :cols] = init.to(dtype)
        self.buf, self.before, self.box = host.to(dev), host, (lead, rows, cols)
        self.view = self.buf[lead:lead + rows, :cols]

    def start(self):
        l, r, c = self.box
        return self.before[l:l + r, :c]

    def intact(self):
        """everything outside the view is bit-identical to the pre-fill"""
        l, r, c = self.box
        now = self.buf.cpu().clone()
        now[l:l + r, :c] = self.before[l:l + r, :c]
        return torch.equal(now, self.before)


def poison(dev, t, ld, tail=2):
    """the 2-D tensor t inside a NaN buffer [rows + tail, ld]: its padding columns and the rows behind it are poison"""
    rows, cols = t.shape
    buf = torch.full((rows + tail, ld), NAN, dtype=t.dtype)
    buf[:rows, :cols] = t
    return buf.to(dev)[:rows, :cols]


def plane(dev, t):
    """an NHWC tensor between GR NaN rows (of C elements) on either side"""
    C = t.shape[-1]
    rows = t.numel() // C
    buf = torch.full((rows + 2 * GR, C), NAN, dtype=t.dtype)
    buf[GR:GR + rows] = t.reshape(rows, C)
    return buf.to(dev)[GR:GR + rows].view(t.shape)


@contextlib.contextmanager
def routed(k, tile=0):
    """FORCE_TILE for the calls whose ops entry has no tile argument, and a record of every launch's (tile, a_kind, b_kind)"""
    old = (k.FORCE_TILE, k.PROFILE)
    k.FORCE_TILE, k.PROFILE = tile, {"key": None, "records": [], "other": {}}
    keys = []
    try:
        yield keys
        torch.cuda.synchronize()
        keys.extend(r[3] for r in k.PROFILE["records"])
    finally:
        k.FORCE_TILE, k.PROFILE = old


def epi_of(t, sw, M, N):
    """the reference's epilogue operands for the switches `sw` of a case (1 = 'use the generated tensor')"""
    e = {key: v for key, v in sw.items() if key in ("alpha", "act", "drop_where", "drop_p", "drop_seed", "out_f32", "pre_out", "kernel")}
    for key in ("scale", "shift", "rscale", "res"):
        if sw.get(key):
            e[key] = t[key]
    act = sw.get("act", 0)
    if act >= gb.ACT_MASK_POS:
        e["aux"] = torch.sigmoid(t["aux"].float()).to(BF) if act == gb.ACT_SIGMOID_BWD else t["aux"]
    if sw.get("accumulate"):
        e["out0"] = t["out0"]
    return e


def run_plain(k, dev, name, M, N, K, ak, bk, tile, sw, fam="gemm_tiles", expect=None, flags=0, split_k=1, split_epilogue=False, defer=False, colsum=False,
              exact=False, calls=1):
    """one plain product through kernels.gemm with poisoned pitches and a guarded output; returns (got, ref, bound) of the output"""
    t = gb.plain_inputs(name, M, N, K, exact)
    sw = dict(sw, kernel=fam)
    e = epi_of(t, sw, M, N)
    A = poison(dev, t["A"], K + 8) if ak == k.A_ROWK else poison(dev, t["A"].t().contiguous(), up8(M) + 8)
    B = poison(dev, t["B"], K + 8) if bk == k.B_ROWK else poison(dev, t["B"].t().contiguous(), up8(N) + 8)
    f32 = bool(sw.get("out_f32"))
    ldc = N + (4 if f32 else 8)
    out = Guard(dev, M, N, F32 if f32 else BF, ld=ldc, seed=gb.seed_of(name), init=e.get("out0"))
    pre = Guard(dev, M, N, BF, ld=ldc, seed=gb.seed_of(name) + 1) if sw.get("pre_out") else None
    res = poison(dev, e["res"], N + 16) if "res" in e else None
    aux = poison(dev, e["aux"], N + 24) if "aux" in e else None
    cs = Guard(dev, 1, M, F32, ld=M + 4, lead=1, tail=1, seed=7, init=t["colsum0"].view(1, M)) if colsum else None
    dv = lambda key: e[key].to(dev) if key in e else None
    with routed(k) as keys:
        for _ in range(calls):
            k.gemm(M, N, K, ak, k.operand(A, A.stride(0)), bk, k.operand(B, B.stride(0)), out.view, ldc, tile=tile, flags=flags, split_k=split_k,
                   split_epilogue=split_epilogue, defer_reduce=defer, alpha=sw.get("alpha", 1.0), scale=dv("scale"), shift=dv("shift"), rscale=dv("rscale"),
                   res=res, ldr=N + 16 if res is not None else 0, aux=aux, ldaux=N + 24 if aux is not None else 0, act=sw.get("act", 0),
                   pre_out=pre.view if pre else None, accumulate=bool(sw.get("accumulate")), drop_where=sw.get("drop_where", 0), drop_p=sw.get("drop_p", 0.0),
                   drop_seed=sw.get("drop_seed", 0), a_colsum=cs.view.view(M) if cs else None)
        if defer:
            k.flush_reductions()
    want = (expect if expect is not None else tile & 255, ak, bk)
    assert keys == [want] * calls, f"{name}: ran on {keys}, not on {want}"
    if calls == 2:                      # two deferred calls into one output: out0 + 2 (A B^T); the second copy of the operands doubles every term
        r = gb.plain_ref(torch.cat([t["A"], t["A"]], 1), torch.cat([t["B"], t["B"]], 1), e)
    else:
        r = gb.plain_ref(t["A"], t["B"], e)
    assert out.intact() and (pre is None or pre.intact()) and (cs is None or cs.intact()), f"{name}: bytes outside the output changed"
    label = f"{fam}.{want[0]}"
    if pre:
        gb.hold(label + ".pre_out", name, pre.view, *r["pre_out"])
    if cs:
        gb.hold(label + ".a_colsum", name, cs.view.view(M), *gb.colsum_ref(torch.cat([t["A"]] * calls, 1), t["colsum0"]))
    gb.hold(label, name, out.view, *r["out"])
    return out.view, r["out"]


E_LEAN, E_GEN, E_ACC, E_MASK, E_SIG, E_DROP1, E_DROP2, ROTATE, seams = gb.E_LEAN, gb.E_GEN, gb.E_ACC, gb.E_MASK, gb.E_SIG, gb.E_DROP1, gb.E_DROP2, gb.ROTATE, gb.seams


def pairs(k):
    return [(k.A_ROWK, k.B_ROWK), (k.A_ROWK, k.B_KROW), (k.A_KROW, k.B_KROW)]


# ------------------------------------------------------------------------------------------------------------------ generic tiles
@pytest.mark.parametrize("tile", sorted(TILES))
def test_generic_tiles_at_their_seams(kern, dev, tile):
    """codes 64, 65 and 130 run every plain operand pair at every seam; the other codes rotate the pairs.  The epilogues rotate with the case, so every
    code sees the lean and the general epilogue, f32 accumulation, both dropouts and an aux activation; N % 8 == 4 always lands on the general one.
    Two of the cases of a code also run with flags bit 0 (the validation fragment path)."""
    k = kern
    i = sorted(TILES).index(tile)
    for s, (M, N, K) in enumerate(seams(tile)):
        prs = pairs(k) if tile in (64, 65, 130) else [pairs(k)[(i + s) % 3]]
        for p, (ak, bk) in enumerate(prs):
            sw = ROTATE[(i + s + 2 * p) % len(ROTATE)]
            for flags in ((0, 1) if (p == len(prs) - 1 and s in (1, 3)) else (0,)):
                run_plain(k, dev, f"t{tile}/{M}x{N}x{K}/a{ak}b{bk}/f{flags}", M, N, K, ak, bk, tile, sw, flags=flags)


@pytest.mark.parametrize("act", range(7))
def test_every_activation_on_the_lean_and_the_general_epilogue(kern, dev, act):
    """N = 72 with aligned pitches takes epilogue_lean where it implements the activation (not SIGMOID); N = 68 and an f32 output take epilogue_row8"""
    k = kern
    for N, f32 in ((72, 0), (68, 0), (72, 1)):
        run_plain(k, dev, f"act{act}/N{N}/f32{f32}", 67, N, 136, k.A_ROWK, k.B_ROWK, 65, dict(alpha=0.75, scale=1, shift=1, res=1, act=act, out_f32=f32))


@pytest.mark.parametrize("tile", [64, 65])
def test_erff_measurement(kern, dev, tile):
    """gemm_bounds.ERF_MEASURED: K = 8, operands on a 2^-4 grid and a shift on a 2^-8 grid make the pre-activation value exact in f32 (checked), so
    the f32 output's whole error is the activation's; recorded per case as measured_erf_err, and held like every other case."""
    k = kern
    for M, N in ((65, 72), (259, 136)):
        for act in (gb.ACT_GELU, gb.ACT_GELU_BWD):
            name = f"erf/t{tile}/{M}x{N}/act{act}"
            got, (ref, _) = run_plain(k, dev, name, M, N, 8, k.A_ROWK, k.B_ROWK, tile, dict(shift=1, act=act, out_f32=1), exact=True)
            t = gb.plain_inputs(name, M, N, 8, True)
            v = t["A"].to(F64) @ t["B"].to(F64).t() + t["shift"].to(F64)
            assert torch.equal(v.to(F32).to(F64), v)
            err = (got.cpu().to(F64) - ref).abs()
            w = v.abs().clamp(min=1) if act == gb.ACT_GELU else v.abs().clamp(min=2.0 ** -20)
            rb.record("erff", name, float((err / w).max()) / gb.ERF_LIB, widen=1.0, file=gb.FILE, extra={"measured_erf_err": float((err / w).max())})
            assert float((err / w).max()) <= gb.ERF_LIB


# ------------------------------------------------------------------------------------------------------------------ epilogue switches
@pytest.mark.parametrize("tile", [65, 130])
def test_residual_broadcast_second_operand_and_batch_strides(kern, dev, tile):
    k = kern
    BM = TILES[tile][0]
    # res_bcast: 3 consecutive blocks of res_mod = 50 rows share one residual map; neither 50 nor 150 divides the row tile
    M, N, K, div, mod = 2 * 150 + 37, 72, 72, 150, 50
    name = f"res_bcast/t{tile}"
    t = gb.plain_inputs(name, M, N, K)
    rows = (M + div - 1) // div * mod
    rmap = t["res"][:rows]
    m = torch.arange(M)
    e = dict(alpha=0.75, shift=t["shift"], res=rmap[(m // div) * mod + m % mod], act=gb.ACT_RELU, kernel="gemm_tiles")
    A, B, res = poison(dev, t["A"], K + 8), poison(dev, t["B"], K + 8), poison(dev, rmap, N + 16)
    out = Guard(dev, M, N, BF, ld=N + 8)
    with routed(k) as keys:
        k.gemm(M, N, K, k.A_ROWK, k.operand(A, K + 8), k.B_ROWK, k.operand(B, K + 8), out.view, N + 8, tile=tile, alpha=0.75, shift=t["shift"].to(dev), res=res,
               ldr=N + 16, act=k.ACT_RELU, res_bcast=(div, mod))
    assert keys == [(tile, k.A_ROWK, k.B_ROWK)] and out.intact()
    gb.hold(f"gemm_tiles.{tile}", name, out.view, *gb.plain_ref(t["A"], t["B"], e)["out"])
    # a2: the columns from a2_from = 128 on read their A rows from a second matrix (lean and general epilogue: N = 136 / 132)
    for N in (136, 132):
        M, K, name = BM + 5, 72, f"a2/t{tile}/N{N}"
        t, t2 = gb.plain_inputs(name, M, N, K), gb.plain_inputs(name + "/second", M, N, K)
        e = dict(alpha=1.25, shift=t["shift"], res=t["res"], kernel="gemm_tiles")
        A, A2, B, res = poison(dev, t["A"], K + 8), poison(dev, t2["A"], K + 8), poison(dev, t["B"], K + 8), poison(dev, t["res"], N + 16)
        out = Guard(dev, M, N, BF, ld=N + 8)
        with routed(k) as keys:
            k.gemm(M, N, K, k.A_ROWK, k.operand(A, K + 8), k.B_ROWK, k.operand(B, K + 8), out.view, N + 8, tile=tile, alpha=1.25, shift=t["shift"].to(dev), res=res,
                   ldr=N + 16, a2=A2, a2_from=128)
        assert keys == [(tile, k.A_ROWK, k.B_ROWK)] and out.intact()
        r1, r2 = gb.plain_ref(t["A"], t["B"], e)["out"], gb.plain_ref(t2["A"], t["B"], e)["out"]
        col = (torch.arange(N) >= 128).view(1, N)
        gb.hold(f"gemm_tiles.{tile}", name, out.view, torch.where(col, r2[0], r1[0]), torch.where(col, r2[1], r1[1]))
    # batch = 6 as 3 x 2 with distinct outer / inner strides on A, B and C (the attention products' addressing), both B kinds; the bf16 output takes
    # the lean epilogue, the f32 one the general
    for bk, f32 in ((k.B_ROWK, 0), (k.B_KROW, 0), (k.B_ROWK, 1), (k.B_KROW, 1)):
        M, N, K, name = 37, 40, 72, f"batch/t{tile}/b{bk}/f32{f32}"
        t = gb.plain_inputs(name, 6 * M, 6 * N, K)
        Az, Bz = t["A"].view(6, M, K), t["B"].view(6, N, K)
        # A: [outer][m][inner][k] (heads side by side in a packed row), B: [outer][inner][n][k] or k-major [outer][inner][k][n], C: [inner][outer][m][n]
        Ah = torch.full((3, M, 2, K + 8), NAN, dtype=BF)
        Ah[..., :K] = Az.view(3, 2, M, K).permute(0, 2, 1, 3)
        if bk == k.B_ROWK:
            Bh = torch.full((3, 2, N + 8, K), NAN, dtype=BF)
            Bh[:, :, :N] = Bz.view(3, 2, N, K)
            Bd = Bh.to(dev)
            b = k.operand(Bd, K, bs_outer=2 * (N + 8) * K, bs_inner=(N + 8) * K)
        else:
            Bh = torch.full((3, 2, K + 8, N), NAN, dtype=BF)
            Bh[:, :, :K] = Bz.view(3, 2, N, K).transpose(2, 3)
            Bd = Bh.to(dev)
            b = k.operand(Bd, N, bs_outer=2 * (K + 8) * N, bs_inner=(K + 8) * N)
        Ad = Ah.to(dev)                      # (held: operand() keeps the address only)
        out = Guard(dev, 6 * (M + 3), N, F32 if f32 else BF, ld=N + 8)
        with routed(k) as keys:
            k.gemm(M, N, K, k.A_ROWK, k.operand(Ad, 2 * (K + 8), bs_outer=M * 2 * (K + 8), bs_inner=K + 8), bk, b, out.view, N + 8, batch=6, batch_inner=2,
                   cs_outer=(M + 3) * (N + 8), cs_inner=3 * (M + 3) * (N + 8), alpha=0.5, tile=tile)
        assert keys == [(tile, k.A_ROWK, bk)] and out.intact()
        got = out.view.view(2, 3, M + 3, N)
        assert torch.equal(got[:, :, M:].cpu(), out.start().view(2, 3, M + 3, N)[:, :, M:]), "the rows between two batch entries changed"
        for z in range(6):
            gb.hold(f"gemm_tiles.{tile}", f"{name}/z{z}", got[z % 2, z // 2, :M],
                    *gb.plain_ref(Az[z], Bz[z], dict(alpha=0.5, out_f32=f32, kernel="gemm_tiles"))["out"])


def test_linear_entries_of_ops(kern, dev):
    """ops.linear / linear_dgrad / linear_wgrad on pitched views, the dispatcher's own pick at the smallest shapes auto_tile() admits for 64 (K <= 64), 65,
    132 (N <= 32, M >= 4096), 133 (M <= 32, N >= 128) and 135 (128 row tiles: panel_sized)"""
    from toist_amd import ops
    k = kern
    for M, N, K, want in ((70, 72, 64, 64), (70, 72, 72, 65), (4096, 8, 72, 132), (31, 136, 72, 133), (8129, 8, 8, 135)):
        name = f"ops.linear/{M}x{N}x{K}"
        t = gb.plain_inputs(name, M, N, K)
        x, w, res = poison(dev, t["A"], K + 8), poison(dev, t["B"], K + 8), poison(dev, t["res"], N + 16)
        out = Guard(dev, M, N, BF, ld=N + 8)
        with routed(k) as keys:
            ops.linear(x, w, t["shift"].to(dev), out=out.view, act=k.ACT_RELU, res=res, alpha=0.75, scale=t["scale"].to(dev))
        assert keys == [(want, k.A_ROWK, k.B_ROWK)] and out.intact(), keys
        fam = "gemm_panel" if want == 135 else "gemm_tiles"
        gb.hold(f"{fam}.{want}", name, out.view, *gb.plain_ref(t["A"], t["B"], dict(E_LEAN, scale=t["scale"], shift=t["shift"], res=t["res"], kernel=fam))["out"])
    M, N, K = 70, 72, 136                    # dy [M,N] w [N,K]: dx = dy w, w read k-major; then dw [N,K] += dy^T x with the bias gradient
    name = "ops.linear_dgrad"
    t = gb.plain_inputs(name, M, K, N)       # logical A [M,N], B [K,N]
    dy, w, aux = poison(dev, t["A"], N + 8), poison(dev, t["B"].t().contiguous(), K + 8), poison(dev, t["aux"], K + 24)
    out = Guard(dev, M, K, BF, ld=K + 8)
    with routed(k) as keys:
        ops.linear_dgrad(dy, w, out=out.view, act=k.ACT_GELU_BWD, aux=aux, alpha=1.25)
    assert keys == [(65, k.A_ROWK, k.B_KROW)] and out.intact()
    gb.hold("gemm_tiles.65", name, out.view, *gb.plain_ref(t["A"], t["B"], dict(alpha=1.25, act=gb.ACT_GELU_BWD, aux=t["aux"], kernel="gemm_tiles"))["out"])
    name = "ops.linear_wgrad"
    t = gb.plain_inputs(name, N, K, M)       # logical A [N,M] = dy^T, B [K,M] = x^T
    dy, x = poison(dev, t["A"].t().contiguous(), N + 8), poison(dev, t["B"].t().contiguous(), K + 8)
    out, bias = Guard(dev, N, K, F32, ld=K + 4, init=t["out0"]), Guard(dev, 1, N, F32, ld=N + 4, lead=1, tail=1, init=t["colsum0"].view(1, N))
    with routed(k) as keys:
        ops.linear_wgrad(dy, x, out=out.view, bias_out=bias.view.view(N), split_k=1)
    assert keys == [(65, k.A_KROW, k.B_KROW)] and out.intact() and bias.intact()
    gb.hold("gemm_tiles.65", name, out.view, *gb.plain_ref(t["A"], t["B"], dict(out_f32=1, out0=t["out0"], kernel="gemm_tiles"))["out"])
    gb.hold("gemm_tiles.65.a_colsum", name, bias.view.view(N), *gb.colsum_ref(t["A"], t["colsum0"]))


# ------------------------------------------------------------------------------------------------------------------ split-K finishes
@pytest.mark.parametrize("tile", [64, 65, 130])
def test_split_k_finishes_on_the_generic_tiles(kern, dev, tile):
    """GEMM_POST_REDUCE, GEMM_POST_EPILOGUE (GELU + residual + bias; bf16 and f32) and GEMM_POST_DEFERRED (once, and twice into one output before the
    flush) with 2, 3, ktiles and ktiles + 2 slices (the last clamps), K with a tail; a_colsum with per-slice rows (M % 4 == 0) and with atomics."""
    k = kern
    BK = TILES[tile][2]
    kt = 5
    K = kt * BK - 8
    for split in (2, 3, kt, kt + 2):
        for M, N in ((68, 72), (131, 68)):
            tag = f"t{tile}/{M}x{N}x{K}/s{split}"
            run_plain(k, dev, f"reduce/{tag}", M, N, K, k.A_KROW, k.B_KROW, tile, E_ACC, split_k=split, colsum=True)
            run_plain(k, dev, f"deferred/{tag}", M, N, K, k.A_KROW, k.B_KROW, tile, E_ACC, split_k=split, defer=True, colsum=True)
            for f32 in (0, 1):
                run_plain(k, dev, f"splitepi/{tag}/f32{f32}", M, N, K, k.A_ROWK, k.B_ROWK if split % 2 else k.B_KROW, tile,
                          dict(alpha=0.75, shift=1, res=1, act=gb.ACT_GELU, out_f32=f32), split_k=split, split_epilogue=True)
    run_plain(k, dev, f"deferred-twice/t{tile}", 68, 72, K, k.A_KROW, k.B_KROW, tile, dict(out_f32=1, accumulate=1), split_k=3, defer=True, calls=2)
    run_plain(k, dev, f"unsplit-colsum/t{tile}", 67, 72, K, k.A_KROW, k.B_KROW, tile, E_ACC, colsum=True)


# ------------------------------------------------------------------------------------------------------------------ panel kernels
@pytest.mark.parametrize("variant", [1, 0, 2, 3])
def test_panel_kernels(kern, dev, variant):
    """tile 135: variant 1 (panel_kernel), the default panel2_kernel and its ring variants 2 and 3; M on both sides of the 8 x 64-row minimum and of a
    row tile, N from one 8-column chunk to three column blocks and a fourth partial one, K from one MFMA step to the 256 limit"""
    k = kern
    code = 135 | variant << 8
    grid = [(449, 8, 256, E_LEAN), (512, 64, 8, E_MASK), (577, 200, 72, E_DROP1), (449, 200, 8, E_DROP2), (577, 64, 256, dict(alpha=1.25, scale=1, shift=1, res=1)),
            (512, 8, 72, E_LEAN)]
    for i, (M, N, K, sw) in enumerate(grid):
        bk = k.B_KROW if i % 2 else k.B_ROWK
        run_plain(k, dev, f"panel{variant}/{M}x{N}x{K}/b{bk}", M, N, K, k.A_ROWK, bk, code, sw, fam="gemm_panel")


# ------------------------------------------------------------------------------------------------------------------ gemm128
def test_gemm128_plain(kern, dev):
    """tile 136, row-major A with both B kinds: one row, a block and one row, two blocks and a part; K = 4, 5 and 9 k-tiles (the two 32-deep halves,
    an odd count for the cross-wave k-fold)"""
    k = kern
    grid = [(1, 136, 256, E_LEAN), (129, 8, 320, E_MASK), (300, 256, 576, E_LEAN), (129, 136, 576, dict(alpha=1.25, scale=1, shift=1, res=1)),
            (300, 8, 256, E_MASK), (1, 256, 320, E_LEAN)]
    for i, (M, N, K, sw) in enumerate(grid):
        for bk in (k.B_ROWK, k.B_KROW):
            run_plain(k, dev, f"gemm128/{M}x{N}x{K}/b{bk}", M, N, K, k.A_ROWK, bk, 136, sw, fam="gemm128")


# ------------------------------------------------------------------------------------------------------------------ convolutions
def run_conv(k, dev, name, Nb, H, W, C, Co, R, stride, pad, dil, tile, fam, want=None, passes=("fwd", "dgrad", "wgrad"), split_k=1, defer=False, f32_dgrad=False):
    """forward (scale, shift, residual, ReLU), data gradient (scale, residual, MASK_POS) and weight gradient (rscale, accumulate) of one convolution on one
    forced tile code; every launch of a pass must report the tile `want` (default: the forced code).  f32_dgrad: the data gradient into an f32 output,
    which takes the general epilogue (the row scatter and the aux mask are then epilogue_row8's, not epilogue_lean's)."""
    from toist_amd import ops
    want = tile & 255 if want is None else want
    t = gb.conv_inputs(name, Nb, H, W, C, Co, R, stride, pad, dil)
    OH, OW = t["OH"], t["OW"]
    geo = dict(stride=stride, pad=pad, dil=dil)
    x, dy, w = plane(dev, t["x"]), plane(dev, t["dy"]), t["w"].to(dev)
    label = f"{fam}.{want}"
    if "fwd" in passes:
        out = Guard(dev, Nb * OH * OW, Co, BF, lead=GR, tail=GR)
        with routed(k, tile) as keys:
            ops.conv2d(x, w, scale=t["scale"].to(dev), shift=t["shift"].to(dev), res=plane(dev, t["res"]), act=k.ACT_RELU, out=out.view.view(Nb, OH, OW, Co),
                       tile=tile, **geo)
        assert keys and all(key[0] == want and key[2] == k.B_ROWK for key in keys) and out.intact(), f"{name} fwd: {keys}"
        e = dict(scale=t["scale"], shift=t["shift"], res=t["res"].reshape(-1, Co), act=gb.ACT_RELU, kernel=fam)
        gb.hold(label, name + "/fwd", out.view, *gb.conv_fwd_ref(t["x"], t["w"], e, **geo)["out"])
    if "dgrad" in passes:
        out = Guard(dev, Nb * H * W, C, F32 if f32_dgrad else BF, lead=GR, tail=GR)
        with routed(k, tile) as keys:
            ops.conv2d_dgrad(dy, w, (H, W), scale=t["dscale"].to(dev), res=plane(dev, t["dres"]), act=k.ACT_MASK_POS, aux=plane(dev, t["daux"]),
                             out=out.view.view(Nb, H, W, C), tile=tile, **geo)
        assert keys and all(key[0] == want and key[2] == k.B_KROW for key in keys) and out.intact(), f"{name} dgrad: {keys}"
        e = dict(scale=t["dscale"], res=t["dres"].reshape(-1, C), aux=t["daux"].reshape(-1, C), act=gb.ACT_MASK_POS, out_f32=int(f32_dgrad), kernel=fam)
        ref, bound = gb.conv_dgrad_ref(t["dy"], t["w"], (H, W), e, **geo)["out"]
        got = out.view.cpu().to(F64)
        if R == 1 and stride > 1:           # the row scatter writes the pixels (oy * stride, ox * stride) only: every other row keeps the pre-fill, bit for bit
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            hit = ((yy % stride == 0) & (xx % stride == 0)).repeat(Nb, 1, 1).reshape(-1, 1)
            start = out.start().to(F64)
            ref, bound = torch.where(hit, ref, start), torch.where(hit, bound, 0 * bound)
        gb.hold(label, name + ("/dgrad-f32" if f32_dgrad else "/dgrad"), got, ref, bound)
    if "wgrad" in passes:
        out = Guard(dev, Co, R * R * C, F32, lead=3, tail=3, init=t["out0"].reshape(Co, -1))
        with routed(k, tile) as keys:
            ops.conv2d_wgrad(dy, x, (Co, R, R, C), out=out.view.view(Co, R, R, C), rscale=t["rscale"].to(dev), split_k=split_k, defer=defer, **geo)
            if defer:
                k.flush_reductions()
        assert keys and all(key[0] == want and key[1] == k.A_KROW for key in keys) and out.intact(), f"{name} wgrad: {keys}"
        e = dict(rscale=t["rscale"], out0=t["out0"].reshape(Co, -1), out_f32=1, kernel=fam)
        gb.hold(label, name + "/wgrad", out.view, *gb.conv_wgrad_ref(t["dy"], t["x"], (Co, R, R, C), e, **geo)["out"])


CONVS = gb.CONVS


@pytest.mark.parametrize("tile", [64, 65, 130, 129, 134])
@pytest.mark.parametrize("conv", CONVS, ids=[c[0] for c in CONVS])
def test_convolution_geometry_on_the_generic_tiles(kern, dev, tile, conv):
    """A_CONV x B_ROWK, A_CONVT x B_KROW (3x3 stride 1, dilation 2), A_CONV x B_KROW (the four parity classes of the 3x3 stride-2 data gradient),
    A_ROWK x B_KROW with the row scatter (1x1 stride 2) and A_KROW x B_CONVX on codes 64, 65 and 130 (and the 128-row / 128-column codes)"""
    name, *geo = conv
    run_conv(kern, dev, f"{name}/t{tile}", *geo, tile, "gemm_tiles")
    if tile in (64, 65) and geo[6] == 2:            # the strided data gradients (row scatter) once more under the general epilogue
        run_conv(kern, dev, f"{name}/t{tile}", *geo, tile, "gemm_tiles", passes=("dgrad",), f32_dgrad=True)


@pytest.mark.parametrize("H,W", [(1, 9), (7, 1), (5, 6), (8, 7)])
def test_stride2_data_gradient_parity_classes(kern, dev, H, W):
    """ops._dgrad3x3_s2 at odd and even extents; (1, 9) and (7, 1) leave two of the four parity classes empty"""
    for tile in (64, 65):
        run_conv(kern, dev, f"s2dgrad/{H}x{W}/t{tile}", 2, H, W, 64, 72, 3, 2, 1, 1, tile, "gemm_tiles", passes=("dgrad",))


def test_stem_gather_through_the_generic_tiles(kern, dev):
    """the 7x7 stride-2 gather with C = 8 and the reduction padded from 392 to 416 (taps beyond R * S are zero-filled by the gather)"""
    for tile in (64, 65, 130):
        run_conv(kern, dev, f"stem-gather/t{tile}", 2, 13, 17, 8, 64, 7, 2, 3, 1, tile, "gemm_tiles", passes=("fwd",))


@pytest.mark.parametrize("Nb,H,W", [(1, 9, 11), (3, 7, 6)])
def test_gemm128_gathers(kern, dev, Nb, H, W):
    """tile 136: the forward gather at stride 1 and 2 and the stride-1 data-gradient gather, SC = 64 (K = 576), N = 72 / 64; the strided data gradient and
    the weight gradients are not gemm128's"""
    run_conv(kern, dev, f"gemm128/3x3s1/{Nb}x{H}x{W}", Nb, H, W, 64, 72, 3, 1, 1, 1, 136, "gemm128", passes=("fwd",))
    run_conv(kern, dev, f"gemm128/3x3s1/{Nb}x{H}x{W}/dgrad", Nb, H, W, 64, 64, 3, 1, 1, 1, 136, "gemm128", passes=("dgrad",))
    run_conv(kern, dev, f"gemm128/3x3s2/{Nb}x{H}x{W}", Nb, H, W, 64, 72, 3, 2, 1, 1, 136, "gemm128", passes=("fwd",))
    run_conv(kern, dev, f"gemm128/3x3d2/{Nb}x{H}x{W}", Nb, H, W, 128, 64, 3, 1, 2, 2, 136, "gemm128", passes=("fwd", "dgrad"))


@pytest.mark.parametrize("Nb,H,W", [(1, 48, 43), (1, 44, 47), (3, 27, 26)])
def test_halo_kernel(kern, dev, Nb, H, W):
    """tile 131 (M >= 2048): the smallest admitted plane, the widest row the patch buffer takes (SW = 47), and three images whose boundaries fall inside
    128-row blocks; Co (forward) / Ci (data gradient) of one column block, one and 8 columns, two and 8 -- the gathered side stays at SC = 64, the k-tile
    of conv3_applies; the data gradient also at tile = 0 (the dispatcher's own pick)"""
    for j, Cn in enumerate((64, 72, 136)):
        run_conv(kern, dev, f"halo/{Nb}x{H}x{W}/co{Cn}", Nb, H, W, 64, Cn, 3, 1, 1, 1, 131, "gemm_conv3", passes=("fwd",))
        run_conv(kern, dev, f"halo/{Nb}x{H}x{W}/ci{Cn}", Nb, H, W, Cn, 64, 3, 1, 1, 1, 131 if j else 0, "gemm_conv3", want=131, passes=("dgrad",))


# ------------------------------------------------------------------------------------------------------------------ weight-gradient kernels
@pytest.mark.parametrize("tile", [137, 138])
def test_weight_gradient_kernels(kern, dev, tile):
    """gemm128w (137) and gemm256w (138): plain (k-major B) and gathered B (SC = 128, 3x3, stride 1 and 2), 4, 5 and 16 k-tiles, splits of 1, 2 and
    3 -> slices of 6 / 6 / 4 k-tiles (clamp_split; for 138 the 4-tile last slice is the ring-fill edge of gemm256w_applies: 8 stages >= 6), the
    deferred fold, accumulate on and off; 138 takes M = 256 and N a multiple of 128 only"""
    k = kern
    fam = "gemm128w" if tile == 137 else "gemm256w"
    Ms = (8, 72, 256) if tile == 137 else (256,)
    for i, M in enumerate(Ms):
        for N, K, split in ((128, 256, 1), (1152, 320, 1), (128, 1024, 2), (128, 1024, 3)):
            sw = dict(alpha=0.5, rscale=1, out_f32=1, accumulate=(i + split) % 2)
            run_plain(k, dev, f"{fam}/{M}x{N}x{K}/s{split}", M, N, K, k.A_KROW, k.B_KROW, tile, sw, fam=fam, split_k=split)
            if split > 1:
                run_plain(k, dev, f"{fam}/{M}x{N}x{K}/s{split}/deferred", M, N, K, k.A_KROW, k.B_KROW, tile, dict(sw, accumulate=1), fam=fam, split_k=split, defer=True)
    Co = 72 if tile == 137 else 256
    # gathered B: N = 9 * 128 = 1152, K = pixels: 4 x 8 x 8 = 256 (stride 1 on the same-size plane; stride 2 from 16 x 16), 16 x 8 x 8 = 1024 split in 3
    run_conv(k, dev, f"{fam}/convx/s1", 4, 8, 8, 128, Co, 3, 1, 1, 1, tile, fam, passes=("wgrad",))
    run_conv(k, dev, f"{fam}/convx/s2", 4, 16, 16, 128, Co, 3, 2, 1, 1, tile, fam, passes=("wgrad",))
    run_conv(k, dev, f"{fam}/convx/s1/split3", 16, 8, 8, 128, Co, 3, 1, 1, 1, tile, fam, passes=("wgrad",), split_k=3, defer=True)


@pytest.mark.parametrize("tile,n", [(137, 2), (137, 3), (138, 2), (138, 3)])
def test_grouped_weight_gradients(kern, dev, tile, n):
    """ops.conv2d_wgrad_group: n problems of one shape in one launch, every problem with its own rscale and its own running sum (out0), the outputs
    apart in one guarded buffer; unsplit, and split along K with the batched fold"""
    from toist_amd import ops
    k = kern
    fam = "gemm128w" if tile == 137 else "gemm256w"
    Nb, H, W, C, Co, R = 16, 8, 8, 128, (72 if tile == 137 else 256), 3
    for min_tiles in (1, 1 << 20):
        ts = [gb.conv_inputs(f"{fam}/group{n}/p{i}", Nb, H, W, C, Co, R, 1, 1) for i in range(n)]
        per = Co * R * R * C
        gap = 64
        out = Guard(dev, 1, n * (per + gap), F32, lead=1, tail=1,
                    init=torch.cat([torch.cat([t["out0"].reshape(-1), torch.full((gap,), 3.0)]) for t in ts]).view(1, -1))
        flat = out.view.view(-1)
        items = [(plane(dev, t["dy"]), plane(dev, t["x"]), flat[i * (per + gap): i * (per + gap) + per].view(Co, R, R, C), t["rscale"].to(dev)) for i, t in enumerate(ts)]
        old = (ops.GROUP_TILE, ops.GROUP_MIN_TILES)
        ops.GROUP_TILE, ops.GROUP_MIN_TILES = tile, min_tiles
        try:
            with routed(k) as keys:
                ops.conv2d_wgrad_group(items, (Co, R, R, C), pad=1)
                k.flush_reductions()
        finally:
            ops.GROUP_TILE, ops.GROUP_MIN_TILES = old
        assert keys == [(tile, k.A_KROW, k.B_CONVX)] and out.intact(), keys
        got = flat.cpu()
        for i, t in enumerate(ts):
            assert bool((got[i * (per + gap) + per:(i + 1) * (per + gap)] == 3.0).all()), "the gap behind a problem's output changed"
            e = dict(rscale=t["rscale"], out0=t["out0"].reshape(Co, -1), out_f32=1, kernel=fam)
            gb.hold(f"{fam}.{tile}", f"group{n}/p{i}/min_tiles{min_tiles}", got[i * (per + gap): i * (per + gap) + per].view(Co, -1),
                    *gb.conv_wgrad_ref(t["dy"], t["x"], (Co, R, R, C), e, pad=1)["out"])


# ------------------------------------------------------------------------------------------------------------------ the dispatcher's chip-sized picks
def test_automatic_picks_that_need_a_chip_sized_problem(kern, dev):
    """tile = 0 landing on 130, 134, 136, 137 and 138.  These are the only large cases of the file: auto_tile() takes 130 from 1024 tiles of 128 x 128 and
    K >= 1024, 134 from one full round of 1024 tiles of 64 x 64, gemm128_pays from 150 tiles of 128 x 128 and K >= 768, and the weight-gradient kernels
    from 128 workgroups -- the threshold shapes of tests/gemm_route_cases.py (137 wants M % 64 == 0 but not % 256, which that grid does not hold: 1088,
    the nearest above its 1024); no smaller problem reaches these rungs of the ladder.  130 and 134 carry a GELU, which gemm128 (ahead of them on the
    ladder) does not take."""
    k = kern
    run_plain(k, dev, "auto/130", 16384, 1024, 1024, k.A_ROWK, k.B_ROWK, 0, dict(E_LEAN, act=gb.ACT_GELU), expect=130)
    run_plain(k, dev, "auto/134", 17000, 256, 1024, k.A_ROWK, k.B_KROW, 0, dict(E_LEAN, act=gb.ACT_GELU), expect=134)
    run_plain(k, dev, "auto/136", 19200, 128, 768, k.A_ROWK, k.B_ROWK, 0, E_LEAN, fam="gemm128", expect=136)
    run_plain(k, dev, "auto/137", 1088, 1024, 1024, k.A_KROW, k.B_KROW, 0, E_ACC, fam="gemm128w", expect=137, split_k=2)
    run_plain(k, dev, "auto/138", 1024, 1024, 1024, k.A_KROW, k.B_KROW, 0, E_ACC, fam="gemm256w", expect=138, split_k=4, defer=True)


# ------------------------------------------------------------------------------------------------------------------ fused stem
@pytest.mark.parametrize("N,H,W", [(1, 7, 9), (2, 13, 17), (1, 71, 93), (3, 40, 24)])
def test_fused_stem(kern, dev, N, H, W):
    k = kern
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    img = torch.randn(N, 3, H, W, generator=g)
    w8 = torch.nn.functional.pad(torch.randn(64, 7, 7, 3, generator=g) * (2.0 / 147) ** 0.5, (0, 5)).to(BF).contiguous()
    shift = torch.randn(64, generator=g) * 0.3
    OH, OW = gb.out_hw(H, W, 7, 7, 2, 3)
    PH, PW = gb.out_hw(OH, OW, 3, 3, 2, 1)
    out = Guard(dev, N * PH * PW, 64, BF, lead=GR, tail=GR)
    k.stem_fwd(img.to(dev), w8.to(dev), shift.to(dev), out.view.view(N, PH, PW, 64))
    assert out.intact()
    ref, bound = gb.stem_ref(img, w8, shift)
    gb.hold("stem_fwd", f"{N}x{H}x{W}", out.view, ref.reshape(-1, 64), bound.reshape(-1, 64))
