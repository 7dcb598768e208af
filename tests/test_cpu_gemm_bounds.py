"""The bounds of tests/gemm_bounds.py are neither wrong nor vacuous: torch f32 EMULATIONS with the kernels' block structure -- k-tiles of 32 and 64 with
one partial sum per MFMA depth (16 / 32), the two 32-deep halves of gemm128, k-slices folded in slice order, partials of four waves folded pairwise;
the tap loop of the gathers, the four parity classes of the stride-2 data gradient, the row scatter, the grouped launch -- followed by epilogue_row8
in f32, stay within `bound` on every case of the grid (the seams of tests/test_gpu_gemm_kernels.py), and named mutants of the emulation, the ways
such kernels go wrong, leave it on the case named beside them.  The references read rounding_bounds.ACC_WIDEN when called, so an entry there is in
force for the mutants too."""
import pytest
import torch

import gemm_bounds as gb
from gemm_bounds import BF, F32, F64, TILES, UB
from oracle.xdec_ref import elem_keep

F = torch.nn.functional


def f32t(x):
    return torch.tensor(x, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------ accumulation structures
def acc_tiles(A, B, bk, depth, drop_tail=False):
    """k-tiles of bk, one MFMA partial sum per `depth` products, added to the accumulator in k order.  drop_tail: the k-tail tile is never staged."""
    K = A.shape[1]
    kend = K // bk * bk if drop_tail else K
    acc = torch.zeros(A.shape[0], B.shape[0])
    for k0 in range(0, kend, depth):
        acc = acc + A[:, k0:k0 + depth] @ B[:, k0:k0 + depth].t()
    return acc


def acc_halves(A, B):
    """gemm128: every 64-deep k-tile feeds two accumulators, one per 32-deep half, added at the end"""
    K = A.shape[1]
    lo, hi = torch.zeros(A.shape[0], B.shape[0]), torch.zeros(A.shape[0], B.shape[0])
    for k0 in range(0, K, 64):
        lo = lo + A[:, k0:k0 + 32] @ B[:, k0:k0 + 32].t()
        hi = hi + A[:, k0 + 32:k0 + 64] @ B[:, k0 + 32:k0 + 64].t()
    return lo + hi


def acc_slices(A, B, bk, split, overlap=False):
    """split-K: slices of ceil(ktiles / split) k-tiles, folded in slice order.  overlap: every slice but the last also takes the next slice's first k-tile."""
    K = A.shape[1]
    ktiles = (K + bk - 1) // bk
    split = min(split, ktiles)
    kper = (ktiles + split - 1) // split
    acc = torch.zeros(A.shape[0], B.shape[0])
    for s in range((ktiles + kper - 1) // kper):
        k0, k1 = s * kper * bk, min((s + 1) * kper, ktiles) * bk + (bk if overlap else 0)
        acc = acc + acc_tiles(A[:, k0:k1], B[:, k0:k1], bk, 32)
    return acc


def acc_waves(A, B, bk=64):
    """k-tiles dealt to four waves, the four partials folded pairwise"""
    K = A.shape[1]
    part = [torch.zeros(A.shape[0], B.shape[0]) for _ in range(4)]
    for i, k0 in enumerate(range(0, K, bk)):
        part[i % 4] = part[i % 4] + A[:, k0:k0 + bk] @ B[:, k0:k0 + bk].t()
    return (part[0] + part[1]) + (part[2] + part[3])


STRUCTURES = {"tiles32x16": lambda A, B: acc_tiles(A, B, 32, 16), "tiles64x32": lambda A, B: acc_tiles(A, B, 64, 32), "halves": acc_halves,
              "slices3": lambda A, B: acc_slices(A, B, 64, 3), "slices2x32": lambda A, B: acc_slices(A, B, 32, 2), "waves4": acc_waves}


# ------------------------------------------------------------------------------------------------------------------ epilogue_row8 in f32
def trunc_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(F32)


def emu_epilogue(acc, e, mutant=None):
    """epilogue_row8 line by line in f32 on an f32 accumulator; e as gemm_bounds.epilogue takes it.  -> (out, pre_out or None), as f32 / bf16 tensors"""
    g = lambda k, d=None: e.get(k, d)
    M, N = acc.shape
    rs = f32t(g("alpha", 1.0)) * g("rscale").view(M, 1) if g("rscale") is not None else f32t(g("alpha", 1.0))
    v = acc * rs
    if mutant == "scale_after_shift":
        v = (v + g("shift").view(1, N)) * g("scale").view(1, N)
    else:
        if g("scale") is not None:
            v = v * g("scale").view(1, N)
        if g("shift") is not None:
            v = v + g("shift").view(1, N)
    dw = g("drop_where", 0)
    if dw:
        keep, sc = elem_keep(M, N, g("drop_p"), g("drop_seed")), f32t(1.0) / (f32t(1.0) - f32t(g("drop_p")))
    if dw == 1:
        v = torch.where(keep, v * sc, torch.zeros_like(v))
    if g("res") is not None:
        r = g("res").float()
        v = v + (torch.roll(r, -1, 0) if mutant == "res_next_row" else r)
    pre = v.to(BF) if g("pre_out") else None
    act, aux = g("act", 0), g("aux").float() if g("aux") is not None else None
    c = f32t(0.70710678118654752)
    gelu_grad = lambda a: f32t(0.5) * (1 + torch.erf(a * c)) + a * f32t(0.3989422804014327) * torch.exp(f32t(-0.5) * a * a)
    if act == gb.ACT_RELU:
        v = v.clamp(min=0)
    elif act == gb.ACT_GELU:
        v = f32t(0.5) * v * (1 + torch.erf(v * c))
    elif act == gb.ACT_SIGMOID:
        v = 1 / (1 + torch.exp(-v))
    elif act == gb.ACT_MASK_POS:
        v = torch.where(aux > 0, v, torch.zeros_like(v))
    elif act == gb.ACT_GELU_BWD:
        v = v * gelu_grad(aux)
    elif act == gb.ACT_SIGMOID_BWD:
        v = v * (aux * (1 - aux))
    if dw == 2:
        v = torch.where(keep, v * sc, torch.zeros_like(v))
    if g("out_f32"):
        return (v if g("out0") is None or mutant == "accumulate_overwrites" else g("out0") + v), pre
    return (trunc_bf16(v) if mutant == "truncated" else v.to(BF).float()), pre


def epi_of(t, sw, fam="gemm_tiles"):
    e = {key: v for key, v in sw.items() if key in ("alpha", "act", "drop_where", "drop_p", "drop_seed", "out_f32", "pre_out")}
    e["kernel"] = fam
    for key in ("scale", "shift", "rscale", "res"):
        if sw.get(key):
            e[key] = t[key]
    if sw.get("act", 0) >= gb.ACT_MASK_POS:
        e["aux"] = torch.sigmoid(t["aux"].float()).to(BF) if sw["act"] == gb.ACT_SIGMOID_BWD else t["aux"]
    if sw.get("accumulate"):
        e["out0"] = t["out0"]
    return e


def plain_grid():
    """(name, M, N, K, switches, family): the seams of every generic tile with the rotating epilogues, and the panel / gemm128 / weight-gradient shapes"""
    out = []
    for i, tile in enumerate(sorted(TILES)):
        for s, (M, N, K) in enumerate(gb.seams(tile)):
            out.append((f"t{tile}/{M}x{N}x{K}", M, N, K, gb.ROTATE[(i + s) % len(gb.ROTATE)], "gemm_tiles"))
    for M, N, K, sw in ((449, 8, 256, gb.E_LEAN), (512, 64, 8, gb.E_MASK), (577, 200, 72, gb.E_DROP1), (449, 200, 8, gb.E_DROP2)):
        out.append((f"panel/{M}x{N}x{K}", M, N, K, sw, "gemm_panel"))
    for M, N, K, sw in ((1, 136, 256, gb.E_LEAN), (129, 8, 320, gb.E_MASK), (300, 256, 576, gb.E_LEAN)):
        out.append((f"gemm128/{M}x{N}x{K}", M, N, K, sw, "gemm128"))
    for M, N, K in ((8, 128, 256), (72, 1152, 320), (256, 128, 1024)):
        out.append((f"gemm128w/{M}x{N}x{K}", M, N, K, gb.E_ACC, "gemm128w"))
    for act in range(7):
        out.append((f"act{act}", 67, 72, 136, dict(alpha=0.75, scale=1, shift=1, res=1, act=act), "gemm_tiles"))
        out.append((f"act{act}/f32", 67, 72, 136, dict(alpha=0.75, scale=1, shift=1, res=1, act=act, out_f32=1), "gemm_tiles"))
    return out


GRID = plain_grid()


def inside(got, ref, bound):
    return gb.ratio(got, ref, bound) <= 1.0


def run_case(case, structure="tiles64x32", mutant=None, acc=None):
    name, M, N, K, sw, fam = case
    t = gb.plain_inputs(name, M, N, K)
    e = epi_of(t, sw, fam)
    a = STRUCTURES[structure](t["A"].float(), t["B"].float()) if acc is None else acc(t["A"].float(), t["B"].float())
    got, pre = emu_epilogue(a, e, mutant)
    r = gb.plain_ref(t["A"], t["B"], e)
    return got, pre, r


@pytest.mark.parametrize("structure", sorted(STRUCTURES))
def test_every_block_structure_stays_inside_the_bound_on_the_whole_grid(structure):
    for case in GRID:
        got, pre, r = run_case(case, structure)
        assert inside(got, *r["out"]), (structure, case[0], gb.ratio(got, *r["out"]))
        if pre is not None:
            assert inside(pre, *r["pre_out"]), (structure, case[0], "pre_out")


def test_the_bound_is_not_vacuous():
    """the median bound / |ref| of every bf16 output stays below 2^-7 (a bf16 ulp is 2^-8 .. 2^-7 of the value)"""
    for case in GRID:
        if case[4].get("out_f32"):
            continue
        _, _, r = run_case(case)
        ref, bound = r["out"]
        live = ref != 0
        if bool(live.any()):
            assert float((bound[live] / ref[live].abs()).median()) < 2.0 ** -7, case[0]


def test_the_erff_term_is_far_below_the_storage_term():
    assert gb.ERF_LIB == 4 * gb.ERF_MEASURED and gb.ERF_LIB <= UB / 64
    for case in GRID:
        if case[4].get("act") in (gb.ACT_GELU, gb.ACT_GELU_BWD) and not case[4].get("out_f32"):
            _, _, r = run_case(case)
            ref = r["out"][0]
            lib = gb.ERF_LIB * ref.abs().clamp(min=1)            # an upper estimate of the term on either activation (|gelu(v)| <= |v|, |gelu'| < 1.13)
            assert float((lib / (UB * ref.abs())).median()) <= 1.0 / 64, case[0]


def case_named(name):
    return next(c for c in GRID if c[0] == name)


# ------------------------------------------------------------------------------------------------------------------ mutants of the plain products
PLAIN_MUTANTS = {       # mutant -> (case, how the emulation goes wrong)
    "k_tail_dropped": ("t65/63x8x136", dict(acc=lambda A, B: acc_tiles(A, B, 64, 32, drop_tail=True))),           # K % BK = 8: the last 8 products never summed
    "k_tile_in_two_slices": ("t65/259x68x64", None),                                                              # (replaced below: needs several k-tiles)
    "res_next_row": ("t130/259x68x64", dict(mutant="res_next_row")),
    "scale_after_shift": ("t130/259x68x64", dict(mutant="scale_after_shift")),
    "accumulate_overwrites": ("gemm128w/72x1152x320", dict(mutant="accumulate_overwrites")),
    "truncated": ("t130/259x68x64", dict(mutant="truncated")),
}
PLAIN_MUTANTS["k_tile_in_two_slices"] = ("gemm128w/256x128x1024", dict(acc=lambda A, B: acc_slices(A, B, 64, 3, overlap=True)))


@pytest.mark.parametrize("mutant", sorted(PLAIN_MUTANTS))
def test_plain_mutants_leave_the_bound(mutant):
    name, kw = PLAIN_MUTANTS[mutant]
    case = case_named(name)
    good, _, r = run_case(case)
    assert inside(good, *r["out"])
    got, _, r = run_case(case, **kw)
    assert not inside(got, *r["out"]), (mutant, name)


def test_last_partial_tile_reading_the_neighbours_row_or_column():
    """a row tile of 64 over M = 65: the tile's last row clamps to row M of the buffer (the neighbour's first row) instead of M - 1; likewise the last
    column block (N = 72, BN = 64) reading column N"""
    name, M, N, K = "edge/65x72x72", 65, 72, 72
    t, nb = gb.plain_inputs(name, M, N, K), gb.plain_inputs(name + "/neighbour", M, N, K)
    e = epi_of(t, gb.E_LEAN)
    ref, bound = gb.plain_ref(t["A"], t["B"], e)["out"]
    assert inside(emu_epilogue(acc_tiles(t["A"].float(), t["B"].float(), 64, 32), e)[0], ref, bound)
    A = torch.cat([t["A"][:M - 1], nb["A"][:1]]).float()
    assert not inside(emu_epilogue(acc_tiles(A, t["B"].float(), 64, 32), e)[0], ref, bound)
    B = torch.cat([t["B"][:N - 1], nb["B"][:1]]).float()
    assert not inside(emu_epilogue(acc_tiles(t["A"].float(), B, 64, 32), e)[0], ref, bound)


def test_res_bcast_mutant():
    """res row = (m / res_div) * res_mod + m % res_mod; the mutant takes m % res_div"""
    M, N, K, div, mod = 337, 72, 72, 150, 50
    t = gb.plain_inputs("res_bcast", M, N, K)
    m = torch.arange(M)
    rmap = t["res"][:(M + div - 1) // div * mod]
    acc = acc_tiles(t["A"].float(), t["B"].float(), 64, 32)
    e = dict(alpha=0.75, shift=t["shift"], res=rmap[(m // div) * mod + m % mod], act=gb.ACT_RELU, kernel="gemm_tiles")
    ref, bound = gb.plain_ref(t["A"], t["B"], e)["out"]
    assert inside(emu_epilogue(acc, e)[0], ref, bound)
    bad = dict(e, res=t["res"][(m // div) * mod + m % div])
    assert not inside(emu_epilogue(acc, bad)[0], ref, bound)


def test_a2_switch_one_column_block_late():
    M, N, K = 69, 264, 72
    t, t2 = gb.plain_inputs("a2", M, N, K), gb.plain_inputs("a2/second", M, N, K)
    e = dict(alpha=1.25, shift=t["shift"], res=t["res"], kernel="gemm_tiles")
    r1, r2 = gb.plain_ref(t["A"], t["B"], e)["out"], gb.plain_ref(t2["A"], t["B"], e)["out"]
    col = (torch.arange(N) >= 128).view(1, N)
    ref, bound = torch.where(col, r2[0], r1[0]), torch.where(col, r2[1], r1[1])
    o1 = emu_epilogue(acc_tiles(t["A"].float(), t["B"].float(), 64, 32), e)[0]
    o2 = emu_epilogue(acc_tiles(t2["A"].float(), t["B"].float(), 64, 32), e)[0]
    assert inside(torch.where(col, o2, o1), ref, bound)
    late = (torch.arange(N) >= 128 + 64).view(1, N)
    assert not inside(torch.where(late, o2, o1), ref, bound)


def test_grouped_launch_with_problem_zeros_rscale():
    M, N, K = 72, 128, 256
    ts = [gb.plain_inputs(f"group/p{i}", M, N, K) for i in range(3)]
    for i, t in enumerate(ts):
        e = dict(alpha=0.5, rscale=t["rscale"], out0=t["out0"], out_f32=1, kernel="gemm128w")
        ref, bound = gb.plain_ref(t["A"], t["B"], e)["out"]
        acc = acc_waves(t["A"].float(), t["B"].float())
        assert inside(emu_epilogue(acc, e)[0], ref, bound)
        if i:
            assert not inside(emu_epilogue(acc, dict(e, rscale=ts[0]["rscale"]))[0], ref, bound)


# ------------------------------------------------------------------------------------------------------------------ gathers
def emu_conv_fwd(x, w, stride, pad, dil, border_shift=False):
    """the forward gather tap by tap in f32: an out-of-plane tap is a zero row.
    one pixel to the right (the rest of the image is right).  border_shift: the left tap of the centre row, tap (R / 2, 0), where it lies ONE pixel outside
    the plane (ix = -1: the pixels of the left border) reads pixel 0 instead of a zero; every other pixel and tap is right."""
    Nb, H, W, C = x.shape
    Co, R, S_, _ = w.shape
    OH, OW = gb.out_hw(H, W, R, S_, stride, pad, dil)
    oy, ox = torch.meshgrid(torch.arange(OH), torch.arange(OW), indexing="ij")
    acc = torch.zeros(Nb, OH, OW, Co)
    xf, wf = x.float(), w.float()
    for r in range(R):
        for s in range(S_):
            iy, ix = oy * stride - pad + r * dil, ox * stride - pad + s * dil
            if border_shift and r == R // 2 and s == 0:
                ix = torch.where(ix == -1, ix + 1, ix)
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            tap = xf[:, iy.clamp(0, H - 1), ix.clamp(0, W - 1)] * ok.view(1, OH, OW, 1)
            acc = acc + tap @ wf[:, r, s].t()
    return acc.reshape(-1, Co)


@pytest.mark.parametrize("conv", gb.CONVS + [("stem", 2, 13, 17, 8, 64, 7, 2, 3, 1), ("halo", 1, 12, 47, 64, 72, 3, 1, 1, 1)], ids=lambda c: c[0])
def test_gather_emulations_and_the_border_tap_mutant(conv):
    name, Nb, H, W, C, Co, R, stride, pad, dil = conv
    t = gb.conv_inputs(name, Nb, H, W, C, Co, R, stride, pad, dil)
    geo = dict(stride=stride, pad=pad, dil=dil)
    e = dict(scale=t["scale"], shift=t["shift"], res=t["res"].reshape(-1, Co), act=gb.ACT_RELU, kernel="gemm_tiles")
    ref, bound = gb.conv_fwd_ref(t["x"], t["w"], e, **geo)["out"]
    assert inside(emu_epilogue(emu_conv_fwd(t["x"], t["w"], stride, pad, dil), e)[0], ref, bound)
    assert float((bound[ref != 0] / ref[ref != 0].abs()).median()) < 2.0 ** -7
    if pad:
        assert not inside(emu_epilogue(emu_conv_fwd(t["x"], t["w"], stride, pad, dil, border_shift=True), e)[0], ref, bound)
    # data gradient and weight gradient in f32 through autograd's kernels (another order of the same products)
    ed = dict(scale=t["dscale"], res=t["dres"].reshape(-1, C), aux=t["daux"].reshape(-1, C), act=gb.ACT_MASK_POS, kernel="gemm_tiles")
    dref, dbound = gb.conv_dgrad_ref(t["dy"], t["w"], (H, W), ed, **geo)["out"]
    xg = t["x"].float().permute(0, 3, 1, 2).requires_grad_(True)
    wg = t["w"].float().permute(0, 3, 1, 2).requires_grad_(True)
    F.conv2d(xg, wg, stride=stride, padding=pad, dilation=dil).backward(t["dy"].float().permute(0, 3, 1, 2))
    dx = xg.grad.permute(0, 2, 3, 1).reshape(-1, C)
    assert inside(emu_epilogue(dx, ed)[0], dref, dbound)
    ew = dict(rscale=t["rscale"], out0=t["out0"].reshape(Co, -1), out_f32=1, kernel="gemm_tiles")
    wref, wbound = gb.conv_wgrad_ref(t["dy"], t["x"], (Co, R, R, C), ew, **geo)["out"]
    dw = wg.grad.permute(0, 2, 3, 1).reshape(Co, -1)
    assert inside(emu_epilogue(dw, ew)[0], wref, wbound)
    if stride == 2 and R == 3:
        # the parity classes of ops._dgrad3x3_s2: class (py, px) owns the pixels (2 yy + py, 2 xx + px); the mutant writes class (1, 0)'s rows at class
        # (0, 1)'s pixels (and leaves its own at the residual)
        good = emu_epilogue(dx, ed)[0].view(Nb, H, W, C)
        bad = good.clone()
        src, dst = good[:, 1::2, 0::2], bad[:, 0::2, 1::2]
        h, w_ = min(src.shape[1], dst.shape[1]), min(src.shape[2], dst.shape[2])
        if h and w_:
            dst[:, :h, :w_] = src[:, :h, :w_]
            assert not inside(bad.reshape(-1, C), dref, dbound)
    if stride == 2 and R == 1:
        # the row scatter ((n * cH + oy * cst) * cW + ox * cst) with cH and cW swapped: 5 x 7 planes, so the rows land elsewhere
        OH, OW = t["OH"], t["OW"]
        rows = dx.view(Nb, H, W, C)[:, ::2, ::2].reshape(-1, C)                    # the rows the GEMM computes, in (n, oy, ox) order
        m = torch.arange(Nb * OH * OW)
        n_img, oy, ox = m // (OH * OW), m % (OH * OW) // OW, m % OW
        for swapped in (False, True):
            cH, cW = (W, H) if swapped else (H, W)
            crow = (n_img * cH + oy * 2) * cW + ox * 2
            full = torch.zeros(Nb * H * W, C)
            full[crow] = rows
            hit = torch.zeros(Nb * H * W, 1, dtype=torch.bool)
            hit[crow] = True
            out = torch.where(hit, emu_epilogue(full, ed)[0], torch.zeros(1))
            true_hit = torch.zeros(Nb, H, W, 1, dtype=torch.bool)
            true_hit[:, ::2, ::2] = True
            want = torch.where(true_hit.reshape(-1, 1), dref, torch.zeros(1, dtype=F64))
            assert inside(out, want, torch.where(true_hit.reshape(-1, 1), dbound, 0 * dbound)) != swapped


def test_stem_reference_against_its_f32_emulation():
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 13, 17, generator=g)
    w8 = F.pad(torch.randn(64, 7, 7, 3, generator=g) * (2.0 / 147) ** 0.5, (0, 5)).to(BF)
    shift = torch.randn(64, generator=g) * 0.3
    ref, bound = gb.stem_ref(img, w8, shift)
    y = F.conv2d(img.to(BF).float(), w8[..., :3].float().permute(0, 3, 1, 2), stride=2, padding=3) + shift.view(1, -1, 1, 1)
    got = F.max_pool2d(torch.relu(y), 3, 2, 1).permute(0, 2, 3, 1).to(BF)
    assert inside(got, ref, bound)
    assert float((bound[ref != 0] / ref[ref != 0].abs()).median()) < 2.0 ** -7
    shifted = F.max_pool2d(torch.relu(y), 3, 2, 0).permute(0, 2, 3, 1).to(BF)                  # the pool window one pixel off (no padding)
    h, w_ = shifted.shape[1], shifted.shape[2]
    assert not inside(shifted, ref[:, :h, :w_], bound[:, :h, :w_])
