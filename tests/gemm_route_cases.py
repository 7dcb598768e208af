"""Named toist_gemm descriptors for the routing tests (tests/test_cpu_gemm_route.py, tests/golden/make_golden_gemm_routes.py).

Deterministic: the same list, in the same order, on every call.  The addresses are made up (16-byte aligned unless a case says otherwise),
so these descriptors are only ever handed to the host-side routing code, never to a launch on a machine that has a GPU.  The grids put cases
on both sides of every numeric threshold of csrc/gemm_route.cpp."""
import ctypes
import hashlib
import itertools

from toist_amd import _lib
from toist_amd._lib import Gemm

A_ROWK, A_KROW, A_CONV, A_CONVT = _lib.A_ROWK, _lib.A_KROW, _lib.A_CONV, _lib.A_CONVT
B_ROWK, B_KROW, B_CONVX = _lib.B_ROWK, _lib.B_KROW, _lib.B_CONVX
ACT_NONE, ACT_RELU, ACT_GELU, ACT_MASK_POS = _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_GELU, _lib.ACT_MASK_POS
DEFER, SPLIT_EPI, COLSUM_SLICES = (_lib.CONSTANTS["TOIST_GEMM_" + n] for n in ("DEFER_REDUCE", "SPLIT_EPILOGUE", "COLSUM_SLICES"))

# made-up addresses, one 16 MiB lane per pointer field
PA, PB, PC, PRES, PAUX, PSCALE, PSHIFT, PWS, PCOLSUM, PGROUP, PA2, PRSCALE, PPRE = (0x10000000 + i * 0x1000000 for i in range(13))


def _up8(n):
    return (n + 7) & ~7


def base(M, N, K, a_kind, b_kind, f32=False):
    d = Gemm()
    d.M, d.N, d.K, d.a_kind, d.b_kind = M, N, K, a_kind, b_kind
    d.a.ptr, d.b.ptr, d.c = PA, PB, PC
    d.a.ld = _up8(M) if a_kind == A_KROW else _up8(K)
    d.b.ld = _up8(N) if b_kind == B_KROW else _up8(K)
    d.ldc = _up8(N)
    d.batch = d.batch_inner = d.split_k = 1
    d.epi.alpha = 1.0
    d.epi.out_f32 = 1 if f32 else 0
    return d


def geom(o, SH, SW, SC, PH, PW, R, stride, pad=None, dil=1):
    o.SH, o.SW, o.SC, o.PH, o.PW, o.R, o.S, o.stride, o.dil = SH, SW, SC, PH, PW, R, R, stride, dil
    o.pad = R // 2 if pad is None else pad
    o.ld = 0


def epilogue(d, act=ACT_NONE, res=False, scale=False):
    d.epi.act = act
    if act >= ACT_MASK_POS:
        d.epi.aux, d.epi.ldaux = PAUX, d.ldc
    if res:
        d.epi.res, d.epi.ldr = PRES, d.ldc
    if scale:
        d.epi.scale, d.epi.shift = PSCALE, PSHIFT
    return d


def linear(M, N, K, b_kind=B_ROWK, act=ACT_NONE, res=False, f32=False, tile=0):
    d = epilogue(base(M, N, K, A_ROWK, b_kind, f32), act, res)
    d.tile = tile
    return d


def conv_fwd(n, SH, SW, SC, Co, R, stride, act=ACT_RELU, res=False, tile=0):
    PH, PW = (SH - 1) // stride + 1, (SW - 1) // stride + 1
    d = epilogue(base(n * PH * PW, Co, R * R * SC, A_CONV, B_ROWK), act, res, scale=True)
    geom(d.a, SH, SW, SC, PH, PW, R, stride)
    d.tile = tile
    return d


def conv_dgrad(n, H, W, Co, Ci, act=ACT_MASK_POS, tile=0):
    """3x3 stride-1 data gradient: transposed gather of dy [n, H, W, Co], two-level k-major weights [tap][Co][Ci]"""
    d = epilogue(base(n * H * W, Ci, 9 * Co, A_CONVT, B_KROW), act)
    geom(d.a, H, W, Co, H, W, 3, 1)
    d.b.kin, d.b.tap_stride = Co, Co * d.b.ld
    d.tile = tile
    return d


def wgrad(M, N, K, split_k=1, tile=0, group=0, colsum=0, convx=None):
    """dW [M = Co][N] = dy^T x: k-major A, f32 output.  group = problems of a grouped launch; colsum: 1 = a_colsum, 2 = per-slice rows;
    convx = (SH, SW, SC, R, stride): B gathered from the layer's input (N = R * R * SC, K = n * PH * PW)."""
    d = base(M, N, K, A_KROW, B_CONVX if convx else B_KROW, f32=True)
    d.ldc = N
    if convx:
        SH, SW, SC, R, stride = convx
        geom(d.b, SH, SW, SC, (SH - 1) // stride + 1, (SW - 1) // stride + 1, R, stride)
    d.split_k, d.tile = split_k, tile
    if split_k > 1:
        d.workspace = PWS
    if group:
        d.group, d.batch = PGROUP, group
        if split_k > 1:
            d.flags |= DEFER
    if colsum:
        d.a_colsum = PCOLSUM
        if colsum == 2:
            d.flags |= COLSUM_SLICES
    return d


def _linear_grid():
    Ms = (32, 33, 500, 4095, 4096, 8128, 8192, 12160, 12288, 16256, 16384, 17000, 19072, 19200, 20416, 20480, 49152)
    Ns = (32, 40, 64, 127, 128, 256, 512, 1024)
    Ks = (64, 72, 256, 264, 512, 576, 704, 768, 1024)
    for M, N, K, bk, act, res, f32 in itertools.product(Ms, Ns, Ks, (B_ROWK, B_KROW), (ACT_NONE, ACT_RELU, ACT_GELU), (False, True), (False, True)):
        yield f"linear/{M}x{N}x{K}/b{bk}/act{act}/res{int(res)}/f32{int(f32)}", linear(M, N, K, bk, act, res, f32)


def _conv_grid():
    for n, (SH, SW), SC, Co, R, stride, res, tile in itertools.product((1, 8), ((25, 34), (50, 67), (100, 134)), (64, 128, 256), (64, 128, 256, 512),
                                                                       (1, 3), (1, 2), (False, True), (0, 131, 136)):
        yield f"conv/n{n}/{SH}x{SW}x{SC}/co{Co}/r{R}s{stride}/res{int(res)}/t{tile}", conv_fwd(n, SH, SW, SC, Co, R, stride, res=res, tile=tile)
    # gathers at exactly 95 / 96 tiles of 128x128 (M = 12160 / 12288): gemm128_pays' threshold for them
    for (n, H, W), Co, R, tile in itertools.product(((8, 40, 38), (8, 48, 32)), (128, 256), (1, 3), (0, 131, 136)):
        yield f"conv96/n{n}/{H}x{W}/co{Co}/r{R}/t{tile}", conv_fwd(n, H, W, 128, Co, R, 1, tile=tile)
    # 3x3 data gradient on both sides of M >= 2048 (the halo kernel), of 96 tiles of 128x128 and of N % 128 (gemm128)
    for (n, H, W), Co, Ci, act, tile in itertools.product(((1, 60, 34), (1, 64, 32), (2, 25, 34), (3, 25, 34), (7, 50, 34), (8, 40, 38), (8, 48, 32), (8, 50, 34), (8, 50, 67)), (64, 128, 256),
                                                          (64, 128, 192, 256), (ACT_NONE, ACT_MASK_POS), (0, 65, 131, 136)):
        yield f"dgrad/n{n}/{H}x{W}/co{Co}/ci{Ci}/act{act}/t{tile}", conv_dgrad(n, H, W, Co, Ci, act, tile)


def _wgrad_grid():
    shapes = ((64, 64), (72, 128), (256, 256), (512, 512), (1024, 1024), (256, 1024), (2048, 512))
    variants = ((0, 0), (0, 1), (0, 2), (23, 0), (3, 0))      # (group, colsum)
    for (M, N), K, split, tile, (group, colsum) in itertools.product(shapes, (256, 1000, 1024, 2048, 13600), (1, 2, 4, 8, 16, 37),
                                                                     (0, 65, 129, 130, 134, 137, 138), variants):
        if colsum == 2 and split == 1:
            continue        # refused by the precondition: one explicit case below
        yield f"wgrad/{M}x{N}x{K}/s{split}/t{tile}/g{group}/cs{colsum}", wgrad(M, N, K, split, tile, group, colsum)
    # conv weight gradients: B gathered from the input plane (K = pixels)
    for (n, SH, SW), SC, R, stride, Co, split, tile in itertools.product(((8, 50, 34), (8, 25, 32), (2, 16, 16)), (64, 128, 256), (1, 3), (1, 2), (128, 256),
                                                                         (1, 4, 16), (0, 130, 137, 138)):
        K = n * ((SH - 1) // stride + 1) * ((SW - 1) // stride + 1)
        yield f"wgradx/n{n}/{SH}x{SW}x{SC}/r{R}s{stride}/co{Co}/s{split}/t{tile}", wgrad(Co, R * R * SC, K, split, tile, convx=(SH, SW, SC, R, stride))


def _forced_and_misaligned():
    bases = {
        "small": lambda: linear(500, 64, 64),
        "panel": lambda: linear(8192, 64, 256, act=ACT_RELU, res=True),
        "panelk": lambda: linear(8192, 64, 256, b_kind=B_KROW, act=ACT_MASK_POS),
        "deep": lambda: linear(19200, 128, 1024, act=ACT_RELU, res=True),
        "gelu": lambda: linear(19200, 128, 1024, act=ACT_GELU),
        "narrow_n": lambda: linear(4096, 32, 256),
        "narrow_m": lambda: linear(32, 128, 256),
        "conv3": lambda: conv_fwd(8, 50, 34, 128, 128, 3, 1),
        "dgrad3": lambda: conv_dgrad(3, 25, 34, 128, 128),
        "wgrad": lambda: wgrad(1024, 1024, 2048, split_k=4),
    }
    codes = (64, 65, 128, 129, 130, 131, 132, 133, 134, 135, 136, 137, 138, 200, 3 << 8, 65 | 3 << 8, 129 | 2 << 8, 131 | 2 << 8, 136 | 2 << 8,
             135 | 1 << 8, 135 | 2 << 8, 135 | 3 << 8, 135 | 18 << 8, 135 | 255 << 8)
    for (name, make), code in itertools.product(bases.items(), codes):
        d = make()
        d.tile = code
        yield f"forced/{name}/t{code & 255}v{code >> 8}", d
    # 8 bytes off, field by field, and the validation fallback (flags bit 0): each takes the lean / panel / 128x128 paths away
    for name in ("panel", "panelk", "deep", "conv3", "dgrad3"):
        for field in ("c", "res", "aux", "scale", "shift", "flags"):
            for tile in (0, 135, 136):
                d = bases[name]()
                d.tile = tile
                if field == "flags":
                    d.flags |= 1
                elif field == "c":
                    d.c += 8
                else:
                    if field == "res" and not d.epi.res:
                        d.epi.res, d.epi.ldr = PRES, d.ldc
                    if field == "aux" and not d.epi.aux:
                        d.epi.act, d.epi.aux, d.epi.ldaux = ACT_MASK_POS, PAUX, d.ldc
                    if field in ("scale", "shift") and not d.epi.scale:
                        d.epi.scale, d.epi.shift = PSCALE, PSHIFT
                    setattr(d.epi, field, getattr(d.epi, field) + 8)
                yield f"misaligned/{name}/{field}/t{tile}", d
    # huge planes: the 32-bit offset limits of the panel kernels
    # (K = 64: the C plane passes 2^30 elements -- the first-generation kernel's reach -- before the A plane does)
    for M, K in itertools.product((1 << 21, 1 << 22, 1 << 23), (64, 256)):
        yield f"huge/panel/{M}x{K}", linear(M, 256, K, act=ACT_RELU, res=True)
    # split-K with the complete epilogue, and the second A operand
    for M, N, K, split, tile in itertools.product((128, 500), (256, 1024), (1024, 3072), (2, 4, 8, 64), (0, 65, 130)):
        d = linear(M, N, K, act=ACT_GELU, res=True, tile=tile)
        d.split_k, d.workspace, d.flags = split, PWS, SPLIT_EPI
        yield f"splitepi/{M}x{N}x{K}/s{split}/t{tile}", d
    for M, N, K, tile in itertools.product((500, 19200), (768,), (256, 1024), (0, 65, 134, 135, 136)):
        d = linear(M, N, K, tile=tile)
        d.a2, d.a2_from = PA2, 512
        yield f"a2/{M}x{N}x{K}/t{tile}", d
    # batched launches (attention products), zero batch fields (normalised by the dispatcher)
    for batch, inner, tile in itertools.product((0, 1, 64), (0, 1, 8), (0, 65, 135, 136)):
        d = linear(19200, 128, 1024, tile=tile)
        d.batch, d.batch_inner, d.split_k = batch, inner, 0
        d.a.bs_outer = d.b.bs_outer = d.cs_outer = 1 << 20
        yield f"batched/b{batch}i{inner}/t{tile}", d
    for inner, split, tile in itertools.product((0, 1), (0, 1, 4), (0, 130, 137)):
        d = wgrad(1024, 1024, 2048, split_k=max(split, 1), tile=tile)
        d.batch_inner, d.split_k = inner, split
        yield f"wgrad0/i{inner}s{split}/t{tile}", d


def _refusals():
    """at least one descriptor for every refusal message of toist_gemm_bf16, in the order of its checks"""
    def edit(d, **kw):
        for k, v in kw.items():
            obj, _, leaf = k.rpartition("__")
            setattr(getattr(d, obj) if obj else d, leaf, v)
        return d
    lin = lambda: linear(500, 64, 256)       # noqa: E731
    yield "refuse/shape", edit(lin(), M=0)       # (K = 0: see unrecorded())
    yield "refuse/null", edit(lin(), c=None)
    yield "refuse/ab_align", edit(lin(), a__ptr=PA + 8)
    yield "refuse/batch_stride", edit(lin(), b__bs_outer=12)
    yield "refuse/src_channels", edit(conv_fwd(1, 25, 34, 64, 64, 3, 1), a__SC=60)
    yield "refuse/conv_geometry", edit(conv_fwd(1, 25, 34, 64, 64, 3, 1), a__stride=0, tile=65)
    yield "refuse/conv_geometry_136", edit(conv_fwd(8, 50, 34, 128, 128, 3, 1, tile=136), a__PH=0)       # (the predicates divide by PH * PW)
    yield "refuse/conv_geometry_0", edit(conv_fwd(8, 50, 34, 128, 128, 3, 1), a__SW=0)
    yield "refuse/convx_geometry_137", edit(wgrad(128, 1152, 13600, tile=137, convx=(50, 34, 128, 3, 1)), b__PW=0)
    yield "refuse/ld", edit(lin(), a__ld=252)
    yield "refuse/convx_n", edit(wgrad(128, 576, 1600, convx=(25, 34, 64, 3, 1)), N=572)
    yield "refuse/krow_lda", edit(wgrad(256, 256, 1024), a__ld=248)
    yield "refuse/krow_ldb", edit(wgrad(256, 256, 1024), b__ld=248)
    yield "refuse/split_f32", edit(linear(500, 64, 1024), split_k=2, workspace=PWS)
    yield "refuse/accumulate_f32", edit(lin(), epi__accumulate=1)
    yield "refuse/split_epilogue", edit(linear(128, 256, 1024), split_k=2, flags=SPLIT_EPI)
    yield "refuse/colsum_kind", edit(lin(), a_colsum=PCOLSUM)
    yield "refuse/colsum_slices", wgrad(256, 256, 1024, split_k=1, colsum=2)
    yield "refuse/group", edit(wgrad(256, 256, 1024, split_k=4, group=23), flags=0)
    yield "refuse/split_epilogue_kind", edit(wgrad(256, 256, 1024, split_k=4), epi__scale=PSCALE)
    yield "refuse/split_batch", edit(wgrad(256, 256, 1024, split_k=4), batch=2)
    yield "refuse/split_workspace", edit(wgrad(256, 256, 1024, split_k=4), workspace=None)
    yield "refuse/split_ldc", edit(wgrad(256, 256, 1024, split_k=4), ldc=258)
    yield "refuse/aux", edit(lin(), epi__act=ACT_MASK_POS)
    yield "refuse/a2", edit(lin(), a2=PA2, a2_from=100)
    yield "refuse/dropout", edit(lin(), epi__drop_where=1, epi__drop_p=1.5)
    yield "refuse/gemm128", edit(linear(19200, 128, 200), tile=136)
    yield "refuse/conv3", edit(conv_fwd(8, 50, 67, 128, 128, 3, 1), tile=131)
    yield "refuse/panel", edit(linear(8192, 64, 512), tile=135)
    yield "refuse/gemm128w", edit(wgrad(256, 256, 128), tile=137)
    yield "refuse/gemm256w", edit(wgrad(384, 256, 2048), tile=138)
    yield "refuse/colsum_clamp", wgrad(256, 256, 64, split_k=4, tile=65, colsum=2)
    yield "refuse/kin", edit(conv_dgrad(1, 25, 34, 64, 64, tile=65), b__kin=60)
    yield "refuse/tile_code", edit(lin(), tile=77)
    yield "refuse/operand_kinds", edit(wgrad(256, 256, 1024, tile=65), b_kind=B_ROWK, b__ld=1024)
    yield "refuse/operand_kinds_convt", edit(conv_dgrad(1, 25, 34, 64, 64, tile=65), b_kind=B_ROWK, b__ld=576, b__kin=0)


def cases():
    """[(name, Gemm)]: every case of every group above"""
    out = []
    for group in (_linear_grid, _conv_grid, _wgrad_grid, _forced_and_misaligned, _refusals):
        out.extend(group())
    names = [n for n, _ in out]
    assert len(set(names)) == len(names) and len(names) <= 100000
    return out


def unrecorded():
    """[(name, Gemm)] the golden table cannot hold: the library it was recorded from divided by zero on them (K <= 0 in its
    toist_gemm_effective_split).  Only the stand-alone program runs them: refused as a bad shape, and the queries answer one slice."""
    out = []
    for K, split, tile in itertools.product((0, -64), (0, 1, 4), (0, 65, 64, 137)):
        d = linear(500, 64, 256, tile=tile) if tile != 137 else wgrad(256, 256, 1024, tile=137)
        d.K, d.split_k = K, split
        out.append((f"unrecorded/k{K}/s{split}/t{tile}", d))
    return out


def digest(case_list):
    """changes when the generator does: over the names and the descriptors' bytes"""
    h = hashlib.sha256()
    for name, d in case_list:
        h.update(name.encode())
        h.update(bytes(d))
    return h.hexdigest()


def raw(case_list):
    """the descriptors as consecutive toist_gemm structs (tests/gemm_route_main.cpp reads this)"""
    return b"".join(bytes(d) for _, d in case_list)


assert ctypes.sizeof(Gemm) % 8 == 0
