"""Every kernel that draws a dropout mask, against masks formed on the HOST from the restated hashes (oracle/xdec_ref.py elem_keep, oracle/train_ref.py
softmax_keep / small_attn_keep) and fp64 math -- not against another kernel of ours.  What is pinned per kernel: WHICH elements are dropped (exactly:
no mismatch is allowed, so an element index built with the wrong pitch fails), the factor 1 / (1 - p), and where the mask sits in the epilogue
(drop_where = 1: before the residual, drop_where = 2: after the activation).

  kernels.dropout                     bit-exact: bf16(float32(x) * sc), sc = 1.f / (1.f - p) in float32, +0 where dropped
  GEMM epilogues through ops.linear   generic tiles (64 / 128 / 65 / 130 / 134 / auto), the short-K panel kernel, the lean and the general epilogue, split-K
                                      with the complete epilogue; the element index is (m * N + n) whatever the row pitch of the output.  gemm128_kernel
                                      carries NO dropout epilogue (gemm128_applies refuses drop_where): the explicit tile code must be refused loudly.
                                      Values at the bound of tests/test_gpu_gemm.py test_linear_fwd / test_linear_epilogues (_close, K-scaled)
  kernels.softmax_fwd / softmax_bwd   the per-op attention core: index row * round8(Sk) + k; tolerances of test_attention_products
  attn_small_fwd / attn_small_bwd     index ((b * H + h) * S + i) * S + j; tolerances of test_small_attention_against_autograd
  layernorm_bwd(dx_drop), rowgemm     ROW_LN_BWD out2 and ROW_LN_FWD z: index m * 256 + n; the masked copy within the bound tests/test_gpu_tlayer.py gives it

Element indices at or above 2^32 are not covered: the host hash handles lower indices only, and no tensor here comes near (all <= 1M elements)."""
import math

import pytest
import torch

from oracle import train_ref as tr
from oracle import xdec_ref as xr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def kern():
    """kernels.SEED_DEV is process-wide: None for this module (a test that wants a word sets it itself), restored afterwards"""
    from toist_amd import kernels as k
    seed_dev = k.SEED_DEV
    k.SEED_DEV = None
    yield k
    k.SEED_DEV = seed_dev


def _bits(t):
    return t.contiguous().view(torch.int16)


def _seed_word(k, dev, word):
    k.SEED_DEV = None if word is None else torch.full((1,), word, dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------------------------ a. toist_dropout_bf16
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("shape", [(1, 8), (37, 256), (130, 768)])
def test_dropout_kernel_bit_exact(dev, kern, shape, p):
    k = kern
    g = torch.Generator().manual_seed(shape[0] * 1000 + int(p * 100))
    x = (torch.randn(*shape, generator=g) * 3).to(BF)
    sc = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    scaled = (x.float() * sc).to(BF)
    xd = x.to(dev)
    # the last pair: a device seed word whose sum with the host seed crosses 2^32 (the kernels add the two as 64-bit integers)
    for seed, word in ((7, None), (0x123456789ABC, None), (0x7FFFFFFFFFFF, None), (0xFFFFFFF0, 0x123)):
        out = torch.full(shape, float("nan"), dtype=BF, device=dev)
        _seed_word(k, dev, word)
        try:
            k.dropout(xd, p, seed, out)
        finally:
            _seed_word(k, dev, None)
        keep = xr.elem_keep(shape[0], shape[1], p, seed + (word or 0))
        want = torch.where(keep, scaled, torch.zeros((), dtype=BF))
        assert torch.equal(_bits(out.cpu()), _bits(want)), (seed, word, int((_bits(out.cpu()) != _bits(want)).sum()))


# ------------------------------------------------------------------------------------------------------------------ b. GEMM epilogues
def _act64(k, act, t):
    if act == k.ACT_RELU:
        return torch.relu(t)
    if act == k.ACT_GELU:
        return torch.nn.functional.gelu(t)
    return t


# (M, N, K, tile, split_k, out_dtype, wide): tile codes as in tests/test_gpu_gemm.py (64 / 128: k-tiles of 32; 65 / 130 / 134: the lean epilogue for a bf16
# output, the general one for f32; 135: the short-K panel kernel; 0: the dispatcher's choice); wide: output and residual are column slices of wider tensors
_GEMM_CASES = {
    "tile64": (200, 72, 96, 64, 1, BF, False),
    "tile128": (333, 256, 256, 128, 1, BF, False),
    "auto": (300, 264, 128, 0, 1, BF, False),
    "lean65": (333, 256, 256, 65, 1, BF, False),
    "lean130": (333, 256, 256, 130, 1, BF, False),
    "lean134": (300, 264, 128, 134, 1, BF, False),
    "general65_f32": (200, 72, 96, 65, 1, torch.float32, False),
    "panel_a": (800, 512, 128, 135, 1, BF, False),
    "panel_b": (1000, 264, 72, 135, 1, BF, False),
    "split3": (100, 256, 2048, 0, 3, BF, False),
    "lean65_wide": (333, 256, 256, 65, 1, BF, True),
    "general65_f32_wide": (200, 72, 96, 65, 1, torch.float32, True),
    "split3_wide": (100, 256, 2048, 0, 3, BF, True),
}


_GEMM_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_gemm_cases():
    """the cases' device tensors live as long as this module's tests, not as long as the process"""
    yield
    _GEMM_CACHE.clear()


def _gemm_case(name, dev):
    """operands and the fp64 product x w^T + b of one case, formed once and shared by its epilogue variants"""
    if name in _GEMM_CACHE:
        return _GEMM_CACHE[name]
    M, N, K, tile, split_k, odt, wide = _GEMM_CASES[name]
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g).to(BF), (torch.randn(N, K, generator=g) * 0.1).to(BF)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g).to(BF)
    c = dict(name=name, M=M, N=N, K=K, tile=tile, split_k=split_k, odt=odt, wide=wide, res=res, y=x.double() @ w.double().t() + bias.double(),
             xd=x.to(dev), wd=w.to(dev), bd=bias.to(dev))
    if wide:            # row pitch N + 16, the slice starts 8 elements into the row: the mask index must follow N, not the pitch
        c["res_wide"] = torch.zeros(M, N + 16, dtype=BF, device=dev)
        c["res_wide"][:, 8:8 + N] = res.to(dev)
        c["resd"] = c["res_wide"][:, 8:8 + N]
    else:
        c["resd"] = res.to(dev)
    _GEMM_CACHE[name] = c
    return c


# every case with both mask positions, without and with ReLU; GELU with drop_where = 1 on the generic tiles, through the lean and the general epilogue
_GEMM_VARIANTS = [(n, dw, act) for n in _GEMM_CASES for dw in (1, 2) for act in ("none", "relu")] + [(n, 1, "gelu") for n in ("tile64", "lean65", "general65_f32")]


@pytest.mark.parametrize("name,drop_where,act", _GEMM_VARIANTS)
def test_gemm_epilogue_dropout(dev, kern, name, drop_where, act):
    from test_gpu_gemm import _close
    from toist_amd import ops
    k, c = kern, _gemm_case(name, dev)
    M, N, K, p, seed = c["M"], c["N"], c["K"], 0.1, 0x1234567 + drop_where
    act_code = {"none": k.ACT_NONE, "relu": k.ACT_RELU, "gelu": k.ACT_GELU}[act]
    wide_out = None
    if c["wide"]:
        wide_out = torch.full((M, N + 16), float("nan"), dtype=c["odt"], device=dev)
        out = ops.linear(c["xd"], c["wd"], c["bd"], out=wide_out[:, 8:8 + N], res=c["resd"], act=act_code, drop_where=drop_where, drop_p=p, drop_seed=seed,
                         tile=c["tile"], split_k=c["split_k"])
    else:
        out = ops.linear(c["xd"], c["wd"], c["bd"], out_dtype=c["odt"], res=c["resd"], act=act_code, drop_where=drop_where, drop_p=p, drop_seed=seed,
                         tile=c["tile"], split_k=c["split_k"])
    out = out.cpu()
    keep = xr.elem_keep(M, N, p, seed)
    sc = 1.0 / (1.0 - p)
    res64 = c["res"].double()
    if drop_where == 1:
        ref = _act64(k, act_code, torch.where(keep, c["y"] * sc, torch.zeros((), dtype=F64)) + res64)
        if_dropped = _act64(k, act_code, res64)
    else:
        ref = torch.where(keep, _act64(k, act_code, c["y"] + res64) * sc, torch.zeros((), dtype=F64))
        if_dropped = torch.zeros_like(ref)
    atol = 4e-3 * math.sqrt(K)                      # _close's absolute term
    # 1. mask positions, exact
    if act != "gelu":                               # what a dropped element holds is exact in bf16: 0, the residual, relu(residual)
        alt = if_dropped.to(out.dtype)
        wrong = (out != alt) & ~keep
        assert not bool(wrong.any()), f"{c['name']}: {int(wrong.sum())} dropped elements do not hold the dropped value, first at {wrong.nonzero()[0].tolist()}"
        if act == "none" and out.dtype == BF and drop_where == 1:
            assert torch.equal(_bits(out)[~keep], _bits(c["res"])[~keep])          # the bf16 residual bit for bit
        if drop_where == 2:
            assert float(out[~keep].abs().max()) == 0.0
        missing = (out == alt) & keep & ((ref - if_dropped).abs() > atol)
        assert not bool(missing.any()), f"{c['name']}: {int(missing.sum())} kept elements hold the dropped value, first at {missing.nonzero()[0].tolist()}"
    else:                                           # a dropped element holds gelu(residual), formed in f32 and stored as bf16 (or f32): one bf16 ulp (2^-7
        # relative at most; 1e-5 for the vanishing left tail, where 1 + erf cancels in f32) around the fp64 value pins the positions on this path too
        tol = 2.0 ** -7 * if_dropped.abs() + 1e-5
        wrong = ((out.double() - if_dropped).abs() > tol) & ~keep
        assert not bool(wrong.any()), f"{c['name']}: {int(wrong.sum())} dropped elements are not gelu(residual), first at {wrong.nonzero()[0].tolist()}"
        # a kept element farther from gelu(residual) than twice the value bound below (+ tol) cannot sit within tol of it unless it misses that bound
        far = keep & ((ref - if_dropped).abs() > 2 * (atol + 1.5e-2 * ref.abs()) + tol)
        assert float(far.double().mean()) > 0.5
        missing = far & ((out.double() - if_dropped).abs() <= tol)
        assert not bool(missing.any()), f"{c['name']}: {int(missing.sum())} kept elements hold gelu(residual), first at {missing.nonzero()[0].tolist()}"
    assert 0.07 < 1.0 - float(keep.double().mean()) < 0.13
    # 2. values: bias, mask, 1 / (1 - p), residual and activation in the stated order
    _close(out, ref, K, f"{c['name']} drop_where={drop_where} act={act}")
    if wide_out is not None:                         # nothing outside the slice is written
        assert bool(torch.isnan(wide_out[:, :8]).all()) and bool(torch.isnan(wide_out[:, 8 + N:]).all())


def test_gemm128_kernel_refuses_a_dropout_epilogue(dev, kern):
    """csrc/gemm.hip gemm128_kernel (tile code 136) has no dropout in its epilogue and gemm128_applies says so: asked for by its tile code with drop_where set,
    the library must refuse -- not run the kernel without the mask, not hand the call to another kernel -- and the same call without dropout must run"""
    from toist_amd import ops
    k = kern
    g = torch.Generator().manual_seed(136)
    M, N, K = 300, 264, 320
    x, w = torch.randn(M, K, generator=g).to(BF).to(dev), (torch.randn(N, K, generator=g) * 0.1).to(BF).to(dev)
    bias, res = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(BF).to(dev)
    ops.linear(x, w, bias, res=res, act=k.ACT_RELU, tile=136, split_k=1)
    for dw in (1, 2):
        with pytest.raises(RuntimeError, match="128x128"):
            ops.linear(x, w, bias, res=res, act=k.ACT_RELU, drop_where=dw, drop_p=0.1, drop_seed=5, tile=136, split_k=1)


# ------------------------------------------------------------------------------------------------------------------ c. toist_softmax_fwd / bwd
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("B,H,Sq,Sk", [(2, 2, 33, 52), (1, 4, 100, 17)])
def test_softmax_dropout_forward_and_backward(dev, kern, B, H, Sq, Sk, p):
    from test_gpu_gemm import _close
    from toist_amd import ops
    k = kern
    g = torch.Generator().manual_seed(Sq * Sk + int(p * 100))
    ld = ops.round8(Sk)
    rows, seed = B * H * Sq, 0x2468ACE13579
    s = (torch.randn(rows, ld, generator=g) * 2).to(BF)
    s[:, Sk:] = 1e4                                   # the pad columns of a score row hold anything
    key_pad = torch.zeros(B, Sk, dtype=torch.uint8)
    key_pad[B - 1, Sk - 5:] = 1
    key_pad[0, 3] = 1
    dead = key_pad.bool().view(B, 1, 1, Sk).expand(B, H, Sq, Sk).reshape(rows, Sk)
    prob = torch.full((B * H, Sq, ld), float("nan"), dtype=BF, device=dev)
    pdrop = torch.full((B * H, Sq, ld), float("nan"), dtype=BF, device=dev)
    k.softmax_fwd(s.view(B * H, Sq, ld).to(dev), key_pad.to(dev), B, H, Sq, Sk, ld, prob, pdrop, p, seed)
    keep = tr.softmax_keep(rows, Sk, p, seed)
    sc = 1.0 / (1.0 - p)
    P = torch.softmax(s[:, :Sk].double().masked_fill(dead, float("-inf")), -1)
    pc, pd = prob.cpu().view(rows, ld), pdrop.cpu().view(rows, ld)
    assert float(pc[:, Sk:].abs().max()) == 0.0 and float(pd[:, Sk:].abs().max()) == 0.0          # columns past Sk stay 0
    assert float(pd[:, :Sk][~keep].abs().max()) == 0.0                                              # exactly 0 where dropped
    live = keep & ~dead & (P > 2e-3)
    assert bool((pd[:, :Sk][live] != 0).all())
    _close(pc[:, :Sk], P, 1, "softmax", rtol=1e-2, atol_unit=2e-3)
    _close(pd[:, :Sk], P * keep * sc, 1, "dropped-out softmax", rtol=1e-2, atol_unit=2e-3)
    # backward: ds = P (m dp - sum_j P_j m_j dp_j), m = keep / (1 - p), from the probabilities the forward stored
    dp = (torch.randn(rows, ld, generator=g) * 3).to(BF)
    ds = torch.full((B * H, Sq, ld), float("nan"), dtype=BF, device=dev)
    k.softmax_bwd(prob, dp.view(B * H, Sq, ld).to(dev), rows, Sk, ld, ds, p, seed)
    Pb = pc[:, :Sk].double()
    gm = dp[:, :Sk].double() * keep * sc
    ref = Pb * (gm - (Pb * gm).sum(-1, keepdim=True))
    dsc = ds.cpu().view(rows, ld)
    assert float(dsc[:, Sk:].abs().max()) == 0.0
    assert float(dsc[:, :Sk][dead].abs().max()) == 0.0                                              # padded keys: exactly no gradient
    _close(dsc[:, :Sk], ref, 1, "softmax backward", rtol=3e-2, atol_unit=6e-3)
    # ... and as a whole: the reference is formed from the probabilities the kernel itself reads, so what separates the two is the bf16 rounding of ds
    # (half an ulp: at most 2^-8 of every element, hence of the norm) and f32 arithmetic (1e-4 is generous); a mask shifted by one row pitch gives ~1
    assert xr.relF(dsc[:, :Sk].double(), ref) < 2.0 ** -8 + 1e-4


# ------------------------------------------------------------------------------------------------------------------ d. csrc/attn_small.hip
def _small_attention(dev, k, B, H, S, dh, p, word):
    """the shapes, inputs and tolerances of tests/test_gpu_gemm.py test_small_attention_against_autograd with the dropout mask on: softmax -> keep / (1 - p)
    -> @ v in fp64 autograd, the mask from the host hash; word: the device seed word, added to the host seed"""
    from test_gpu_gemm import _close
    g = torch.Generator().manual_seed(S * dh)
    d = H * dh
    seed = 0x1F2E3D4C5B
    qkv = torch.randn(B * S, 3 * d, generator=g).to(BF)
    bias = [torch.randn(d, generator=g) * 0.3 for _ in range(3)]
    pad = torch.zeros(B, S, dtype=torch.uint8)
    for b in range(B):
        pad[b, S - (b % 3):] = 1 if b % 3 else 0
    dctx = torch.randn(B * S, d, generator=g).to(BF)
    scale = dh ** -0.5
    keep = tr.small_attn_keep(B, H, S, p, seed + (word or 0))
    leaves = [(qkv[:, i * d:(i + 1) * d].double() + bias[i].double()).view(B, S, H, dh).transpose(1, 2).requires_grad_(True) for i in range(3)]
    sc = ((leaves[0] @ leaves[1].transpose(-1, -2)) * scale).masked_fill(pad.bool()[:, None, None, :], float("-inf"))
    ctx_ref = ((sc.softmax(-1) * keep / (1.0 - p)) @ leaves[2]).transpose(1, 2).reshape(B * S, d)
    ctx_ref.backward(dctx.double())
    ref_grads = [t.grad.transpose(1, 2).reshape(B * S, d) for t in leaves]
    qkv_d = qkv.to(dev)
    q, kk, v = (qkv_d[:, i * d:(i + 1) * d] for i in range(3))
    bd = [t.to(dev) for t in bias]
    ctx = torch.full((B * S, d), float("nan"), dtype=BF, device=dev)
    stats = torch.empty(B * H * S * 2, dtype=torch.float32, device=dev)
    dqkv = torch.full((B * S, 3 * d), float("nan"), dtype=BF, device=dev)
    dq, dk, dv = (dqkv[:, i * d:(i + 1) * d] for i in range(3))
    _seed_word(k, dev, word)
    try:
        k.attn_small_fwd(q, kk, v, pad.to(dev), B, H, S, dh, scale, p, seed, ctx, stats, *bd)
        k.attn_small_bwd(q, kk, v, pad.to(dev), B, H, S, dh, scale, p, seed, stats, dctx.to(dev), dq, dk, dv, *bd)
    finally:
        _seed_word(k, dev, None)
    _close(ctx, ctx_ref.detach(), S, "small attention forward", rtol=2e-2, atol_unit=3e-3)
    for name, got, ref in zip("qkv", (dq, dk, dv), ref_grads):
        _close(got, ref, S * 4, f"small attention d{name}", rtol=3e-2, atol_unit=3e-3)


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("B,H,S,dh", [(8, 12, 16, 64), (3, 4, 11, 32), (2, 2, 40, 64), (1, 3, 64, 16)])
def test_small_attention_dropout_against_autograd(dev, kern, B, H, S, dh, p):
    _small_attention(dev, kern, B, H, S, dh, p, None)


def test_small_attention_dropout_with_a_device_seed_word(dev, kern):
    """host seed + device word cross 2^32: the reference of the sum must be the output's"""
    _small_attention(dev, kern, 3, 4, 11, 32, 0.1, 0xFFFFFF00)


# ------------------------------------------------------------------------------------------------------------------ e. row kernels
def _masked_copy_checks(got, dx, keep, p, what):
    """got: the dropout-masked copy of the gradient dx (both bf16 [M, 256]): exactly 0 where dropped; elsewhere bf16(dx * sc) to one bf16 ulp (the kernels mask
    the unrounded value) -- the bound tests/test_gpu_tlayer.py holds the same copy to"""
    from test_gpu_tlayer import _close
    got, dx = got.cpu(), dx.cpu()
    assert float(got[~keep].abs().max()) == 0.0, what
    assert bool((got[keep & (dx != 0)] != 0).all()), what
    want = torch.where(keep, dx.float() * (1.0 / (1.0 - p)), torch.zeros(()))
    _close(got, want, what, rtol=8e-3, atol=1e-5)


@pytest.mark.parametrize("rows", [37, 53, 800])
def test_layernorm_bwd_masked_copy(dev, kern, rows):
    k = kern
    g = torch.Generator().manual_seed(rows)
    D, p, seed = 256, 0.1, 0x7654321FEDC
    x = (torch.randn(rows, D, generator=g) * 2 + 0.3).to(BF).to(dev)
    gamma, beta = (torch.rand(D, generator=g) + 0.5).to(dev), torch.zeros(D, device=dev)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    k.layernorm_fwd(x, gamma, beta, 1e-5, y, mean, rstd)
    dy = torch.randn(rows, D, generator=g).to(BF).to(dev)
    dx = torch.full((rows, D), float("nan"), dtype=BF, device=dev)
    dxd = torch.full((rows, D), float("nan"), dtype=BF, device=dev)
    k.layernorm_bwd(dy, x, mean, rstd, gamma, dx, None, None, dx_drop=dxd, drop_p=p, seed=seed)
    _masked_copy_checks(dxd, dx, xr.elem_keep(rows, D, p, seed), p, "layernorm_bwd dx_drop")


@pytest.mark.parametrize("M,K,parts", [(53, 768, 3), (800, 256, 4)])
def test_rowgemm_ln_bwd_masked_copy(dev, kern, M, K, parts):
    k = kern
    g = torch.Generator().manual_seed(M + K + parts)
    p, seed = 0.1, 0x13579BDF02468
    w = (torch.randn(K, 256, generator=g) / math.sqrt(K)).to(BF)
    res, res2 = torch.randn(M, 256, generator=g).to(BF), torch.randn(M, 256, generator=g).to(BF)
    z = (torch.randn(M, 256, generator=g) * 2 + 0.3).to(BF)
    gamma = torch.rand(256, generator=g) + 0.5
    mu = z.float().mean(1)
    rs = (((z.float() - mu[:, None]) ** 2).mean(1) + 1e-5).rsqrt()
    a = torch.randn(M, K, generator=g).to(BF)
    fold = (torch.randn(parts, M, 256, generator=g) * 0.5).to(BF)
    dz = torch.full((M, 256), float("nan"), dtype=BF, device=dev)
    dzd = torch.full((M, 256), float("nan"), dtype=BF, device=dev)
    k.rowgemm(a.to(dev), w.to(dev), dz, b_kind=k.B_KROW, epi=k.ROW_LN_BWD, res=res.to(dev), res2=res2.to(dev), gamma=gamma.to(dev), z=z.to(dev), mean=mu.to(dev),
              rstd=rs.to(dev), out2=dzd, drop_p=p, drop_seed=seed, fold=fold.to(dev), fold_cols=256)
    _masked_copy_checks(dzd, dz, xr.elem_keep(M, 256, p, seed), p, "rowgemm ROW_LN_BWD out2")


@pytest.mark.parametrize("M,K", [(37, 768), (800, 256)])
def test_rowgemm_ln_fwd_dropped_rows_hold_the_residual(dev, kern, M, K):
    from test_gpu_tlayer import _close
    k = kern
    g = torch.Generator().manual_seed(M + K)
    p, seed = 0.1, 0xABCDEF012345
    a = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(256, K, generator=g) / math.sqrt(K)).to(BF)
    bias = torch.randn(256, generator=g) * 0.1
    res = torch.randn(M, 256, generator=g).to(BF)
    gamma, beta = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.1
    z = torch.full((M, 256), float("nan"), dtype=BF, device=dev)
    y = torch.empty(M, 256, dtype=BF, device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    k.rowgemm(a.to(dev), w.to(dev), y, b_kind=k.B_ROWK, epi=k.ROW_LN_FWD, bias=bias.to(dev), res=res.to(dev), gamma=gamma.to(dev), beta=beta.to(dev), eps=1e-5,
              z=z, mean=mean, rstd=rstd, drop_p=p, drop_seed=seed)
    keep = xr.elem_keep(M, 256, p, seed)
    zc = z.cpu()
    assert torch.equal(_bits(zc)[~keep], _bits(res)[~keep])                  # the residual exactly where the branch is dropped
    t = a.double() @ w.double().t() + bias.double()
    moved = keep & (t.abs() > 0.05)                                         # 0.05 / 0.9 is above half a bf16 ulp of any |residual| < 8
    assert bool((zc[moved] != res[moved]).all())
    _close(zc, torch.where(keep, t / (1.0 - p), torch.zeros((), dtype=F64)) + res.double(), "z", rtol=4e-3, atol=1e-3)      # test_rowgemm_layernorm_forward's bound on z
