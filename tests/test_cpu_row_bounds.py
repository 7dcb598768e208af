"""The bounds of tests/row_bounds.py are neither wrong nor vacuous: for every reference there, a torch f32 EMULATION of the kernel's arithmetic
(per-lane partial sums in the kernel's order, folded as wave_sum folds them, the block's LDS fold, round-to-nearest-even stores) stays within
`bound` on every case of the grids the GPU tests run (tests/test_gpu_row_kernels.py, tests/test_gpu_elem.py), and mutants of the emulation --
the ways such kernels go wrong -- exceed it on at least one case of those same grids, which the assertion names.  The references read
rounding_bounds.ACC_WIDEN when called, so an entry there is in force for the mutants too."""
import functools

import pytest
import torch

import rounding_bounds as rb
import row_bounds as rw
from oracle import xdec_ref as xr
from rounding_bounds import BF, F32

F = torch.nn.functional
LANES = torch.arange(64)


def trunc_bf16(v):
    """f32 -> bf16 by dropping the low 16 bits (the mutant store)"""
    return (v.to(F32).contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def wave_fold(v):
    """wave_sum: the xor butterfly over the 64 lanes [..., 64] -> [...] (every lane ends with the same value)"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANES ^ o]
    return v[..., 0]


def lane_sum8(t):
    """sum of each row of t [rows, L] (L % 8 == 0) as the LayerNorm / softmax kernels form it: lane l holds the 8-element chunks l, l + 64, ...,
    adds them element by element, then wave_sum"""
    rows, L = t.shape
    nI = (L // 8 + 63) // 64
    t = F.pad(t, (0, nI * 512 - L)).view(rows, nI, 64, 8)
    s = torch.zeros(rows, 64)
    for i in range(nI):
        for j in range(8):
            s = s + t[:, i, :, j]
    return wave_fold(s)


def lane_sum1(t):
    """the l2norm kernel's order: lane l adds elements l, l + 64, ..."""
    rows, D = t.shape
    K = (D + 63) // 64
    t = F.pad(t, (0, K * 64 - D)).view(rows, K, 64)
    s = torch.zeros(rows, 64)
    for i in range(K):
        s = s + t[:, i]
    return wave_fold(s)


def within(got, ref, bound):
    r = rb.ratio(got, ref, bound)
    assert r <= 1.0, r
    return r


def caught(mutant, cases):
    """cases: iterable of (case name, err / bound of the mutant): the worst must exceed 1; the message names it"""
    name, r = max(cases, key=lambda c: c[1])
    assert r > 1.0, f"mutant '{mutant}' stays within the bound everywhere; its worst case is [{name}] at err/bound {r}"
    print(f"mutant '{mutant}' leaves the bound at [{name}]: err/bound {r:.3g}")


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def emu_ln_fwd(t, eps, mutant=None):
    x = t["x"].to(F32)
    D = x.shape[1]
    Df = torch.tensor(float(D), dtype=F32)
    live = x[:, :512] if mutant == "second_chunk" else x                # the mutant never reads channels >= 512 for its statistics
    mean = lane_sum8(live) / Df
    d = x - mean[:, None]
    dl = d[:, :512] if mutant == "second_chunk" else d
    var = lane_sum8(dl * dl) / (Df - 1 if mutant == "var_dm1" else Df)
    e32 = torch.tensor(eps, dtype=F32)
    rstd = 1.0 / (torch.sqrt(var) + e32) if mutant == "eps_outside" else torch.rsqrt(var + e32)
    o = d * rstd[:, None] * t["gamma"] + t["beta"]
    y = trunc_bf16(o) if mutant == "trunc_store" else o.to(BF)
    y2 = ((o if mutant == "y2_unrounded" else y.to(F32)) + t["add"].to(F32)).to(BF)
    return mean, rstd, y, y2


def ln_blocks(rows, deferred):
    return min(512, (rows + 7) // 8) if deferred else min(128, (rows + 15) // 16)


def emu_ln_bwd(t, mean, rstd, deferred, mutant=None, keep=None, p=0.0):
    x, dy, gam = t["x"].to(F32), t["dy"].to(F32), t["gamma"]
    rows, D = x.shape
    Df = torch.tensor(float(D), dtype=F32)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gam
    s1 = lane_sum8(g) / Df
    s2 = lane_sum8(g * xh) / (Df - 1 if mutant == "s2_dm1" else Df)
    o = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
    dx = o.to(BF)
    dxd = None if keep is None else torch.where(keep, o * rw.f32_scale(p), torch.zeros(())).to(BF)
    # parameter gradients: wave w of the grid walks rows w, w + nwaves, ...; the block's 4 waves fold in LDS as (0 + 1) + (2 + 3); then one atomic
    # per block (here: in block order) or one partial row per block, folded in block order and added to the contents
    blocks = ln_blocks(rows, deferred)
    nw = 4 * blocks
    R = (rows + nw - 1) // nw
    valid = (torch.arange(R * nw) < rows).view(R, nw)
    if mutant == "last_row":
        nxt = torch.cat([valid[1:], torch.zeros(1, nw, dtype=torch.bool)])
        valid = valid & nxt                                                           # the last row a wave walks never reaches its sums
    out = []
    for term, init in ((dy * xh, t["dg0"]), (dy, t["db0"])):
        term = F.pad(term, (0, 0, 0, R * nw - rows)).view(R, nw, D) * valid[..., None]
        a = torch.zeros(nw, D)
        for r in range(R):
            a = a + term[r]
        a = a.view(blocks, 4, D)
        blk = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
        acc = torch.zeros(D) if deferred else init.clone()
        for b in range(blocks):
            acc = acc + blk[b]
        out.append(init + acc if deferred else acc)
    return dx, out[0], out[1], dxd


def ln_cases():
    for D in rw.LN_D:
        for rows in rw.LN_ROWS:
            for eps in rw.LN_EPS:
                yield f"{rows}x{D} eps={eps:g}", rows, D, eps, 0.0
    for rows, D in rw.LN_BIG:
        yield f"{rows}x{D}", rows, D, 1e-5, 0.0
    yield "17x520 offset 4", 17, 520, 1e-5, 4.0


@functools.lru_cache(maxsize=None)
def ln_case(rows, D, eps, offset):
    t = rw.ln_inputs(rows, D, offset)
    fwd = rw.ln_fwd_ref(t["x"], t["gamma"], t["beta"], eps)
    mean, rstd, y, y2 = emu_ln_fwd(t, eps)
    return t, fwd, (mean, rstd, y, y2), rw.ln_bwd_ref(t["dy"], t["x"], mean, rstd, t["gamma"], t["dg0"], t["db0"])


def test_layernorm_emulation_within_every_bound():
    worst = 0.0
    for name, rows, D, eps, off in ln_cases():
        t, fwd, (mean, rstd, y, y2), bwd = ln_case(rows, D, eps, off)
        within(mean, *fwd["mean"]), within(rstd, *fwd["rstd"])
        worst = max(worst, within(y, *fwd["y"]))
        assert torch.equal(y2, rw.ln_y2_ref(y, t["add"])), name
        for deferred in (False, True):
            dx, dg, db, _ = emu_ln_bwd(t, mean, rstd, deferred)
            within(dx, *bwd["dx"]), within(dg, *bwd["dgamma"]), within(db, *bwd["dbeta"])
    assert worst > 0.5, worst                  # not vacuous: the correct emulation uses most of the bf16 bound
    rows, eps, p, seed = rw.LN_DROP            # dx_drop: the GPU grid's cases, with its masks
    for D in rw.LN_D:
        t, _, (mean, rstd, _, _), _ = ln_case(rows, D, eps, 0.0)
        keep = xr.elem_keep(rows, D, p, seed)
        ref = rw.ln_bwd_ref(t["dy"], t["x"], mean, rstd, t["gamma"], t["dg0"], t["db0"], keep=keep, p=p)
        dxd = emu_ln_bwd(t, mean, rstd, False, keep=keep, p=p)[3]
        within(dxd, *ref["dx_drop"])
        assert not dxd[~keep].any()
        unscaled = emu_ln_bwd(t, mean, rstd, False, keep=keep, p=0.0)[3]          # the mask without the factor 1 / (1 - p)
        assert rb.ratio(unscaled, *ref["dx_drop"]) > 1.0, f"dx_drop without its scale stays within the bound at {rows}x{D}"


def test_layernorm_constant_row_is_exact_in_the_emulation():
    for D in (8, 520, 768):
        t = rw.ln_inputs(5, D)
        t["x"][1] = 2.75
        for eps in rw.LN_EPS:
            mean, _, y, _ = emu_ln_fwd(t, eps)
            assert float(mean[1]) == 2.75 and torch.equal(y[1], t["beta"].to(BF))


@pytest.mark.parametrize("mutant", ["var_dm1", "eps_outside", "second_chunk", "trunc_store", "y2_unrounded"])
def test_layernorm_forward_mutants_exceed_the_bound(mutant):
    def ratios():
        for name, rows, D, eps, off in ln_cases():
            t, fwd, _, _ = ln_case(rows, D, eps, off)
            mean, rstd, y, y2 = emu_ln_fwd(t, eps, mutant)
            if mutant == "y2_unrounded":       # y2 is held bit for bit to bf16(bf16(y) + add) of the y that was written
                yield name, float("inf") if not torch.equal(y2, rw.ln_y2_ref(y, t["add"])) else 0.0
            else:
                yield name, max(rb.ratio(mean, *fwd["mean"]), rb.ratio(rstd, *fwd["rstd"]), rb.ratio(y, *fwd["y"]))
    caught(mutant, ratios())


@pytest.mark.parametrize("mutant", ["s2_dm1", "last_row"])
def test_layernorm_backward_mutants_exceed_the_bound(mutant):
    def ratios():
        for name, rows, D, eps, off in ln_cases():
            t, _, (mean, rstd, _, _), bwd = ln_case(rows, D, eps, off)
            for deferred in (False, True):
                dx, dg, db, _ = emu_ln_bwd(t, mean, rstd, deferred, mutant)
                yield f"{name} {'deferred' if deferred else 'atomic'}", max(rb.ratio(dx, *bwd["dx"]), rb.ratio(dg, *bwd["dgamma"]), rb.ratio(db, *bwd["dbeta"]))
    caught(mutant, ratios())


# ------------------------------------------------------------------------------------------------------------------ softmax
def emu_sm_fwd(t, mutant=None):
    Sk, ld, rows = t["Sk"], t["ld"], t["rows"]
    s = t["scores"].to(F32)
    col = torch.arange(ld)
    dead = (col >= Sk)[None, :].expand(rows, ld).clone()
    if mutant == "last_key_dead":
        dead |= (col == Sk - 1)[None, :]
    if t["key_pad"] is not None:
        row = torch.arange(rows)
        img = (row // rw.SM_SQ) % rw.SM_NB if mutant == "wrong_image" else row // (rw.SM_H * rw.SM_SQ)
        dead[:, :Sk] |= t["key_pad"].bool()[img]
    v = s.masked_fill(dead, float("-inf"))
    e = torch.exp(v - v.max(1, keepdim=True).values)
    es = e.clone()
    if mutant == "chunk1":
        es[:, 512:1024] = 0                    # register chunk 1 never reaches the sum
    inv = 1.0 / lane_sum8(es)
    return (e * inv[:, None]).to(BF)


def emu_sm_bwd(p, dp, Sk, mutant=None):
    pv, gv = p.to(F32).clone(), dp.to(F32).clone()
    if mutant != "dot_over_ld":
        pv[:, Sk:], gv[:, Sk:] = 0, 0
    dot = lane_sum8(pv * gv)
    pv[:, Sk:] = 0
    return (pv * (gv - dot[:, None])).to(BF)


def sm_cases(min_sk=1):
    for Sk in rw.SM_SK:
        if Sk >= min_sk:
            for ld in rw.sm_lds(Sk):
                for pad in rw.sm_pads(Sk):
                    yield f"Sk={Sk} ld={ld} pad={pad}", Sk, ld, pad


@functools.lru_cache(maxsize=None)
def sm_case(Sk, ld, pad):
    t = rw.sm_inputs(Sk, ld, pad)
    p = emu_sm_fwd(t)
    p[:, Sk:] = 0.25                           # what the GPU test hands to the backward: garbage in the pad columns
    return t, rw.sm_fwd_ref(t), p, rw.sm_bwd_ref(p, t["dp"], Sk)


def test_softmax_emulation_within_every_bound():
    worst = 0.0
    for name, Sk, ld, pad in sm_cases():
        t, fref, p, bref = sm_case(Sk, ld, pad)
        got = emu_sm_fwd(t)
        worst = max(worst, within(got, *fref))
        assert not got[:, Sk:].any(), name
        ds = emu_sm_bwd(p, t["dp"], Sk)
        within(ds, *bref)
        assert not ds[:, Sk:].any(), name
    assert worst > 0.5, worst


@pytest.mark.parametrize("mutant", ["last_key_dead", "wrong_image", "chunk1"])
def test_softmax_forward_mutants_exceed_the_bound(mutant):
    # a dead key Sk - 1 at Sk = 1 leaves no key at all (NaN by construction): that mutant is judged from Sk = 7 on
    caught(mutant, ((name, rb.ratio(emu_sm_fwd(sm_case(Sk, ld, pad)[0], mutant), *sm_case(Sk, ld, pad)[1]))
                    for name, Sk, ld, pad in sm_cases(7 if mutant == "last_key_dead" else 1)))


def test_softmax_backward_mutant_exceeds_the_bound():
    caught("dot_over_ld", ((name, rb.ratio(emu_sm_bwd(sm_case(Sk, ld, pad)[2], sm_case(Sk, ld, pad)[0]["dp"], Sk, "dot_over_ld"), *sm_case(Sk, ld, pad)[3]))
                           for name, Sk, ld, pad in sm_cases()))


# ------------------------------------------------------------------------------------------------------------------ colsum
def emu_colsum(g, out0, narrow=False, mutant=None):
    """generic: slabs of 256 rows, row lane ry adds rows ry, ry + 8, ... of its slab, the 8 lanes fold in order, one atomic per slab (in slab order).
    narrow: blocks of 8192 rows, 256 / (N / 8) rows per pass."""
    M, N = g.shape
    slab, lanes = (rw.CS_ROWS, 256 // (N // 8)) if narrow else (256, 8)
    nb = (M + slab - 1) // slab
    g = g.to(F32)
    if mutant == "ragged_pass":                # a pass runs only when all its rows exist: the rows behind the last full pass of the last block are lost
        g = g[:M - (M - (nb - 1) * slab) % lanes]
    if mutant == "last_block" and M % slab:    # the grid is M / 8192 rounded DOWN
        g = g[:(nb - 1) * slab]
    t = F.pad(g, (0, 0, 0, nb * slab - g.shape[0])).view(nb, slab // lanes, lanes, N)
    if mutant == "tail_column" and N % 8:
        t = t.clone()
        t[..., N - 1] = 0                      # the last column of a chunk with n + 8 > N is never read
    a = torch.zeros(nb, lanes, N)
    for i in range(slab // lanes):
        a = a + t[:, i]
    s = torch.zeros(nb, N)
    for r in range(lanes):
        s = s + a[:, r]
    out = torch.zeros(N) if mutant == "overwrite" else out0.clone()
    for b in range(nb):
        out = out + s[b]
    return out


def cs_cases():
    for M in rw.CS_M:
        for N in rw.CS_N:
            for kind in rw.CS_LD:
                yield f"{M}x{N} ld={kind}", M, N, kind, False
    for M in rw.CS_NARROW_M:
        for N in rw.CS_NARROW_N:
            yield f"{M}x{N} narrow", M, N, "N", True
    yield "32768x24 ld=N", 32768, 24, "N", False


def test_colsum_emulation_within_every_bound():
    for name, M, N, kind, narrow in cs_cases():
        _, view, _, out0 = rw.cs_inputs(M, N, kind)
        within(emu_colsum(view, out0, narrow), *rw.colsum_ref(view, out0))


@pytest.mark.parametrize("mutant", ["tail_column", "overwrite"])
def test_colsum_mutants_exceed_the_bound(mutant):
    def ratios():
        for name, M, N, kind, narrow in cs_cases():
            _, view, _, out0 = rw.cs_inputs(M, N, kind)
            yield name, rb.ratio(emu_colsum(view, out0, narrow, mutant), *rw.colsum_ref(view, out0))
    caught(mutant, ratios())


@pytest.mark.parametrize("mutant", ["ragged_pass", "last_block"])
def test_colsum_narrow_mutants_exceed_the_bound_at_every_width(mutant):
    """the ragged last block of 40997 rows (37 rows; 5 of them behind the last full pass at N = 64 and 128, all 37 at N <= 32): each width on its own"""
    M = rw.CS_NARROW_M[1]
    for N in rw.CS_NARROW_N:
        _, view, _, out0 = rw.cs_inputs(M, N, "N")
        r = rb.ratio(emu_colsum(view, out0, True, mutant), *rw.colsum_ref(view, out0))
        assert r > 1.0, f"mutant '{mutant}' stays within the bound at [{M}x{N} narrow]: err/bound {r}"
    _, view, _, out0 = rw.cs_inputs(32768, 24, "N")                                  # and ONE element lost anywhere among the tall inputs
    ref, bound = rw.colsum_ref(view, out0)
    assert float(bound.max()) < 0.5 and float(view.to(F32).abs()[view != 0].min()) >= 1.0


def test_recorded_widening_factor_is_the_one_the_reference_used(monkeypatch):
    monkeypatch.setitem(rb.ACC_WIDEN, "colsum", 2.0)
    monkeypatch.setitem(rb.ACC_WIDEN, "layernorm_bwd", 4.0)
    assert rw.widen_of("colsum (narrow)") == 2.0 and rw.widen_of("layernorm_bwd.dgamma (atomic)") == 4.0 and rw.widen_of("l2norm_fwd") == 1.0
    _, view, _, out0 = rw.cs_inputs(255, 9, "N")
    assert torch.equal(rw.colsum_ref(view, out0)[1], 2.0 * (255 + 3) * rb.U * (view.double().abs().sum(0) + out0.double().abs()))


# ------------------------------------------------------------------------------------------------------------------ exact kernels
def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(rw.bits(got), rw.bits(want))


def test_add_and_dropout_emulations_on_their_grids():
    """the kernel's statement by another road: the exact (fp64) sum or product, rounded once to f32 as the f32 operation rounds it, then to bf16; b by
    the index i % b_period; on every (n, period) and (n, p) of the GPU grids, the strided sizes included"""
    for n, period in rw.ADD_CASES:
        a, b = rw.add_inputs(n, period)
        got = (a.double() + b.double()[torch.arange(n) % (period or n)]).to(F32).to(BF)
        assert same_bits(got, rw.add_ref(a, b, period)), (n, period)
        if period:
            assert not same_bits((a.double() + b.double()[(torch.arange(n) + 1) % period]).to(F32).to(BF), rw.add_ref(a, b, period))       # b one element off
    for n in rw.DROP_N:
        for p in rw.DROP_P:
            x, seed = rw.drop_inputs(n, p)
            keep = xr.elem_keep(1, n, p, seed).view(-1)
            got = torch.where(keep, (x.double() * float(rw.f32_scale(p))).to(F32).to(BF), torch.zeros((), dtype=BF))
            want = rw.dropout_ref(x, keep, p)
            assert same_bits(got, want) and not want[~keep].any(), (n, p)
            if p:
                assert not same_bits(torch.where(keep, x, torch.zeros((), dtype=BF)), want), (n, p)                                        # the scale forgotten
            else:
                assert bool(keep.all()) and same_bits(want, x)


def test_pack_unpack_maxpool_emulations_on_their_grids():
    """the kernels' own index arithmetic on flat buffers, on every shape of the GPU grids (the strided ones included)"""
    for N, C, H, W in [(n, c, h, w) for c in rw.PACK_C for n, h, w in rw.PACK_NHW] + [rw.PACK_BIG]:
        x = rw.pack_inputs(N, C, H, W)
        pix, c = torch.arange(N * H * W)[:, None], torch.arange(8)[None, :]
        n, hw = pix // (H * W), pix % (H * W)
        src = x.reshape(-1)[((n * C + c.clamp(max=C - 1)) * H * W + hw)]
        got = torch.where(c < C, src, torch.zeros(())).to(BF).view(N, H, W, 8)
        assert same_bits(got, rw.pack_ref(x)), (N, C, H, W)
        assert not same_bits(trunc_bf16(torch.where(c < C, src, torch.zeros(()))).view(N, H, W, 8), rw.pack_ref(x)) or N * H * W == 1      # a truncating store
    for N, HW, C in rw.UNPACK:
        x = rw.unpack_inputs(N, HW, C)
        o = torch.arange(N * C * HW)
        n, c, p_ = o // (C * HW), o // HW % C, o % HW
        assert same_bits(x.reshape(-1)[(n * HW + p_) * C + c].to(F32).view(N, C, HW), rw.unpack_ref(x)), (N, HW, C)
    cases = [(n, h, w, c, False) for c in rw.POOL_C for n, h, w in rw.POOL_NHW] + [(2, 7, 9, c, True) for c in rw.POOL_C] + [rw.POOL_BIG + (False,)]
    for N, H, W, C, neg in cases:
        x = rw.pool_inputs(N, H, W, C, negative=neg)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1

        def pool(fill):
            xp = F.pad(x.to(F32), (0, 0, 1, 2, 1, 2), value=fill)                     # taps oy * 2 - 1 + dy: one ring before, enough behind
            m = torch.full((N, OH, OW, C), float("-inf"))
            for dy in range(3):
                for dx in range(3):
                    m = torch.maximum(m, xp[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
            return m.to(BF)
        assert same_bits(pool(float("-inf")), rw.maxpool_ref(x)), (N, H, W, C)
        if neg:
            assert not same_bits(pool(0.0), rw.maxpool_ref(x))                        # padding that contributes a 0


# ------------------------------------------------------------------------------------------------------------------ embeddings
def test_embed_emulations_and_the_type_row_mutant():
    def ratios():
        for D in rw.EMB_D:
            for B, L in rw.EMB_BL:
                t = rw.emb_inputs(B, L, D)
                pos_ids = rw.position_ids(t["ids"])
                assert int(pos_ids.max()) < t["pos"].shape[0]
                ref = rw.embed_fwd_ref(t["ids"], pos_ids, t["word"], t["pos"], t["type"][0])
                idf, pf = t["ids"].reshape(-1), pos_ids.reshape(-1)
                for n in range(B * L):                                                # the kernel's statement, token by token
                    assert torch.equal(ref[n], ((t["word"][idf[n]] + t["type"][0]) + t["pos"][pf[n]]).to(BF))
                bad = rw.embed_fwd_ref(t["ids"], pos_ids, t["word"], t["pos"], t["type"][1])
                yield f"n={B * L} D={D}", float("inf") if not torch.equal(bad, ref) else 0.0
    caught("type row 1", ratios())
    for D in rw.TYPE_D:
        for n in rw.TYPE_N:
            gen = torch.Generator().manual_seed(100 * n + D)
            g, d0 = torch.randn(n, D, generator=gen).to(BF), torch.randn(D, generator=gen) + 1.5
            t = F.pad(g.to(F32), (0, 0, 0, (n + 7) // 8 * 8 - n)).view(-1, 8, D)          # token lane ry adds tokens ry, ry + 8, ...
            a = torch.zeros(8, D)
            for i in range(t.shape[0]):
                a = a + t[i]
            s = torch.zeros(D)
            for r in range(8):
                s = s + a[r]
            ref, bound = rw.embed_type_ref(g, d0)
            within(d0 + s, ref, bound)
            assert rb.ratio(s, ref, bound) > 1.0                                      # overwritten instead of accumulated


# ------------------------------------------------------------------------------------------------------------------ sine position
def emu_sine(mask, mutant=None):
    """-> [B, H, W, 2F] f32, the kernel's operations in f32"""
    nf = rw.SINE_F
    nm = (~mask).to(F32)
    ye, xe = nm.cumsum(1), nm.cumsum(2)
    yt, xt = ye[:, -1:, :].clone(), xe[:, :, -1:].clone()
    if mutant == "count_to_y_minus_1":
        ye, xe = ye - nm, xe - nm
    eps, two_pi = torch.tensor(1e-6, dtype=F32), torch.tensor(6.283185307179586, dtype=F32)
    ay, ax = ye / (yt + eps) * two_pi, xe / (xt + eps) * two_pi
    j = torch.arange(nf // 2, dtype=F32)
    ex = (j if mutant == "exponent_j_over_F" else 2 * j) / nf
    dim_t = torch.pow(torch.tensor(rw.SINE_T, dtype=F32), ex)

    def half(a):
        th = a[..., None] / dim_t
        pair = [th.cos(), th.sin()] if mutant == "sin_cos_swapped" else [th.sin(), th.cos()]
        return torch.stack(pair, -1).flatten(3)
    hy, hx = half(ay), half(ax)
    return torch.cat([hx, hy] if mutant == "halves_swapped" else [hy, hx], 3)


def sine_cases():
    for B, H, W in rw.SINE_BHW + [rw.SINE_BIG]:
        for kind in (rw.SINE_MASKS if (B, H, W) != rw.SINE_BIG else ["random"]):
            yield f"{B}x{H}x{W} mask={kind}", rw.sine_mask(B, H, W, kind)


def test_sine_emulation_within_every_bound():
    assert rw.SINE_LIB > 0                     # the measured library term is in place
    for name, mask in sine_cases():
        v = emu_sine(mask)
        B, H, W, C = v.shape
        within(v.permute(0, 3, 1, 2), *rw.sine_nchw_ref(mask))
        within(v.reshape(B, H * W, C).to(BF), *rw.sine_tok_ref(mask))
        seq = F.pad(v.reshape(B, H * W, C).to(BF), (0, 0, 0, 16))
        within(seq, *rw.sine_tok_ref(mask, 16))


@pytest.mark.parametrize("mutant", ["sin_cos_swapped", "exponent_j_over_F", "count_to_y_minus_1", "halves_swapped"])
def test_sine_mutants_exceed_the_bound(mutant):
    def ratios():
        for name, mask in sine_cases():
            v = emu_sine(mask, mutant)
            B, H, W, C = v.shape
            yield name, rb.ratio(v.reshape(B, H * W, C).to(BF), *rw.sine_tok_ref(mask))       # the bf16 output: the wider of the two bounds
    caught(mutant, ratios())


# ------------------------------------------------------------------------------------------------------------------ l2norm
def emu_l2(x, dy):
    eps = torch.tensor(1e-12, dtype=F32)
    inv = 1.0 / torch.maximum(torch.sqrt(lane_sum1(x * x)), eps)[:, None]
    dot = lane_sum1(x * inv * dy)[:, None]
    return x * inv, (dy - x * inv * dot) * inv


def test_l2norm_emulation_within_every_bound_and_mutants_outside():
    short, flat = [], []
    for D in rw.L2_D:
        for rows in rw.L2_ROWS:
            t = rw.l2_inputs(rows, D)
            y, dx = emu_l2(t["x"], t["dy"])
            fref, bref = rw.l2norm_fwd_ref(t["x"]), rw.l2norm_bwd_ref(t["x"], t["dy"])
            within(y, *fref), within(dx, *bref)
            if rows >= 5:
                assert not y[2].any()
                assert torch.equal(dx[2], t["dy"][2] * (torch.tensor(1.0) / torch.tensor(1e-12, dtype=F32)))
            xm = t["x"].clone()                # mutant 1: the last element of a row never reaches the norm (D = 1: the norm is the clamp)
            xm[:, -1] = 0
            short.append((f"{rows}x{D}", rb.ratio(t["x"] / xm.norm(dim=1, keepdim=True).clamp(min=1e-12), *fref)))
            inv = 1.0 / t["x"].norm(dim=1, keepdim=True).clamp(min=1e-12)              # mutant 2: the backward without its projection term
            flat.append((f"{rows}x{D}", rb.ratio(t["dy"] * inv, *bref)))
    caught("l2norm_fwd: last element missing from the norm", short)
    caught("l2norm_bwd: no projection term", flat)
