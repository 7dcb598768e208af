"""The bounds of tests/attn_bounds.py are neither wrong nor vacuous: a torch f32 EMULATION of each attention core's arithmetic -- the forward's 128-key
blocks with a running maximum, one rescale alpha per block, four per-lane-group row sums and probabilities rounded to bf16 before P V; the backward's
32-key waves, 128-key splits with nw active waves, 32-query tiles dealt to two groups, dS and Pd rounded to bf16; attn_small's 16 / 32 / 64-lane row
groups folded by xor butterflies -- stays within `bound` on every case the GPU tests run (tests/test_gpu_attn_cores.py), and named mutants of the
emulation, the ways such kernels go wrong, leave it on the case named beside them.  The references read rounding_bounds.ACC_WIDEN when called, so an
entry there is in force for the mutants too."""
import functools

import pytest
import torch

import attn_bounds as ab
import rounding_bounds as rb
from rounding_bounds import BF, F32

F = torch.nn.functional
NAN = float("nan")
LOG2E = torch.tensor(1.4426950408889634, dtype=F32)


def f32t(x):
    return torch.tensor(x, dtype=F32)


def dscale_f32(p):
    return f32t(1.0) / (f32t(1.0) - f32t(p)) if p > 0 else f32t(1.0)


# ------------------------------------------------------------------------------------------------------------------ attn2 forward
def _a2_operands(t, KP, keep_ld=None, tail_live=False, dead_shift=False):
    B, H, dh, Sq, Sk = t["B"], t["H"], t["dh"], t["Sq"], t["Sk"]
    q = ab.heads(t["q"].float(), B, Sq, H, dh)
    k = F.pad(ab.heads(t["k"].float(), B, Sk, H, dh), (0, 0, 0, KP - Sk))          # keys past Sk are staged as zeros
    v = F.pad(ab.heads(t["v"].float(), B, Sk, H, dh), (0, 0, 0, KP - Sk))
    dead = torch.zeros(B, KP, dtype=torch.bool)
    if not tail_live:
        dead[:, Sk:] = True
    if t["key_pad"] is not None:
        dead[:, :Sk] |= t["key_pad"].bool()
    if dead_shift:
        dead = torch.cat([torch.zeros(B, 1, dtype=torch.bool), dead[:, :-1]], 1)
    keep = F.pad(ab.a2_keep(B * H, Sq, Sk, t["p"], t["seed"], ld=keep_ld).view(B, H, Sq, Sk), (0, KP - Sk), value=True)
    return B, H, dh, Sq, Sk, q, k, v, dead.view(B, 1, 1, KP), keep


def emu_a2_fwd(t, mutant=None):
    """attn2_fwd_kernel in f32: -> (ctx bf16 [B * Sq, 96], lse f32 [B * H, Sq, 2])"""
    KP = (t["Sk"] + 127) // 128 * 128
    B, H, dh, Sq, Sk, q, k, v, dead, keep = _a2_operands(t, KP, keep_ld=t["Sk"] if mutant == "pair_pitch_sk" else None, tail_live=mutant == "tail_live",
                                                         dead_shift=mutant == "dead_shift")
    c = f32t(t["scale"]) * LOG2E
    p_drop = t["p"]
    m = torch.full((B, H, Sq, 1), float("-inf"))
    l = torch.zeros(B, H, Sq, 4)                                  # one partial row sum per lane group g: keys 16 j + 4 g + r of every block
    acc = torch.zeros(B, H, Sq, dh)
    for k0 in range(0, KP, 128):
        sl = slice(k0, k0 + 128)
        s = (q @ k[..., sl, :].transpose(-1, -2)).masked_fill(dead[..., sl], float("-inf"))
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        msafe = torch.where(mn == float("-inf"), torch.zeros_like(mn), mn)
        alpha = torch.exp2((m - msafe) * c)                       # m = -inf: 0
        m = mn
        p = torch.exp2((s - msafe) * c)
        pd = torch.where(keep[..., sl], p, torch.zeros_like(p))
        l = l * alpha + (pd if mutant == "sum_after_dropout" else p).view(B, H, Sq, 8, 4, 4).sum((3, 5))
        if mutant != "no_alpha":
            acc = acc * alpha
        acc = acc + pd.to(BF).float() @ v[..., sl, :]
    lsum = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    inv = (1.0 / lsum).unsqueeze(-1)
    os = inv / (f32t(1.0) - f32t(p_drop)) if p_drop > 0 and mutant != "fwd_no_dropscale" else inv
    return ab.rows(acc * os).to(BF), torch.stack([m[..., 0], inv[..., 0]], -1).reshape(B * H, Sq, 2)


# ------------------------------------------------------------------------------------------------------------------ attn2 backward
def emu_a2_bwd(t, ctx, lse, mutant=None):
    """the key-owning backward in f32 from (q, k, v, ctx, dctx, lse): -> (list of dq shares bf16 [B * Sq, 96], one per split, unwritten rows NaN;
    dk, dv bf16 [B * Sk, 96])"""
    splits = ab.a2_splits(t["Sk"])
    KP = splits * 128
    B, H, dh, Sq, Sk, q, k, v, dead, keep = _a2_operands(t, KP)
    dO, O = ab.heads(t["dctx"].float(), B, Sq, H, dh), ab.heads(ctx.float(), B, Sq, H, dh)
    scale = f32t(t["scale"])
    c = scale * LOG2E
    ls = lse.view(B, H, Sq, 2)
    m, rs = ls[..., :1], ls[..., 1:]
    m = torch.where(m == float("-inf"), torch.zeros_like(m), m)
    ds_c = dscale_f32(t["p"])
    D = (dO * O).sum(-1, keepdim=True)
    if mutant == "d_from_undropped_context":
        pf = torch.exp2(((q @ k.transpose(-1, -2)).masked_fill(dead, float("-inf")) - m) * c) * rs
        D = (dO * (pf @ v)).sum(-1, keepdim=True)
    nkp, n_tiles = (Sk + 31) // 32, (Sq + 31) // 32
    skipped = None
    if mutant == "group1_last_tile_skipped":
        assert n_tiles >= 2
        skipped = n_tiles - 1 if (n_tiles - 1) % 2 == 1 else n_tiles - 2
    dk, dv = torch.zeros(B, H, KP, dh), torch.zeros(B, H, KP, dh)
    dq = [torch.full((B * Sq, H * dh), NAN, dtype=BF) for _ in range(splits)]
    for sp in range(splits):
        nw = min(4, nkp - 4 * sp)
        slabs = []
        for w in range(nw):                                        # the active waves of the split: 32 keys each
            ks = slice((4 * sp + w) * 32, (4 * sp + w) * 32 + 32)
            kw, vw, kp_ = k[..., ks, :], v[..., ks, :], keep[..., ks]
            sc = (q @ kw.transpose(-1, -2)).masked_fill(dead[..., ks], float("-inf"))
            dpd = dO @ vw.transpose(-1, -2)
            p = torch.exp2((sc - m) * c) * rs
            zero = torch.zeros_like(p)
            pdv = torch.where(kp_, p * ds_c, zero)
            dp = torch.where(kp_, dpd if mutant == "dp_no_dropscale" else dpd * ds_c, zero)
            dsb, pdb = (p * (dp - D)).to(BF).float(), pdv.to(BF).float()
            accK, accV = [0.0, 0.0], [0.0, 0.0]                    # the two query groups: every second 32-query tile each
            for tl in range(n_tiles):
                if tl == skipped:
                    continue
                qs = slice(32 * tl, min(Sq, 32 * tl + 32))
                accK[tl % 2] = accK[tl % 2] + dsb[..., qs, :].transpose(-1, -2) @ q[..., qs, :]
                accV[tl % 2] = accV[tl % 2] + pdb[..., qs, :].transpose(-1, -2) @ dO[..., qs, :]
            dk[..., ks, :] = (accK[0] + accK[1]) * scale
            dv[..., ks, :] = accV[0] + accV[1]
            slabs.append(dsb @ kw)
        a = slabs[0]
        for w in range(1, nw):
            a = a + slabs[w]
        if mutant == "nw_always_4":
            for w in range(nw, 4):
                a = a + slabs[0]                                   # an inactive wave never writes its slab: what lies there is stale (here: wave 0's share)
        out = ab.rows(a if mutant == "dq_no_scale" else a * scale).to(BF)
        if skipped is not None:
            out = out.view(B, Sq, H * dh).clone()
            out[:, 32 * skipped:32 * skipped + 32] = NAN
            out = out.view(B * Sq, H * dh)
        dq[(sp + 1) % splits if mutant == "neighbour_part" else sp] = out
    return dq, ab.rows(dk[..., :Sk, :]).to(BF), ab.rows(dv[..., :Sk, :]).to(BF)


@functools.lru_cache(maxsize=None)
def a2_case(Sq, Sk, p, pad):
    """inputs, forward reference, backward reference from the forward reference's host-built (ctx, lse): computed once, never changed"""
    t = ab.a2_inputs(Sq, Sk, p, pad)
    fwd = ab.a2_fwd_ref(t)
    return t, fwd, ab.a2_bwd_ref(t, *fwd["host"])


def a2_case_at(Sq, Sk, pad):
    """the case of the grid at this shape and pattern (its dropout value follows from the rotation)"""
    found = [c for c in ab.a2_cases() if (c[0], c[1], c[3]) == (Sq, Sk, pad)]
    assert found, (Sq, Sk, pad)
    return max(found, key=lambda c: c[2])                  # where a pattern takes all three values: the largest


def a2_fwd_ratios(t, fwd, mutant=None):
    ctx, lse = emu_a2_fwd(t, mutant)
    return dict(ctx=rb.ratio(ctx, *fwd["ctx"]), lse_max=rb.ratio(lse[..., 0], *fwd["lse_max"]), lse_rsum=rb.ratio(lse[..., 1], *fwd["lse_rsum"]))


def a2_bwd_ratios(t, fwd, bwd, mutant=None):
    dq, dk, dv = emu_a2_bwd(t, *fwd["host"], mutant)
    out = dict(dk=rb.ratio(dk, *bwd["dk"]), dv=rb.ratio(dv, *bwd["dv"]))
    for i, (got, rbnd) in enumerate(zip(dq, bwd["dq"])):
        out[f"dq[{i}]"] = rb.ratio(got, *rbnd)
    return out


def test_attn2_grid_reaches_the_seams():
    """what the shapes are there for: Sq on 16 / 32 / 64, 1 2 3 4 6 query tiles (an odd and an even count of iterations per group), Sk on 32 / 128 / 512,
    odd and no multiple of 8, 1 2 5 6 key splits, one and four active waves in the last split; every pattern and every dropout value on every shape"""
    shp = ab.A2_SHAPES
    assert {(Sq + 31) // 32 for Sq, _ in shp} == {1, 2, 3, 4, 6}
    assert {((Sq + 31) // 32 + 1) // 2 % 2 for Sq, _ in shp} == {0, 1}
    assert {16, 32, 64} <= {Sq for Sq, _ in shp if Sq % 16 == 0} | {Sq - 1 for Sq, _ in shp} and {32, 128, 512} <= {Sk - 1 for _, Sk in shp} | {Sk for _, Sk in shp}
    assert {ab.a2_splits(Sk) for _, Sk in shp} >= {1, 2, 5, 6}
    last_nw = {(ab.a2_splits(Sk), (Sk + 31) // 32 - 4 * (ab.a2_splits(Sk) - 1)) for _, Sk in shp}
    assert {nw for _, nw in last_nw} >= {1, 4} and any(Sk % 8 for _, Sk in shp)
    cases = list(ab.a2_cases())
    for Sq, Sk in shp:
        mine = [c for c in cases if c[:2] == (Sq, Sk)]
        assert {c[3] for c in mine} == set(ab.a2_pads(Sk)) and {c[2] for c in mine} == set(ab.A2_DROPS), (Sq, Sk)
    for pad in ab.A2_PADS:
        assert {c[2] for c in cases if c[3] == pad} == set(ab.A2_DROPS), pad
    assert set(ab.a2_pads(641)) == set(ab.A2_PADS)


def test_attn2_emulations_within_every_bound():
    worst = {}
    for case in ab.a2_cases():
        t, fwd, bwd = a2_case(*case)
        for name, r in {**a2_fwd_ratios(t, fwd), **a2_bwd_ratios(t, fwd, bwd)}.items():
            assert r <= 1.0, f"emulation outside the bound at [{ab.a2_name(*case)}] {name}: err/bound {r}"
            worst[name.split("[")[0]] = max(worst.get(name.split("[")[0], 0.0), r)
    assert worst["ctx"] > 0.2 and worst["dk"] > 0.2 and worst["dv"] > 0.2 and worst["dq"] > 0.2, f"vacuous bounds: {worst}"


def test_attn2_backward_emulation_fed_by_the_forward_emulation():
    """the two directions together, as the product runs them: the backward reference from the forward EMULATION's own (ctx, lse)"""
    for case in [(65, 641, "per_image"), (97, 129, "first_block"), (17, 17, "last")]:
        case = a2_case_at(*case)
        t = ab.a2_inputs(*case)
        ctx, lse = emu_a2_fwd(t)
        bwd = ab.a2_bwd_ref(t, ctx, lse)
        dq, dk, dv = emu_a2_bwd(t, ctx, lse)
        for got, (ref, bound) in [(dk, bwd["dk"]), (dv, bwd["dv"])] + list(zip(dq, bwd["dq"])):
            assert rb.ratio(got, ref, bound) <= 1.0, case


def test_attn2_padded_and_dropped_elements_are_exactly_nothing():
    """rows of dk and dv at padded keys: reference 0, bound 0; a dq share whose 128 keys are all padded likewise"""
    t, fwd, bwd = a2_case(*a2_case_at(65, 641, "first_stage"))
    dead = t["key_pad"].bool().view(-1)
    for name in ("dk", "dv"):
        ref, bound = bwd[name]
        assert float(ref[dead].abs().max()) == 0.0 and float(bound[dead].max()) == 0.0 and float(bound[~dead].min()) > 0.0
    for sp in range(4):
        assert float(bwd["dq"][sp][0].abs().max()) == 0.0 and float(bwd["dq"][sp][1].max()) == 0.0
    assert float(bwd["dq"][4][1].min()) > 0.0


# mutant -> (direction, (Sq, Sk, pad) of the grid, the output that leaves its bound there)
A2_MUTANTS = {
    "no_alpha": ("fwd", (97, 129, "none"), "ctx"),                              # accumulator not rescaled when the maximum moves in the second block
    "tail_live": ("fwd", (65, 127, "none"), "lse_rsum"),                        # keys in [Sk, round128(Sk)) not marked dead: a score of 0 each
    "dead_shift": ("fwd", (64, 513, "block2_first"), "ctx"),                    # dead flag shifted by one key
    "pair_pitch_sk": ("fwd", (65, 127, "first"), "ctx"),                        # dropout pair index built with Sk instead of round8(Sk)
    "sum_after_dropout": ("fwd", (17, 17, "first"), "lse_rsum"),                # row sum taken after dropout
    "fwd_no_dropscale": ("fwd", (17, 17, "first"), "ctx"),                      # 1 / (1 - p) missing in the forward
    "dp_no_dropscale": ("bwd", (17, 17, "first"), "dk"),                        # 1 / (1 - p) missing on dP
    "d_from_undropped_context": ("bwd", (17, 17, "first"), "dk"),               # D from the pre-dropout context
    "nw_always_4": ("bwd", (97, 129, "none"), "dq[1]"),                         # an inactive wave's slab added
    "neighbour_part": ("bwd", (97, 129, "none"), "dq[0]"),                      # a split writing the neighbour's dq_part
    "group1_last_tile_skipped": ("bwd", (97, 129, "none"), "dq[0]"),            # the last query tile of group 1 skipped
    "dq_no_scale": ("bwd", (17, 17, "none"), "dq[0]"),                          # scale missing on dq
}


@pytest.mark.parametrize("mutant", sorted(A2_MUTANTS))
def test_attn2_mutants_leave_the_bound_on_their_named_case(mutant):
    direction, at, output = A2_MUTANTS[mutant]
    case = a2_case_at(*at)
    t, fwd, bwd = a2_case(*case)
    r = (a2_fwd_ratios(t, fwd, mutant) if direction == "fwd" else a2_bwd_ratios(t, fwd, bwd, mutant))[output]
    assert r > 1.0, f"mutant '{mutant}' stays within the bound of {output} at [{ab.a2_name(*case)}]: err/bound {r}"


# ------------------------------------------------------------------------------------------------------------------ attn_small
def butterfly(v, op):
    """the xor butterfly over the G lanes [..., G] of a row group -> [...]"""
    G = v.shape[-1]
    lanes = torch.arange(G)
    o = G >> 1
    while o > 0:
        v = op(v, v[..., lanes ^ o])
        o >>= 1
    return v[..., 0]


def _as_operands(t, mutant):
    B, H, dh, S = t["B"], t["H"], t["dh"], t["S"]
    load = lambda n, b: ab.heads(t[n].float(), B, S, H, dh) + (0.0 if t[b] is None or (mutant == "bias_on_k_not_q" and b == "bq") else t[b].view(1, H, 1, dh))
    q, k, v = load("q", "bq"), load("k", "bk"), load("v", "bv")
    dead = (torch.zeros(B, 1, 1, S, dtype=torch.bool) if t["key_pad"] is None else t["key_pad"].bool().view(B, 1, 1, S))
    keep = ab.small_attn_keep(B, H, S, t["p"], t["seed"]) if t["p"] > 0 else torch.ones(B, H, S, S, dtype=torch.bool)
    s = ((q @ k.transpose(-1, -2)) * f32t(t["scale"])).masked_fill(dead, float("-inf"))
    return B, H, dh, S, q, k, v, keep, s


def emu_as_fwd(t, mutant=None):
    """attn_small_fwd_kernel in f32: -> (ctx bf16 [B * S, H dh], stats f32 [B * H, S, 2]); __expf(x) = exp2(x log2(e))"""
    B, H, dh, S, q, k, v, keep, s = _as_operands(t, mutant)
    G = 64 if mutant == "lane_group_64" else (16 if S <= 16 else (32 if S <= 32 else 64))
    sp = F.pad(s, (0, G - S), value=0.0 if mutant == "lane_group_64" else float("-inf"))       # the mutant reads jl >= S as a score of 0 (stale LDS)
    mx = butterfly(sp, torch.maximum).unsqueeze(-1)
    rs = 1.0 / butterfly(torch.exp2((sp - mx) * LOG2E), torch.add).unsqueeze(-1)
    pv = torch.exp2((s - mx) * LOG2E) * rs
    pd = torch.where(keep, pv * dscale_f32(t["p"]), torch.zeros_like(pv))
    return ab.rows(pd @ v).to(BF), torch.stack([mx[..., 0], rs[..., 0]], -1).reshape(B * H, S, 2)


def emu_as_bwd(t, stats, mutant=None):
    """attn_small_bwd_kernel in f32 from the given statistics: -> dq, dk, dv bf16 [B * S, H dh]"""
    B, H, dh, S, q, k, v, keep, s = _as_operands(t, mutant)
    g = ab.heads(t["dctx"].float(), B, S, H, dh)
    st = stats.view(B, H, S, 2)
    p = torch.exp2((s - st[..., :1]) * LOG2E) * st[..., 1:]
    dsc = dscale_f32(t["p"])
    zero = torch.zeros_like(p)
    pd = torch.where(keep, p * dsc, zero)
    dp = torch.where(keep, (g @ v.transpose(-1, -2)) * dsc, zero)
    G = 16 if S <= 16 else (32 if S <= 32 else 64)
    rowdot = butterfly(F.pad(p * dp, (0, G - S)), torch.add).unsqueeze(-1)
    dS = p * (dp - rowdot) * f32t(t["scale"])
    return ab.rows(dS @ k).to(BF), ab.rows(dS.transpose(-1, -2) @ q).to(BF), ab.rows(pd.transpose(-1, -2) @ g).to(BF)


@functools.lru_cache(maxsize=None)
def as_case(*case):
    t = ab.as_inputs(*case)
    fwd = ab.as_fwd_ref(t)
    return t, fwd, ab.as_bwd_ref(t, fwd["host"])


def as_ratios(t, fwd, bwd, mutant=None):
    ctx, stats = emu_as_fwd(t, mutant)
    dq, dk, dv = emu_as_bwd(t, fwd["host"], mutant)
    return dict(ctx=rb.ratio(ctx, *fwd["ctx"]), stat_max=rb.ratio(stats[..., 0], *fwd["stat_max"]), stat_rsum=rb.ratio(stats[..., 1], *fwd["stat_rsum"]),
                dq=rb.ratio(dq, *bwd["dq"]), dk=rb.ratio(dk, *bwd["dk"]), dv=rb.ratio(dv, *bwd["dv"]))


def test_attn_small_grid_covers_every_setting():
    cases = list(ab.as_cases())
    assert {(c[0], c[1]) for c in cases} == {(S, dh) for S in ab.AS_S for dh in ab.AS_DH}
    for S in ab.AS_S:
        mine = [c for c in cases if c[0] == S]
        assert {c[2] for c in mine} == set(ab.AS_DROPS) and {c[3] for c in mine} == {True, False}, S
        assert {c[4] for c in mine} == (set(ab.AS_PADS) if S > 1 else {"none"}), S


def test_attn_small_emulations_within_every_bound():
    worst = {}
    for case in ab.as_cases():
        for name, r in as_ratios(*as_case(*case)).items():
            assert r <= 1.0, f"emulation outside the bound at [{ab.as_name(*case)}] {name}: err/bound {r}"
            worst[name] = max(worst.get(name, 0.0), r)
    assert min(worst[n] for n in ("ctx", "dq", "dk", "dv")) > 0.5, f"vacuous bounds: {worst}"


AS_MUTANTS = {
    "lane_group_64": ((7, 8), "stat_rsum"),                # lane-group width 64 always and `jl < S` dropped: 57 lanes of score 0 join the row sum
    "bias_on_k_not_q": ((16, 8), "ctx"),                   # bias added to k but not to q
}


@pytest.mark.parametrize("mutant", sorted(AS_MUTANTS))
def test_attn_small_mutants_leave_the_bound_on_their_named_case(mutant):
    (S, dh), output = AS_MUTANTS[mutant]
    case = [c for c in ab.as_cases() if c[:2] == (S, dh)][0]
    if mutant == "bias_on_k_not_q":
        assert case[3], "the named case must carry biases"
    r = as_ratios(*as_case(*case), mutant)[output]
    assert r > 1.0, f"mutant '{mutant}' stays within the bound of {output} at [{ab.as_name(*case)}]: err/bound {r}"


# ------------------------------------------------------------------------------------------------------------------ records
def test_recorded_widening_factor_is_the_one_the_reference_used(monkeypatch):
    assert all(key not in rb.ACC_WIDEN for key in ab.WIDEN_KEYS), "an entry in ACC_WIDEN for an attention core must be stated in DESIGN.md; then update this line"
    case = a2_case_at(17, 17, "none")
    t = ab.a2_inputs(*case)
    base = ab.a2_fwd_ref(t)
    monkeypatch.setitem(rb.ACC_WIDEN, "attn2_fwd", 3.0)
    monkeypatch.setitem(rb.ACC_WIDEN, "attn_small_bwd", 2.0)
    assert ab.widen_of("attn2_fwd.ctx") == 3.0 and ab.widen_of("attn_small_bwd.dq") == 2.0 and ab.widen_of("attn2_bwd.dq_part") == 1.0 and ab.widen_of("attn_small_fwd.ctx") == 1.0
    wide = ab.a2_fwd_ref(t)
    # the factor sits on both accumulations of the forward, the row sum (through e_rs A) and P V: the context's bound grows by (3 - 1) times
    # 2 (Sk + 2) u A (1 + ub), A = sum_j |Pd_j v_j| (to first order in the row sum's error)
    B, H, dh = t["B"], t["H"], t["dh"]
    keep = ab.a2_keep(B * H, 17, 17, t["p"], t["seed"]).view(B, H, 17, 17)
    q, k, v = (ab.heads(t[n].double(), B, 17, H, dh) for n in ("q", "k", "v"))
    P = torch.softmax(q @ k.transpose(-1, -2) * ab.f32v(t["scale"]) * ab.LOG2E * ab.LN2, -1) * keep * ab.drop_scale(t["p"])
    A = ab.rows(P @ v.abs())
    grow = wide["ctx"][1] - base["ctx"][1]
    assert float((grow - 4 * 19 * rb.U * A * (1 + rb.UB)).abs().max()) <= 1e-3 * float(grow.max())
    assert torch.equal(wide["lse_max"][1], base["lse_max"][1])
