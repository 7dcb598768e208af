"""The bounds of tests/rounding_bounds.py are neither wrong nor vacuous: for every reference there, a torch EMULATION of the kernel's arithmetic
(fp32 operations, bf16 rounding where the kernel stores) stays within `bound` at the shapes the GPU tests use, and mutants of the emulation --
the ways such kernels go wrong -- exceed it somewhere.  Two of the mutants still pass the norm-wise check the suite had (rel < 1e-2): that is
why it was not enough.  The seeds of the GroupNorm-backward and gn_in cases leave no pre-ReLU value within the evaluation error of zero (a
condition on the INPUTS, checked here, so the ReLU mask the GPU tests compare is unambiguous)."""
import pytest
import torch

import rounding_bounds as rb
from rounding_bounds import BF, F32, F64, G

F = torch.nn.functional


# ------------------------------------------------------------------------------------------------ emulations (fp32 + bf16 where the kernel stores)
def trunc_bf16(v):
    """f32 -> bf16 by dropping the low 16 bits (the mutant store)"""
    return (v.to(F32).contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def emu_coeffs(stats, gamma, beta, HW, C, eps=rb.EPS, shift_groups=0):
    Cg = C // G
    cnt = torch.tensor(float(HW) * float(Cg), dtype=F32)
    mean = stats[..., 0] / cnt
    var = (stats[..., 1] / cnt - mean * mean).clamp(min=0)
    rs = torch.rsqrt(var + eps)
    ch = ((torch.arange(C) + shift_groups) // Cg).clamp(max=G - 1)       # shift_groups = 1: the group boundary one channel early (a mutant)
    a = rs[:, ch] * gamma
    return mean[:, ch], rs[:, ch], a, beta - mean[:, ch] * a


def emu_gn_stats(x, C, shift_groups=0):
    N, HW = x.shape[:2]
    xf = x.to(F32)
    if shift_groups:
        ch = ((torch.arange(C) + shift_groups) // (C // G)).clamp(max=G - 1)
        onehot = F.one_hot(ch, G).to(F32)
        return torch.stack([xf.sum(1) @ onehot, (xf * xf).sum(1) @ onehot], -1)
    xf = xf.reshape(N, HW, G, C // G)
    return torch.stack([xf.sum((1, 3)), (xf * xf).sum((1, 3))], -1)


def emu_gn_apply(x, stats, gamma, beta, relu, shift_groups=0):
    _, _, a, b = emu_coeffs(stats, gamma, beta, x.shape[1], x.shape[2], shift_groups=shift_groups)
    o = x.to(F32) * a.unsqueeze(1) + b.unsqueeze(1)
    return (o.clamp(min=0) if relu else o).to(BF)


def emu_gn_bwd(dy, x, stats, gamma, beta, relu, y, dg0, db0):
    N, HW, C = x.shape
    Cg = C // G
    cnt = torch.tensor(float(HW) * float(Cg), dtype=F32)
    mean, rs, a, b = emu_coeffs(stats, gamma, beta, HW, C)
    xf, d = x.to(F32), dy.to(F32)
    if relu:
        yy = y.to(F32) if y is not None else xf * a.unsqueeze(1) + b.unsqueeze(1)
        d = torch.where(yy > 0, d, torch.zeros_like(d))
    xh = (xf - mean.unsqueeze(1)) * rs.unsqueeze(1)
    grp = lambda t: t.reshape(N, HW, G, Cg).sum((1, 3))
    bstats = torch.stack([grp(d * gamma), grp(d * xh * gamma)], -1)
    ch = torch.arange(C) // Cg
    m1, m2 = (bstats[..., 0] / cnt)[:, ch].unsqueeze(1), (bstats[..., 1] / cnt)[:, ch].unsqueeze(1)
    dx = (rs.unsqueeze(1) * (d * gamma - m1 - xh * m2)).to(BF)
    return dx, bstats, dg0 + (d * xh).sum((0, 1)), db0 + d.sum((0, 1))


def conv32(x, w, dgrad=False):
    return rb.conv3x3(x.to(F32), w.to(F32), dgrad)


def emu_small(t, dgrad, mode):
    v = conv32(t["src"], t["w"], dgrad)
    if mode != "plain":
        v = v + t["shift"]
    if mode == "shift+res":
        v = v + t["res"].to(F32)
    return v.to(BF)


def emu_wgrad(t):
    dy, x = t["dy"].to(F32), t["x"].to(F32)
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return t["out0"] + torch.stack([torch.stack([torch.einsum("nhwo,nhwc->oc", dy, xp[:, r:r + H, s:s + W]) for s in range(3)], 1) for r in range(3)], 1)


def emu_stage(t, stats=None, mutant=None):
    """mask_stage_kernel in torch: GroupNorm + ReLU in f32 -> bf16 (ms_pack8v) -> upsample -> f32 convolution (+ bias, + the image's FPN term) ->
    bf16 (f32 for out_lay).  mutant: None | corner_tap | trunc_store | gn_padding | last_column | fpn_image"""
    cin, cout, gn_in, up = rb.STAGES[t["stage"]]
    Q, src = t["Q"], t["src"]
    N, SH, SW, _ = src.shape
    x = src.to(F32)
    if gn_in:
        _, _, a, b = emu_coeffs(stats if stats is not None else t["stats"], t["gamma"], t["beta"], SH * SW, cin)
        a, b = a.view(N, 1, 1, cin), b.view(N, 1, 1, cin)
        if mutant == "gn_padding":          # the halo went through GroupNorm + ReLU too: relu(b) instead of 0 around the image (and around it again after the upsample)
            x = F.pad(x, (0, 0, 1, 1, 1, 1))
        x = (x * a + b).clamp(min=0).to(BF).to(F32)
    xin = rb.up2(x) if up else x
    if mutant == "gn_padding":
        k = 2 if up else 1
        xin = xin[:, k - 1:xin.shape[1] - (k - 1), k - 1:xin.shape[2] - (k - 1)]             # one ring of normalised padding at the OUTPUT resolution
        v = F.conv2d(xin.permute(0, 3, 1, 2), t["w"].to(F32).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    else:
        v = conv32(xin, t["w"])
    if mutant == "last_column" and up:      # output column W - 1 reads source column SW - 2
        bad = xin.clone()
        bad[:, :, -1] = rb.up2(x[:, :, SW - 2:SW - 1])[:, :, 0]
        v = v.clone()
        v[:, :, -1] = conv32(bad, t["w"])[:, :, -1]
    if mutant == "corner_tap":              # 30 % of the centre tap at pixel (0, 0) of every map goes missing
        v = v.clone()
        v[:, 0, 0] -= 0.3 * torch.einsum("oc,nc->no", t["w"].to(F32)[:, 1, 1], xin[:, 0, 0])
    if t["bias"] is not None:
        v = v + t["bias"]
    if up:
        img = torch.arange(N) // Q
        if mutant == "fpn_image":
            img = ((torch.arange(N) + 1) // Q).clamp(max=N // Q - 1)
        v = v + t["fpn_conv"].to(F32)[img]
    if cout == 1:
        return v
    return trunc_bf16(v) if mutant == "trunc_store" else v.to(BF)


def emu_attn_fwd(t, store=lambda v: v.to(BF)):
    B, Q, H, HW = t["B"], t["Q"], t["H"], t["HW"]
    s = t["scores"].to(F32)[..., :HW]
    if t["key_pad"] is not None:
        s = s.masked_fill(t["key_pad"].bool()[:, None, None, :], float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e * (1.0 / e.sum(-1, keepdim=True))
    return store(p.reshape(B * Q, H, HW).permute(0, 2, 1).contiguous())


def emu_attn_bwd(prob, dprob, ld):
    P, dP = prob.to(F32).permute(0, 2, 1), dprob.to(F32).permute(0, 2, 1)
    ds = (P * (dP - (P * dP).sum(-1, keepdim=True))).to(BF)
    return F.pad(ds, (0, ld - P.shape[-1]))


def within(got, ref, bound):
    r = rb.ratio(got, ref, bound)
    assert r <= 1.0, r
    return r


# ------------------------------------------------------------------------------------------------ the emulations are within the bounds
@pytest.mark.parametrize("stage", list(rb.STAGES))
def test_stage_emulation_within_bound_and_relu_unambiguous(stage):
    worst = 0.0
    for H, W in rb.STAGE_SHAPES[stage]:
        t = rb.stage_inputs(stage, H, W)
        ref, bound, info = rb.mask_stage_ref(t)
        assert info["n_ambiguous"] == 0, (stage, H, W, info)           # the condition on the seeds
        got = emu_stage(t)
        worst = max(worst, within(got.reshape(ref.shape), ref, bound))
        if rb.STAGES[stage][1] != 1:
            sref, sbound = rb.stage_stats_ref(got)
            o = got.to(F32).reshape(got.shape[0], H * W, G, -1)
            within(torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1), sref, sbound)
    if rb.STAGES[stage][1] != 1:     # not vacuous: with a bf16 output the correct emulation uses most of the bound (out_lay's f32 output has the
        assert worst > 0.5, worst    # worst-case accumulation term alone, which random rounding errors do not approach; its mutants are below)
    print(stage, "clean emulation peaks at", round(worst, 3), "of the bound")


def test_stage_bound_marks_few_inputs_flippable():
    """the shape of the issue: lay5, N = 6, 18 x 34"""
    _, _, info = rb.mask_stage_ref(rb.stage_inputs("lay5", 18, 34))
    assert info["flippable"] < 0.01 and info["zero_flip_outputs"] > 0.5, info


MUTANTS = ["corner_tap", "trunc_store", "gn_padding", "last_column", "fpn_image"]


@pytest.mark.parametrize("stage,mutant", [("lay5", m) for m in MUTANTS] + [("out_lay", "corner_tap"), ("out_lay", "gn_padding"), ("lay4", "last_column"), ("lay4", "fpn_image")])
def test_stage_mutants_exceed_the_bound(stage, mutant):
    t = rb.stage_inputs(stage, *rb.STAGE_SHAPES[stage][2])            # lay5: the 18 x 34 case, N = 6
    ref, bound, _ = rb.mask_stage_ref(t)
    got = emu_stage(t, mutant=mutant)
    r = rb.ratio(got.reshape(ref.shape), ref, bound)
    assert r > 1.0, (mutant, r)
    if stage == "lay5" and mutant in ("corner_tap", "trunc_store"):
        assert rb.rel(got, ref) < 1e-2, rb.rel(got, ref)       # the norm-wise check the suite had does not see these two
    print(mutant, "exceeds the bound by x", round(r, 2), "rel-Frobenius", rb.rel(got, ref))


@pytest.mark.parametrize("C", rb.GN_C)
def test_groupnorm_emulation_within_bound(C):
    for HW in rb.GN_HW:
        t = rb.gn_inputs(C, HW)
        x, gamma, beta = t["x"], t["gamma"], t["beta"]
        stats = emu_gn_stats(x, C)
        within(stats, *rb.gn_stats_ref(x, C))
        for relu in (True, False):
            y = emu_gn_apply(x, stats, gamma, beta, relu)
            yref, ybound, (v, delta) = rb.gn_apply_ref(x, stats, gamma, beta, relu)
            within(y, yref, ybound)
            assert int((v.abs() <= 2 * delta).sum()) == 0, (C, HW)      # the seed's condition, with a factor 2 to spare for the device's own statistics
            for with_y in (True, False):
                dx, bst, dg, db = emu_gn_bwd(t["dy"], x, stats, gamma, beta, relu, y if with_y else None, t["dg0"], t["db0"])
                r = rb.gn_bwd_ref(t["dy"], x, stats, gamma, beta, relu, y=y if (with_y and relu) else None, bstats=bst, dgamma0=t["dg0"], dbeta0=t["db0"])
                assert r["n_flip"] == 0
                within(dx, *r["dx"]), within(bst, *r["bstats"]), within(dg, *r["dgamma"]), within(db, *r["dbeta"])


def test_groupnorm_offset_case_against_true_groupnorm():
    t = rb.gn_inputs(64, 513, offset=4.0)
    stats = emu_gn_stats(t["x"], 64)
    y = emu_gn_apply(t["x"], stats, t["gamma"], t["beta"], True)
    within(y, *rb.gn_true_ref(t["x"], t["gamma"], t["beta"], True))


def test_groupnorm_group_boundary_mutant_is_caught_at_264():
    """C = 264: groups of 33 channels, so an 8-channel chunk spans two groups; the mutant puts the boundary one channel early"""
    t = rb.gn_inputs(264, 130)
    x = t["x"]
    good = emu_gn_stats(x, 264)
    bad = emu_gn_stats(x, 264, shift_groups=1)
    ref, bound = rb.gn_stats_ref(x, 264)
    assert rb.ratio(good, ref, bound) <= 1.0 and rb.ratio(bad, ref, bound) > 1.0
    y = emu_gn_apply(x, good, t["gamma"], t["beta"], True, shift_groups=1)
    yref, ybound, _ = rb.gn_apply_ref(x, good, t["gamma"], t["beta"], True)
    assert rb.ratio(y, yref, ybound) > 1.0


@pytest.mark.parametrize("dgrad", [False, True])
def test_small_conv_emulation_within_bound(dgrad):
    for shape in rb.SMALL_SHAPES:
        for cs, co in (rb.SMALL_DGRAD if dgrad else rb.SMALL_FWD):
            t = rb.small_inputs(shape, cs, co, dgrad)
            for mode in ("shift+res", "shift", "plain"):
                ref, bound = rb.small_conv_ref(t["src"], t["w"], t["shift"] if mode != "plain" else None, t["res"] if mode == "shift+res" else None, dgrad)
                within(emu_small(t, dgrad, mode), ref, bound)
    # the 16-pixel groups are flat: a tap that follows the flat index across a row end (pixel p - 1 of the next row's first pixel) is caught
    t = rb.small_inputs((2, 3, 5), 32, 16, False)
    ref, bound = rb.small_conv_ref(t["src"], t["w"], None, None, False)
    src, w = t["src"].to(F32), t["w"].to(F32)
    leak = conv32(t["src"], t["w"])
    leak[:, 1:, 0] += torch.einsum("oc,nhc->nho", w[:, 1, 0], src[:, :-1, -1])
    assert rb.ratio(leak.to(BF), ref, bound) > 1.0


def test_wgrad_emulation_within_bound():
    for shape in rb.WGRAD_SHAPES:
        for C, Co in rb.WGRAD_CH:
            t = rb.wgrad_inputs(shape, C, Co)
            within(emu_wgrad(t), *rb.wgrad_ref(t["dy"], t["x"], t["out0"]))
    t = rb.wgrad_inputs((2, 3, 5), 16, 8)
    ref, bound = rb.wgrad_ref(t["dy"], t["x"], t["out0"])
    assert rb.ratio(emu_wgrad(t) + 1e-4 * t["out0"], ref, bound) > 1.0      # an idle workgroup's partial that is not quite nothing


def test_resample_and_sum_emulations_within_bound():
    for H, W in rb.UPS_HW:
        for C in rb.UPS_C:
            t = rb.ups_inputs(H, W, C)
            ref, bound = rb.upsample_add_ref(t["inp"], t["fpn"], 3)
            got = (rb.up2(t["inp"].to(F32)) + t["fpn"].to(F32).repeat_interleave(3, 0)).to(BF)
            assert torch.equal(got.to(F64), ref) and float(bound.max()) == 0.0
            wrong = (rb.up2(t["inp"].to(F32)) + t["fpn"].to(F32)[(torch.arange(6) + 1) // 3 % 2]).to(BF)     # the FPN term of image (n + 1) / Q
            assert not torch.equal(wrong.to(F64), ref)
            d = t["dout"].to(F32)
            within(d.reshape(6, H, 2, W, 2, C).sum((2, 4)).to(BF), *rb.upsample_add_bwd_ref(t["dout"]))
            for Q in rb.SUMQ_Q:
                g = torch.Generator().manual_seed(Q + C + H)
                x = torch.randn(2 * Q, H * W * C, generator=g).to(BF)
                acc = torch.zeros(2, H * W * C)
                for q in range(Q):                                       # the kernel's order: one query after the other
                    acc = acc + x.to(F32).reshape(2, Q, -1)[:, q]
                within(acc.to(BF), *rb.sum_queries_ref(x, 2, Q))
                if Q == 100:
                    assert rb.ratio(trunc_bf16(acc), *rb.sum_queries_ref(x, 2, Q)) > 1.0


def test_attnmap_emulation_within_bound():
    for HW in rb.ATT_HW:
        for extra in (0, 8):
            for pad in rb.ATT_PADS:
                t = rb.attnmap_inputs(HW, extra, pad)
                p = emu_attn_fwd(t)
                ref, bound = rb.attnmap_fwd_ref(t)
                within(p, ref, bound)
                if t["key_pad"] is not None:
                    assert float(p.to(F32)[t["key_pad"].bool().repeat_interleave(t["Q"], 0)].abs().max()) == 0.0
                ds = emu_attn_bwd(p, t["dprob"], t["ld"])
                within(ds, *rb.attnmap_bwd_ref(p, t["dprob"], t["ld"]))
    t = rb.attnmap_inputs(130, 0, "middle")
    ref, bound = rb.attnmap_fwd_ref(t)
    assert rb.ratio(emu_attn_fwd(t, store=trunc_bf16), ref, bound) > 1.0


def test_tail_storage_floor_is_measured_not_asserted():
    """lay4 -> gn4 -> lay5 -> gn5 -> out_lay at B = 1, Q = 4, 40 x 40 logits, chained through the references twice: with bf16 rounding at the
    kernels' storage points, and with none.  The worst |delta| - 5e-2 |ref| is the storage floor of the TAIL alone at a small map count, the
    figure DESIGN.md section 5 sets against the 0.097 measured end to end at B = 8.  No threshold: this is a measurement."""
    B, Q = 1, 4
    t4, t5, t6 = rb.stage_inputs("lay4", 20, 20, B, Q, seed=41), rb.stage_inputs("lay5", 40, 40, B, Q, seed=42), rb.stage_inputs("out_lay", 40, 40, B, Q, seed=43)

    def chain(rounding):
        st = lambda o: rb.gn_stats_ref(o.reshape(o.shape[0], -1, o.shape[-1]), o.shape[-1])[0]
        rnd = rb.round_bf16 if rounding else (lambda v: v)
        o4 = rnd(rb.mask_stage_ref(t4, rounding=rounding)[0])
        o5 = rnd(rb.mask_stage_ref(t5, stats=st(o4), rounding=rounding, src64=o4)[0])
        return rb.mask_stage_ref(t6, stats=st(o5), rounding=rounding, src64=o5)[0]
    a, b = chain(True), chain(False)
    d = (a - b).abs()
    excess = float((d - 5e-2 * b.abs()).max())
    print("tail storage floor: max |delta|", float(d.max()), "worst |delta| - 5e-2 |ref|", excess, "max |ref|", float(b.abs().max()))
    assert excess == excess
