"""The mask head's kernels (csrc/maskstage.hip, csrc/smallconv.hip, csrc/segm.hip), called directly through toist_amd.kernels, against the
fp64 references of tests/rounding_bounds.py: EVERY output element within the derived bound (storage + accumulation + flippable-input terms,
none tuned; tests/test_cpu_mask_head_bounds.py shows they hold for a correct implementation and catch the usual mistakes), at the smallest
shapes that reach every branch: a single pixel, exactly one tile / pixel group, partial last tiles in both directions, strips of three and
five tiles (both LDS buffers reused), pixel groups that span rows and images, GroupNorm chunks that span two groups (C = 264).  Every output
sits between sentinel guards that must stay untouched.  The largest err / bound of each case goes to mask_head_kernel_parity.json (rounding_bounds.RECORD)
before it is asserted (committed as profiles/mask_head_kernel_parity.json)."""
import pytest
import torch

import rounding_bounds as rb
from rounding_bounds import BF, F32, F64, G  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
PAD = 1024


def _guarded(shape, dtype, dev, fill=None):
    """a tensor of `shape` with PAD sentinel elements before and after it; fill: initial contents (a CPU tensor) or None (sentinels, to be overwritten)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=dev)
    view = buf[PAD:PAD + n].view(shape)
    if fill is not None:
        view.copy_(fill.to(dtype))
    return buf, view


def _guards_untouched(*bufs):
    for buf in bufs:
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), "guard elements were written"


def _dev(t, dev):
    return None if t is None else t.to(dev)


# ------------------------------------------------------------------------------------------------------------------ mask_stage_fwd
def _run_stage(t, dev, stats_from_kernel=False):
    from toist_amd import kernels as k
    cin, cout, gn_in, up = rb.STAGES[t["stage"]]
    H, W, Q = t["H"], t["W"], t["Q"]
    src = t["src"].to(dev)
    N, SH, SW, _ = src.shape
    stats = None
    if gn_in:
        if stats_from_kernel:        # the product path: statistics only, the consumer normalises on the way in
            stats = torch.empty(N, G, 2, dtype=F32, device=dev)
            k.groupnorm_fwd(src, t["gamma"].to(dev), t["beta"].to(dev), N, SH * SW, cin, G, rb.EPS, True, None, stats)
        else:
            stats = t["stats"].to(dev)
    if cout == 1:
        obuf, out = _guarded((N, H, W), F32, dev)
        sbuf = st = None
    else:
        obuf, out = _guarded((N, H, W, cout), BF, dev)
        sbuf, st = _guarded((N, G, 2), F32, dev)
    k.mask_stage_fwd(src, stats, _dev(t["gamma"], dev), _dev(t["beta"], dev), _dev(t["fpn_conv"], dev), t["w"].to(dev), _dev(t["bias"], dev), out, st,
                     N, Q, H, W, cin, cout, cout, gn_in, up)
    torch.cuda.synchronize()
    return out.cpu(), None if st is None else st.cpu(), None if stats is None else stats.cpu(), [b for b in (obuf, sbuf) if b is not None]


def _check_stage(t, dev, case, stats_from_kernel=False):
    out, st, stats, bufs = _run_stage(t, dev, stats_from_kernel)
    ref, bound, _ = rb.mask_stage_ref(t, stats=stats)
    r = rb.record("mask_stage_fwd." + t["stage"], case, rb.ratio(out.reshape(ref.shape), ref, bound))
    rs = 0.0
    if st is not None:
        rs = rb.record("mask_stage_fwd." + t["stage"] + ".out_stats", case, rb.ratio(st, *rb.stage_stats_ref(out)))
    _guards_untouched(*bufs)
    assert r <= 1.0 and rs <= 1.0, (case, r, rs)


@pytest.mark.parametrize("stage,H,W", [(s, h, w) for s in rb.STAGES for h, w in rb.STAGE_SHAPES[s]], ids=lambda v: str(v))
def test_mask_stage_elementwise(dev, stage, H, W):
    """N = 6 maps of B = 2 images (Q = 3: the FPN term of image n // Q), a different fpn_conv per image; gn_in statistics from the host (fp64 sums
    handed over as f32), so the stage stands apart from the statistics pass"""
    _check_stage(rb.stage_inputs(stage, H, W), dev, f"{H}x{W} host stats")


@pytest.mark.parametrize("stage", ["lay5", "out_lay"])
def test_mask_stage_with_the_statistics_pass(dev, stage):
    """as the product runs it: groupnorm_fwd(y=None) statistics of the source, then the stage; the reference starts from those statistics"""
    H, W = rb.STAGE_SHAPES[stage][2]
    t = rb.stage_inputs(stage, H, W)
    _check_stage(t, dev, f"{H}x{W} groupnorm_fwd stats", stats_from_kernel=True)


# ------------------------------------------------------------------------------------------------------------------ conv3x3_small / wgrad3x3_small
@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("shape", rb.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_small_elementwise(dev, shape, dgrad):
    from toist_amd import kernels as k
    n, H, W = shape
    worst = {}
    for cs, co in (rb.SMALL_DGRAD if dgrad else rb.SMALL_FWD):
        t = rb.small_inputs(shape, cs, co, dgrad)
        for mode in ("shift+res", "shift", "plain"):
            shift = t["shift"] if mode != "plain" else None
            res = t["res"] if mode == "shift+res" else None
            obuf, out = _guarded((n, H, W, co), BF, dev)
            k.conv3x3_small(dgrad, t["src"].to(dev), t["w"].to(dev), _dev(shift, dev), _dev(res, dev), out, n, H, W, cs, co)
            torch.cuda.synchronize()
            case = f"{'dgrad' if dgrad else 'fwd'} {n}x{H}x{W} {cs}->{co} {mode}"
            worst[case] = rb.record("conv3x3_small", case, rb.ratio(out, *rb.small_conv_ref(t["src"], t["w"], shift, res, dgrad)))
            _guards_untouched(obuf)
    bad = {c: r for c, r in worst.items() if not r <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("shape", rb.WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad3x3_small_elementwise(dev, shape):
    """accumulate=True onto a non-zero gradient: the partials of idle workgroups (512 are launched, a few have pixels) must add nothing"""
    from toist_amd import kernels as k
    worst = {}
    for C, Co in rb.WGRAD_CH:
        t = rb.wgrad_inputs(shape, C, Co)
        obuf, out = _guarded((Co, 3, 3, C), F32, dev, fill=t["out0"])
        k.wgrad3x3_small(t["dy"].to(dev), t["x"].to(dev), out, accumulate=True)
        torch.cuda.synchronize()
        case = f"{'x'.join(map(str, shape))} C{C} Co{Co}"
        worst[case] = rb.record("wgrad3x3_small", case, rb.ratio(out, *rb.wgrad_ref(t["dy"], t["x"], t["out0"])))
        _guards_untouched(obuf)
    bad = {c: r for c, r in worst.items() if not r <= 1.0}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("HW", rb.GN_HW)
@pytest.mark.parametrize("C", rb.GN_C)
def test_groupnorm_elementwise(dev, C, HW):
    """N = 3, G = 8.  Statistics against fp64 sums; y (groupnorm_fwd and groupnorm_apply), dx element-wise against the fp64 formula evaluated from
    the kernel's OWN statistics; bstats / dgamma / dbeta (accumulated onto non-zero values) against fp64 sums.  ReLU on and off, backward with y
    and with y = None + beta (the mask re-derived from x)."""
    from toist_amd import kernels as k
    t = rb.gn_inputs(C, HW)
    N = t["x"].shape[0]
    x, dy, gamma, beta = (t[n].to(dev) for n in ("x", "dy", "gamma", "beta"))
    worst = {}

    def note(kernel, case, r):
        worst[kernel + " " + case] = rb.record(kernel, f"C{C} HW{HW} {case}", r)
    for relu in (True, False):
        tag = "relu" if relu else "linear"
        ybuf, y = _guarded((N, HW, C), BF, dev)
        sbuf, stats = _guarded((N, G, 2), F32, dev)
        k.groupnorm_fwd(x, gamma, beta, N, HW, C, G, rb.EPS, relu, y, stats)
        y2buf, y2 = _guarded((N, HW, C), BF, dev)
        k.groupnorm_apply(x, stats, gamma, beta, N, HW, C, G, rb.EPS, relu, y2)
        torch.cuda.synchronize()
        st = stats.cpu()
        note("groupnorm_fwd.stats", tag, rb.ratio(st, *rb.gn_stats_ref(t["x"], C)))
        yref, ybound, _ = rb.gn_apply_ref(t["x"], st, t["gamma"], t["beta"], relu)
        note("groupnorm_fwd.y", tag, rb.ratio(y, yref, ybound))
        note("groupnorm_apply", tag, rb.ratio(y2, yref, ybound))
        assert torch.equal(y, y2)
        _guards_untouched(ybuf, sbuf, y2buf)
        for with_y in (True, False):
            dxbuf, dx = _guarded((N, HW, C), BF, dev)
            gbuf, dg = _guarded((C,), F32, dev, fill=t["dg0"])
            bbuf, db = _guarded((C,), F32, dev, fill=t["db0"])
            bsbuf, bst = _guarded((N, G, 2), F32, dev)
            k.groupnorm_bwd(dy, y if with_y else None, x, stats, gamma, N, HW, C, G, rb.EPS, relu, dx, dg, db, bst, beta=None if with_y else beta)
            torch.cuda.synchronize()
            r = rb.gn_bwd_ref(t["dy"], t["x"], st, t["gamma"], t["beta"], relu, y=y.cpu() if (with_y and relu) else None, bstats=bst.cpu(),
                              dgamma0=t["dg0"], dbeta0=t["db0"])
            sub = tag + (" with y" if with_y else " y=None+beta")
            for name, got in (("dx", dx), ("bstats", bst), ("dgamma", dg), ("dbeta", db)):
                note("groupnorm_bwd." + name, sub, rb.ratio(got, *r[name]))
            _guards_untouched(dxbuf, gbuf, bbuf, bsbuf)
    bad = {c: r for c, r in worst.items() if not r <= 1.0}
    assert not bad, bad


def test_groupnorm_offset_input_against_true_groupnorm(dev):
    """mean ~ 4 std: E[x^2] - mean^2 cancels.  y against the TRUE fp64 GroupNorm of x alone, the statistics bounds propagated through dy/dmean, dy/dvar"""
    from toist_amd import kernels as k
    C, HW = 64, 513
    t = rb.gn_inputs(C, HW, offset=4.0)
    N = t["x"].shape[0]
    ybuf, y = _guarded((N, HW, C), BF, dev)
    stats = torch.empty(N, G, 2, dtype=F32, device=dev)
    k.groupnorm_fwd(t["x"].to(dev), t["gamma"].to(dev), t["beta"].to(dev), N, HW, C, G, rb.EPS, True, y, stats)
    torch.cuda.synchronize()
    rs = rb.record("groupnorm_fwd.stats", "offset C64 HW513", rb.ratio(stats, *rb.gn_stats_ref(t["x"], C)))
    ry = rb.record("groupnorm_fwd.y vs true GroupNorm", "offset C64 HW513", rb.ratio(y, *rb.gn_true_ref(t["x"], t["gamma"], t["beta"], True)))
    _guards_untouched(ybuf)
    assert rs <= 1.0 and ry <= 1.0, (rs, ry)


# ------------------------------------------------------------------------------------------------------------------ upsample_add / _bwd / sum_queries
@pytest.mark.parametrize("C", rb.UPS_C)
@pytest.mark.parametrize("H,W", rb.UPS_HW)
def test_upsample_add_and_its_backward(dev, H, W, C):
    from toist_amd import kernels as k
    BQ, Q = 6, 3
    t = rb.ups_inputs(H, W, C, BQ, Q)
    obuf, out = _guarded((BQ, 2 * H, 2 * W, C), BF, dev)
    k.upsample_add(t["inp"].to(dev), t["fpn"].to(dev), BQ, Q, H, W, C, out)
    dbuf, din = _guarded((BQ, H, W, C), BF, dev)
    k.upsample_add_bwd(t["dout"].to(dev), BQ, H, W, C, din)
    torch.cuda.synchronize()
    ref, _ = rb.upsample_add_ref(t["inp"], t["fpn"], Q)
    exact = torch.equal(out.cpu().to(F64), ref)                  # one add and one rounding: bit for bit
    rb.record("upsample_add", f"{H}x{W} C{C}", 0.0 if exact else float("inf"))
    rbwd = rb.record("upsample_add_bwd", f"{H}x{W} C{C}", rb.ratio(din, *rb.upsample_add_bwd_ref(t["dout"])))
    _guards_untouched(obuf, dbuf)
    assert exact, f"{int((out.cpu().to(F64) != ref).sum())} of {ref.numel()} elements differ"
    assert rbwd <= 1.0, rbwd


@pytest.mark.parametrize("Q", rb.SUMQ_Q)
@pytest.mark.parametrize("C", rb.UPS_C)
def test_sum_queries(dev, C, Q):
    from toist_amd import kernels as k
    B = 2
    worst = {}
    for H, W in rb.UPS_HW:
        g = torch.Generator().manual_seed(1000 * Q + 10 * C + H)
        x = torch.randn(B * Q, H, W, C, generator=g).to(BF)
        obuf, out = _guarded((B, H * W * C), BF, dev)
        k.sum_queries(x.to(dev), B, Q, H * W * C, out)
        torch.cuda.synchronize()
        worst[(H, W)] = rb.record("sum_queries", f"Q{Q} {H}x{W} C{C}", rb.ratio(out, *rb.sum_queries_ref(x, B, Q)))
        _guards_untouched(obuf)
    bad = {c: r for c, r in worst.items() if not r <= 1.0}
    assert not bad, bad
