"""The row kernels (csrc/rows.hip: LayerNorm, masked softmax, column sum, add, dropout, the RoBERTa embedding) and the two l2norm launches of
csrc/contrastive.hip, called directly through toist_amd.kernels, against the fp64 references of tests/row_bounds.py: EVERY output element
within the derived bound (or bit for bit where the operation is one rounding), at the smallest shapes that reach every path -- one live lane,
the register-chunk boundaries (LayerNorm 512 / 520, softmax 512 / 513 and the evaluation's 1066 keys), grids at their caps, the scalar and tail
paths of colsum, the stride loops of add and dropout.  tests/test_cpu_row_bounds.py shows that the bounds hold for a correct implementation and
catch the usual mistakes.  Outputs the kernel overwrites start as NaN, outputs it accumulates onto start non-zero.  The largest err / bound of
each case goes to row_kernel_parity.json (row_bounds.record) before it is asserted (committed as profiles/row_kernel_parity.json)."""
import pytest
import torch

import row_bounds as rw
from oracle import xdec_ref as xr
from rounding_bounds import BF, F32

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def k():
    """toist_amd.kernels with no device seed word (process-wide), restored afterwards"""
    from toist_amd import kernels
    seed_dev = kernels.SEED_DEV
    kernels.SEED_DEV = None
    yield kernels
    kernels.SEED_DEV = seed_dev


def nan_like(shape, dtype, dev):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_forward(k, dev, t, eps, with_add, with_stats):
    rows, D = t["x"].shape
    x, gamma, beta = t["x"].to(dev), t["gamma"].to(dev), t["beta"].to(dev)
    y = nan_like((rows, D), BF, dev)
    mean = nan_like((rows,), F32, dev) if with_stats else None
    rstd = nan_like((rows,), F32, dev) if with_stats else None
    y2 = nan_like((rows, D), BF, dev) if with_add else None
    k.layernorm_fwd(x, gamma, beta, eps, y, mean, rstd, t["add"].to(dev) if with_add else None, y2)
    torch.cuda.synchronize()
    return y, mean, rstd, y2


def _ln_check_forward(k, dev, t, eps, case):
    ref = rw.ln_fwd_ref(t["x"], t["gamma"], t["beta"], eps)
    y, mean, rstd, y2 = _ln_forward(k, dev, t, eps, True, True)
    rw.check("layernorm_fwd.mean", case, mean, *ref["mean"])
    rw.check("layernorm_fwd.rstd", case, rstd, *ref["rstd"])
    rw.check("layernorm_fwd.y", case, y, *ref["y"])
    rw.check_exact("layernorm_fwd.y2", case, y2, rw.ln_y2_ref(y.cpu(), t["add"]))
    yb, _, _, _ = _ln_forward(k, dev, t, eps, False, False)            # without add / y2 and with mean / rstd null: the same y
    rw.check_exact("layernorm_fwd.y (no stats, no y2)", case, yb, y.cpu())
    return mean, rstd


def _ln_check_backward(k, dev, t, mean, rstd, case, defer, drop=False):
    rows, D = t["x"].shape
    dx = nan_like((rows, D), BF, dev)
    dg, db = t["dg0"].to(dev), t["db0"].to(dev)
    p, seed = rw.LN_DROP[2:]
    dxd = nan_like((rows, D), BF, dev) if drop else None
    k.layernorm_bwd(t["dy"].to(dev), t["x"].to(dev), mean, rstd, t["gamma"].to(dev), dx, dg, db, dx_drop=dxd, drop_p=p if drop else 0.0, seed=seed, defer=defer)
    if defer:
        assert k.LN_DEFER, "the deferred cases need the partial-sum path (TOIST_LN_DEFER on); with it off they would re-run the atomic one"
        k.flush_reductions()
    torch.cuda.synchronize()
    ref = rw.ln_bwd_ref(t["dy"], t["x"], mean.cpu(), rstd.cpu(), t["gamma"], t["dg0"], t["db0"], keep=xr.elem_keep(rows, D, p, seed) if drop else None, p=p)
    tag = "deferred" if defer else "atomic"
    rw.check("layernorm_bwd.dx", f"{case} {tag}", dx, *ref["dx"])
    rw.check(f"layernorm_bwd.dgamma ({tag})", case, dg, *ref["dgamma"])
    rw.check(f"layernorm_bwd.dbeta ({tag})", case, db, *ref["dbeta"])
    if drop:
        rw.check("layernorm_bwd.dx_drop", case, dxd, *ref["dx_drop"])


@pytest.mark.parametrize("D", rw.LN_D)
def test_layernorm_every_element(dev, k, D):
    """mean, rstd, y, y2 and the y of the call without add / y2 / mean / rstd; then dx, dgamma, dbeta from the kernel's own statistics, on both
    parameter-gradient paths, onto non-zero contents"""
    for rows in rw.LN_ROWS:
        t = rw.ln_inputs(rows, D)
        for eps in rw.LN_EPS:
            case = f"{rows}x{D} eps={eps:g}"
            mean, rstd = _ln_check_forward(k, dev, t, eps, case)
            for defer in (False, True):
                _ln_check_backward(k, dev, t, mean, rstd, case, defer, drop=((rows, eps) == rw.LN_DROP[:2] and not defer))


@pytest.mark.parametrize("rows,D", rw.LN_BIG)
def test_layernorm_grids_at_their_caps(dev, k, rows, D):
    """2051 rows: the atomic grid is capped at 128 blocks (512 waves, 4 or 5 rows each); 4099 rows: the deferred grid at 512 blocks"""
    t = rw.ln_inputs(rows, D)
    mean, rstd = _ln_check_forward(k, dev, t, 1e-5, f"{rows}x{D}")
    for defer in (False, True):
        _ln_check_backward(k, dev, t, mean, rstd, f"{rows}x{D}", defer)


def test_layernorm_offset_rows(dev, k):
    """x = randn + 4: |mean| ~ 4 std; the two-pass variance has nothing to cancel, so the same bound holds"""
    t = rw.ln_inputs(17, 520, offset=4.0)
    mean, rstd = _ln_check_forward(k, dev, t, 1e-5, "17x520 offset 4")
    _ln_check_backward(k, dev, t, mean, rstd, "17x520 offset 4", False)


@pytest.mark.parametrize("D", [8, 520, 768])
def test_layernorm_constant_row_gives_beta_exactly(dev, k, D):
    """a constant row: the sum of D equal bf16 values and its division by D are exact, so x - mean = 0 and y = bf16(beta) whatever eps is"""
    t = rw.ln_inputs(5, D)
    t["x"][1] = 2.75
    t["x"][3] = -0.0123                        # rounds to a bf16 value: still D equal terms
    for eps in rw.LN_EPS:
        y, mean, rstd, _ = _ln_forward(k, dev, t, eps, False, True)
        want = t["beta"].to(BF).expand(2, D)
        rw.check_exact("layernorm_fwd.y constant row", f"5x{D} eps={eps:g}", y[[1, 3]], want)
        assert torch.equal(mean[[1, 3]].cpu(), t["x"][[1, 3], 0].float())


# ------------------------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("Sk", rw.SM_SK)
def test_softmax_every_element(dev, k, Sk):
    """forward: every live probability within storage + the evaluation term, dead keys and pad columns exactly 0 although the pad columns of the
    input hold 1e4; backward from the device's probabilities, whose pad columns (and dp's) are overwritten with garbage first: they are ignored"""
    for ld in rw.sm_lds(Sk):
        for pad in rw.sm_pads(Sk):
            t = rw.sm_inputs(Sk, ld, pad)
            case = f"Sk={Sk} ld={ld} pad={pad}"
            p = nan_like((t["rows"], ld), BF, dev)
            k.softmax_fwd(t["scores"].to(dev), None if t["key_pad"] is None else t["key_pad"].to(dev), rw.SM_NB, rw.SM_H, rw.SM_SQ, Sk, ld, p)
            torch.cuda.synchronize()
            rw.check("softmax_fwd", case, p, *rw.sm_fwd_ref(t))
            pin = p.clone()
            pin[:, Sk:] = 0.25
            ds = nan_like((t["rows"], ld), BF, dev)
            k.softmax_bwd(pin, t["dp"].to(dev), t["rows"], Sk, ld, ds)
            torch.cuda.synchronize()
            rw.check("softmax_bwd", case, ds, *rw.sm_bwd_ref(pin.cpu(), t["dp"], Sk))


# ------------------------------------------------------------------------------------------------------------------ colsum
def _colsum(k, dev, M, N, kind):
    store, view, ld, out0 = rw.cs_inputs(M, N, kind)
    sd = store.to(dev)
    gd = sd[:, 1:] if kind == "unaligned" else sd
    assert (gd.data_ptr() % 16 != 0) == (kind == "unaligned")
    out = out0.to(dev)
    k.colsum(gd, M, N, ld, out)
    torch.cuda.synchronize()
    return out, view, out0


@pytest.mark.parametrize("M", rw.CS_M)
def test_colsum_generic_every_path(dev, k, M):
    """the vector path, the column tail (n + 8 > N), a row pitch that is no multiple of 8 and an unaligned base (both the scalar path), onto non-zero out"""
    for N in rw.CS_N:
        for kind in rw.CS_LD:
            out, view, out0 = _colsum(k, dev, M, N, kind)
            rw.check("colsum", f"{M}x{N} ld={kind}", out, *rw.colsum_ref(view, out0))


@pytest.mark.parametrize("M", rw.CS_NARROW_M)
def test_colsum_narrow_every_width(dev, k, M):
    """sparse tall inputs (row_bounds.cs_inputs): the bound is below 0.5 and every value at least 1, so a row lost from the ragged last pass, from the
    last block of 37 rows or from either end of an 8192-row block leaves it"""
    for N in rw.CS_NARROW_N:
        out, view, out0 = _colsum(k, dev, M, N, "N")
        rw.check("colsum (narrow)", f"{M}x{N}", out, *rw.colsum_ref(view, out0))


def test_colsum_24_columns_take_the_generic_kernel(dev, k):
    """N = 24 at M = 32768: 3 chunks per row do not divide 256, so the dispatcher keeps the generic kernel.  The result is held to the bound, and is
    bit for bit that of the generic kernel on the same values at a pitch of 32, which never qualifies for the narrow one (the tall inputs of
    row_bounds.cs_inputs sum exactly in f32, so the order of the atomics does not show).  Which kernel ran cannot be seen from outside: this test
    holds what the dispatch must GIVE."""
    M, N = 32768, 24
    out, view, out0 = _colsum(k, dev, M, N, "N")
    rw.check("colsum", f"{M}x{N} ld=N", out, *rw.colsum_ref(view, out0))
    wide = torch.zeros(M, 32, dtype=BF)
    wide[:, :N] = view
    other = out0.to(dev)
    k.colsum(wide.to(dev), M, N, 32, other)
    rw.check_exact("colsum", f"{M}x{N} ld=N equals ld=32", out, other)


# ------------------------------------------------------------------------------------------------------------------ add / dropout
def test_add_plain_broadcast_in_place_and_strided(dev, k):
    for n, period in rw.ADD_CASES:
        a, b = rw.add_inputs(n, period)
        want = rw.add_ref(a, b, period)
        ad, bd = a.to(dev), b.to(dev)
        out = nan_like((n,), BF, dev)
        k.add(ad, bd, out, b_period=period)
        rw.check_exact("add", f"n={n} period={period}", out, want)
        k.add(ad, bd, ad, b_period=period)                             # in place, as engine.py's residual adds run it
        rw.check_exact("add (in place)", f"n={n} period={period}", ad, want)


@pytest.mark.parametrize("p", rw.DROP_P)
@pytest.mark.parametrize("n", rw.DROP_N)
def test_dropout_every_element(dev, k, n, p):
    x, seed = rw.drop_inputs(n, p)
    out = nan_like((n,), BF, dev)
    k.dropout(x.to(dev), p, seed, out)
    rw.check_exact("dropout", f"n={n} p={p}", out, rw.dropout_ref(x, xr.elem_keep(1, n, p, seed).view(-1), p))


# ------------------------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("D", rw.EMB_D)
def test_embed_fwd_bit_exact(dev, k, D):
    for B, L in rw.EMB_BL:
        t = rw.emb_inputs(B, L, D)
        ids = t["ids"].to(dev)
        pos_ids, _ = k.text_prep(ids, t["att"].to(dev), rw.PAD_ID)
        assert torch.equal(pos_ids.cpu(), rw.position_ids(t["ids"]))
        out = nan_like((B * L, D), BF, dev)
        k.embed_fwd(ids.view(-1), pos_ids.view(-1), t["word"].to(dev), t["pos"].to(dev), t["type"][0].contiguous().to(dev), out)
        rw.check_exact("embed_fwd", f"n={B * L} D={D}", out, rw.embed_fwd_ref(t["ids"], pos_ids.cpu(), t["word"], t["pos"], t["type"][0]))


@pytest.mark.parametrize("D", rw.TYPE_D)
def test_embed_type_row_gradient(dev, k, D):
    for n in rw.TYPE_N:
        gen = torch.Generator().manual_seed(100 * n + D)
        g, d0 = torch.randn(n, D, generator=gen).to(BF), torch.randn(D, generator=gen) + 1.5
        ids = torch.randint(3, 9, (n,), generator=gen).to(dev)
        out = d0.to(dev)
        k.embed_bwd(g.to(dev), ids, ids, rw.PAD_ID, None, None, out)
        rw.check("embed_type_bwd", f"n={n} D={D}", out, *rw.embed_type_ref(g, d0))


# ------------------------------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("D", rw.L2_D)
def test_l2norm_every_element(dev, k, D):
    for rows in rw.L2_ROWS:
        t = rw.l2_inputs(rows, D)
        x, dy = t["x"].to(dev), t["dy"].to(dev)
        y, dx = nan_like((rows, D), F32, dev), nan_like((rows, D), F32, dev)
        k.l2norm_fwd(x, y)
        k.l2norm_bwd(x, dy, dx)
        torch.cuda.synchronize()
        rw.check("l2norm_fwd", f"{rows}x{D}", y, *rw.l2norm_fwd_ref(t["x"]))
        rw.check("l2norm_bwd", f"{rows}x{D}", dx, *rw.l2norm_bwd_ref(t["x"], t["dy"]))
        if rows >= 5:                          # the all-zero row: y = 0 and dx = dy * (1.f / eps), the same f32 expression
            assert not y[2].any()
            inv = torch.tensor(1.0, dtype=F32) / torch.tensor(1e-12, dtype=F32)
            rw.check_exact("l2norm_bwd zero row", f"{rows}x{D}", dx[2], t["dy"][2] * inv)
