"""The XCD-resident decoder launches (csrc/xdec.hip: toist_xdec_fwd / toist_xdec_bwd), called DIRECTLY with synthetic parameters, against the plain fp64
decoder stack of oracle/xdec_ref.py -- an independent restatement (tests/test_cpu_xdec_reference.py pins it to oracle/model_ref.py), not the per-op
launches whose arithmetic the XCD kernels copy (tests/test_gpu_xdec.py).  Buffers come from the product's own allocation routines
(tlayer.xdec_fwd_buffers / xdec_bwd_buffers); every output is pre-filled with NaN, kv / sink / dkv are inner column slices of wider tensors.

Three kinds of assertion, per case, layer and tensor:
  teacher-forced   each saved / exported tensor against the fp64 stage fed the launch's OWN preceding tensors, at the tolerances the per-op tests use
                   for the same arithmetic: GEMM + LayerNorm outputs rtol 4e-3 / atol 1e-3 (tests/test_gpu_tlayer.py:44,52,53), mean 1e-4 / 1e-5 and
                   rstd 1e-4 / 1e-6 against the ROUNDED z (:49-50), contexts 1.2e-2 |ref| + 6e-3 and lse 1e-5 / 1e-4, 2e-3 / 1e-6
                   (tests/test_gpu_attn2.py:76-83), LayerNorm input gradients rtol 8e-3 / atol 4e-3 (tests/test_gpu_tlayer.py:102), attention
                   gradients rel Frobenius < 1.5e-2 + the element bound of tests/test_gpu_attn2.py:98-102.
                   The launches fold linear2 (and dh W1 in the backward direction) from 32 bf16 partial sums, one per 64 hidden units (the `part` scratch
                   of the descriptor); that rounding alone exceeds rtol 4e-3 / atol 1e-3 in 6 % of the elements of z4 (measured on the reference:
                   0.8e-3 rms), so the stages of z4 and go3 restate it (round_partials) and keep the tolerance.  A partial within fp32 accumulation error
                   of a bf16 rounding boundary may be stored as either neighbour -- one partial ulp, up to 2e-3 > atol -- so z4 is held against the
                   interval oracle.xdec_ref.st_linear2_bounds derives from the fp32 format alone (worst-case 64 * 2^-24 * sum |h w| per partial: the
                   summation order inside an MFMA is not documented), at the same tolerance on either side.  This is NOT the point comparison the other
                   tensors get: on case d the interval is non-empty for 54 % of the elements, 1.2e-4 wide on average, wider than atol for 1.7 % of
                   them and 3.9e-3 at most.  A dropped or misplaced partial is an error of 0.1.
  exact            y1e == bf16(y1 + qpos), y4e likewise below the last layer, dropped hidden units are 0, padded keys contribute nothing (garbage in their kv
                   rows changes no output bit), padded keys receive a zero gradient, nothing outside the column slices is written.
  free-running     y4 of every layer and every exported gradient against forward() / its autograd with the same masks:
                   relF(launch, reference) <= 3 e_model + 1e-3, e_model = relF(forward(round_stores=True), forward()) -- a reference-only quantity.
                   dq / dk of a softmax over a single key (case a) are exactly zero and leave the fp32 kernels as cancellation noise: only where the fp64 reference is zero (rms < 1e-12) relF takes 1e-4 per element as its norm (the absolute term
                   of tests/test_gpu_attn2.py:101); every other tensor is divided by its own norm alone.
                   At p > 0 the gradients' e_model is 4-10 % (ReLU gates flipped by bf16 rounding), so this bound is loose there; the backward chain
                   is held tightly by the teacher-forced stages of the p = 0 cases, case l (two layers) for the layer-to-layer hand-off.
                   The launch does not export norm1's unmasked input gradient, so the residual share of the x0 gradient (gx_res) is formed only at p = 0
                   (there go1 is it); the in_proj share (gx_proj = sink[:, :768] W_in of layer 0) is compared in every case.
e_model and the measured errors are written to xdec_reference.json (beside the b8 oracle parity test's measurements, see _report) before any assertion;
the last run is committed as profiles/xdec_reference.json."""
import pytest
import torch

from oracle import xdec_ref as xr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = xr.D
FLOOR = 1e-4
NAN = float("nan")


def _report(case, val):
    """xdec_reference.json in the measurement directory of tests/test_gpu_b8_oracle_parity.py, through that test's own report helper"""
    from test_gpu_b8_oracle_parity import _report as report
    report(case, val, name="xdec_reference.json")


@pytest.fixture(scope="module")
def xdec_state():
    """the launches' process-wide state: restored after the module"""
    from toist_amd import kernels as k
    failed, seed_dev = k.XDEC_FAILED, k.SEED_DEV
    k.SEED_DEV = None
    yield k
    k.XDEC_FAILED, k.SEED_DEV = failed, seed_dev


def _checked(k):
    """after every launch: an expired spin fails the test with the library's own message"""
    torch.cuda.synchronize()
    k.xdec_check()


def _forward_launch(k, c, dev, kv_wide):
    from toist_amd import tlayer
    B, Q, S, L = c["B"], c["Q"], c["S"], c["L"]
    tgt_stack = torch.full((L, B * Q, D), NAN, dtype=BF, device=dev)
    out, part = tlayer.xdec_fwd_buffers(B, Q, L, dev, tgt_stack)
    for t in out.values():
        t.fill_(NAN)
    kv = kv_wide[:, 32:32 + L * 2 * D]
    k.xdec_fwd(B, Q, S, c["dev"]["x0"], c["dev"]["qpos"], kv, c["dev"]["key_pad"], c["p"], 1e-5, out, c["dev"]["layers"], part, xe0=c["dev"]["xe0"])
    _checked(k)
    return out, part


def _backward_launch(k, c, dev, out, part):
    from toist_amd import tlayer
    B, Q, S, L = c["B"], c["Q"], c["S"], c["L"]
    M = B * Q
    sink_wide = torch.full((M, L * 4 * D + 64), NAN, dtype=BF, device=dev)
    dkv_wide = torch.full((B * S, L * 2 * D + 64), NAN, dtype=BF, device=dev)
    outs, scratch = tlayer.xdec_bwd_buffers(B, Q, L, dev, sink_wide[:, 32:32 + L * 4 * D], dkv_wide[:, 32:32 + L * 2 * D], part)
    for n in ("gb4", "dh", "go3", "go1", "ln_part"):
        outs[n].fill_(NAN)
    splits_c = ((S + 31) // 32 + 3) // 4
    assert splits_c == k.attn2_splits(S) and 1 <= splits_c <= 4
    scratch["dq_part"][splits_c if splits_c > 1 else 0:].fill_(NAN)          # shares beyond splits_c (all of them without a split) must not be read
    table = [{n: P[n] for n in ("w_in", "w_os", "w_q", "w_oc", "w1", "w2", "g1", "g3", "g4", "seed")} for P in c["dev"]["layers"]]
    kv = c["dev"]["kv_wide"][:, 32:32 + L * 2 * D]
    k.xdec_bwd(B, Q, S, kv, c["dev"]["key_pad"], c["p"], out, c["dev"]["g_out"], outs, table, scratch)
    _checked(k)
    return outs, scratch, sink_wide, dkv_wide, splits_c


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


@pytest.fixture(scope="module", params=list(xr.CASES))
def run(request, dev, xdec_state):
    k = xdec_state
    name = request.param
    c = xr.make_case(name)
    B, Q, S, L, p = c["B"], c["Q"], c["S"], c["L"], c["p"]
    if not k.xdec_supported(B, Q, S, L):
        pytest.skip("device without 8 XCDs x 32 CUs")
    c["dev"] = dict(x0=c["x0"].to(dev), qpos=c["qpos"].to(dev), xe0=(c["x0"].float() + c["qpos"].float()).to(BF).to(dev), kv_wide=c["kv_wide"].to(dev),
                    key_pad=c["key_pad"].to(dev) if c["key_pad"] is not None else None,
                    g_out=c["g_out"].to(dev), layers=[{n: (v if n == "seed" else v.to(dev).contiguous()) for n, v in P.items()} for P in c["layers"]])
    r = dict(c=c, name=name)
    # ---- the launches ----
    out, part = _forward_launch(k, c, dev, c["dev"]["kv_wide"])
    r["kv_untouched"] = torch.equal(c["dev"]["kv_wide"].cpu().view(torch.int16), c["kv_wide"].view(torch.int16))
    r["same_bits_with_garbage"] = None
    if c["key_pad"] is not None:          # garbage in the kv rows of padded keys: no output bit may change
        junk = c["dev"]["kv_wide"].clone()
        junk[c["dev"]["key_pad"].bool().view(-1)] = 1e30
        out2, _ = _forward_launch(k, c, dev, junk)
        r["same_bits_with_garbage"] = {n: bool(torch.equal(_bits(out[n]), _bits(out2[n]))) for n in out}
        del out2, junk
    outs, scratch, sink_wide, dkv_wide, splits_c = _backward_launch(k, c, dev, out, part)
    r["splits_c"] = splits_c
    r["fw"] = {n: t.double().cpu() for n, t in out.items()}
    r["bw"] = {n: outs[n].double().cpu() for n in ("gb4", "dh", "go3", "go1", "ln_part")}
    r["bw"]["sink"], r["bw"]["dkv"] = outs["sink"].double().cpu(), outs["dkv"].double().cpu()
    r["sink_wide"], r["dkv_wide"], r["dq_part"] = sink_wide.float().cpu(), dkv_wide.float().cpu(), scratch["dq_part"].float().cpu()
    del out, part, outs, scratch, sink_wide, dkv_wide
    # ---- the reference, once per case ----
    r["P64"] = [{n: (v if n == "seed" else v.double()) for n, v in P.items()} for P in c["layers"]]
    r["ref"], r["mod"] = xr.run_reference(c), xr.run_reference(c, round_stores=True)
    r["e"] = xr.e_model(r["ref"], r["mod"], FLOOR)
    del r["mod"]
    r["got"] = _launch_grads(r)
    meas = {"y4": [xr.relF(r["fw"]["y4"][l], r["ref"][0]["y4"][l], FLOOR) for l in range(L)]}
    for n, v in r["got"].items():
        meas[n] = [xr.relF(a, b, FLOOR) for a, b in zip(v, r["ref"][1][n])]
    r["meas"] = meas
    r["tf_fwd"], r["tf_bwd"] = _teacher_forced_forward(r), (_teacher_forced_backward(r) if p == 0 else {})
    _report(name, {"shape": dict(B=B, Q=Q, S=S, L=L, p=p, pad=c["pad"], splits_c=splits_c),
                   "free_running": {n: {"e_model": [float("%.3e" % x) for x in r["e"][n]], "launch": [float("%.3e" % x) for x in meas[n]]} for n in meas},
                   "teacher_forced_forward_worst_excess": {n: float("%.3e" % max(v)) for n, v in r["tf_fwd"].items()},
                   "teacher_forced_backward_worst_excess": {n: float("%.3e" % max(v)) for n, v in r["tf_bwd"].items()}})
    return r


def _launch_grads(r):
    """the backward launch's exports under the names of oracle.xdec_ref.GRADS"""
    c, bw = r["c"], r["bw"]
    g = {n: [] for n in xr.GRADS}
    for l in range(c["L"]):
        for n in ("gb4", "dh", "go3", "go1"):
            g[n].append(bw[n][l])
        s0 = l * 4 * D
        for j, n in enumerate(("dq_s", "dk_s", "dv_s", "dq_c")):
            g[n].append(bw["sink"][:, s0 + j * D:s0 + (j + 1) * D])
        g["dk_c"].append(bw["dkv"][:, l * 2 * D:l * 2 * D + D])
        g["dv_c"].append(bw["dkv"][:, l * 2 * D + D:(l + 1) * 2 * D])
        for w, n in enumerate(("1", "3", "4")):
            g["dg" + n].append(bw["ln_part"][l, w, 0].sum(0))
            g["dbe" + n].append(bw["ln_part"][l, w, 1].sum(0))
    g["gx_proj"] = [bw["sink"][:, :3 * D] @ r["P64"][0]["w_in"]]
    if c["p"] == 0:
        g["gx_res"] = [bw["go1"][0]]
    return g


def _excess(got, ref, rtol, atol):
    """worst |got - ref| - (rtol |ref| + atol): <= 0 passes; NaN (an unwritten element) counts as +inf.  ref = (lo, hi): the distance to the interval."""
    if isinstance(ref, tuple):
        lo, hi = ref
        x = torch.maximum(lo - got - (rtol * lo.abs() + atol), got - hi - (rtol * hi.abs() + atol))
    else:
        x = (got - ref).abs() - (rtol * ref.abs() + atol)
    return float(torch.nan_to_num(x, nan=float("inf")).max())


TOL = {"qkv": (4e-3, 1e-3), "z1": (4e-3, 1e-3), "y1": (4e-3, 1e-3), "y1e": (4e-3, 1e-3), "qc": (4e-3, 1e-3), "z3": (4e-3, 1e-3), "y3": (4e-3, 1e-3),
       "h": (4e-3, 1e-3), "z4": (4e-3, 1e-3), "y4": (4e-3, 1e-3), "y4e": (4e-3, 1e-3), "mean1": (1e-4, 1e-5), "mean3": (1e-4, 1e-5), "mean4": (1e-4, 1e-5),
       "rstd1": (1e-4, 1e-6), "rstd3": (1e-4, 1e-6), "rstd4": (1e-4, 1e-6), "ctx_s": (1.2e-2, 6e-3), "ctx_c": (1.2e-2, 6e-3)}


def _layer_io(r, l):
    c, fw = r["c"], r["fw"]
    sv = {n: fw[n][l] for n in xr.SAVED}
    x_in = c["x0"].double() if l == 0 else fw["y4"][l - 1]
    xe_in = xr.bf16(c["x0"].double() + c["qpos"].double()) if l == 0 else fw["y4e"][l - 1]          # layer 0: the xe0 the launch was given
    kv = c["kv"].double()
    return sv, x_in, xe_in, (kv[:, l * 2 * D:l * 2 * D + D], kv[:, l * 2 * D + D:(l + 1) * 2 * D])


def _teacher_forced_forward(r):
    c = r["c"]
    ex = {}
    for l in range(c["L"]):
        sv, x_in, xe_in, kv_l = _layer_io(r, l)
        st = xr.layer_stages(sv, x_in, xe_in, c["qpos"].double(), kv_l, c["key_pad"], r["P64"][l], c["p"], c["B"], c["Q"], c["S"], last=l + 1 == c["L"],
                             round_partials="bounds")
        for n, ref in st.items():
            if n.startswith("lse"):
                ex.setdefault(n + ".max", []).append(_excess(sv[n][..., 0], ref[..., 0], 1e-5, 1e-4))
                ex.setdefault(n + ".inv_sum", []).append(_excess(sv[n][..., 1], ref[..., 1], 2e-3, 1e-6))
            else:
                ex.setdefault(n, []).append(_excess(sv[n], ref, *TOL[n]))
    return ex


def _attn_grad_excess(got, ref):
    """tests/test_gpu_attn2.py:98-102: (rel Frobenius - 1.5e-2, fraction of elements beyond 3e-2 |ref| + 3e-2 mean |ref| + 1e-4 - 1e-3); an exactly zero
    reference (case a) counts as 1e-4 per element in the Frobenius norm (xr.relF)"""
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    err = (got - ref).abs()
    bound = 3e-2 * ref.abs() + 3e-2 * float(ref.abs().mean()) + 1e-4
    return xr.relF(got, ref, FLOOR) - 1.5e-2, float((err > bound).double().mean()) - 1e-3


def _teacher_forced_backward(r):
    c, bw = r["c"], r["bw"]
    L = c["L"]
    exs = [dict(gb4=bw["gb4"][l], dh=bw["dh"][l], go3=bw["go3"][l], go1=bw["go1"][l], sink=bw["sink"][:, l * 4 * D:(l + 1) * 4 * D]) for l in range(L)]
    ex = {}
    for l in range(L - 1, -1, -1):
        sv, _, _, kv_l = _layer_io(r, l)
        gy = c["g_out"][l].double()
        if l < L - 1:
            gy = gy + xr.input_grad(exs[l + 1], r["P64"][l + 1])
        st = xr.backward_stages(sv, exs[l], gy, kv_l, c["key_pad"], r["P64"][l], c["B"], c["Q"], c["S"], round_partials=True)
        for n in ("gb4", "go3", "go1"):
            ex.setdefault(n, []).append(_excess(exs[l][n], st[n], 8e-3, 4e-3))
        ex.setdefault("dh", []).append(_excess(exs[l]["dh"], st["dh"], 4e-3, 1e-3))
        got = {"dq_c": exs[l]["sink"][:, 3 * D:], "dk_c": bw["dkv"][:, l * 2 * D:l * 2 * D + D], "dv_c": bw["dkv"][:, l * 2 * D + D:(l + 1) * 2 * D]}
        for j, n in enumerate(("dq_s", "dk_s", "dv_s")):
            got[n] = exs[l]["sink"][:, j * D:(j + 1) * D]
            st[n] = st["dqkv_s"][:, j * D:(j + 1) * D]
        for n, t in got.items():
            fro, frac = _attn_grad_excess(t, st[n])
            ex.setdefault(n + ".relF", []).append(fro)
            ex.setdefault(n + ".elements", []).append(frac)
    return ex


# ------------------------------------------------------------------------------------------------------------------ forward
def test_forward_teacher_forced(run):
    """every saved tensor of every layer against the fp64 stage fed the launch's own preceding tensors"""
    assert set(run["tf_fwd"]) == (set(xr.SAVED) - {"lse_s", "lse_c"} - ({"y4e"} if run["c"]["L"] == 1 else set())) | {"lse_s.max", "lse_s.inv_sum", "lse_c.max", "lse_c.inv_sum"}
    bad = {n: v for n, v in run["tf_fwd"].items() if not max(v) <= 0}
    assert not bad, f"case {run['name']}: worst excess over the tolerance, per layer: {bad}"


def test_forward_exact_properties(run):
    c, fw = run["c"], run["fw"]
    L, p = c["L"], c["p"]
    qpos = c["qpos"].double()
    for n, t in fw.items():
        live = t if n != "y4e" else t[:L - 1]
        assert bool(torch.isfinite(live).all()), f"{n}: not every element was written"
    assert bool(torch.isnan(fw["y4e"][L - 1]).all())              # the last layer has no successor: left alone
    assert run["kv_untouched"]
    for l in range(L):
        assert torch.equal(fw["y1e"][l], xr.bf16(fw["y1"][l] + qpos)), l
        if l < L - 1:
            assert torch.equal(fw["y4e"][l], xr.bf16(fw["y4"][l] + qpos)), l
        if p > 0:
            keep = xr.elem_keep(c["B"] * c["Q"], xr.FF, p, c["layers"][l]["seed"][4])
            assert float(fw["h"][l][~keep].abs().max()) == 0.0, l
            assert 0.4 < float((fw["h"][l][keep] > 0).double().mean()) < 0.6          # and the kept ones are a ReLU's output
    if run["same_bits_with_garbage"] is not None:
        changed = [n for n, same in run["same_bits_with_garbage"].items() if not same]
        assert not changed, f"1e30 in the kv rows of padded keys changed {changed}"


def test_forward_free_running(run):
    e, meas = run["e"]["y4"], run["meas"]["y4"]
    bad = {l: (m, 3 * x + 1e-3) for l, (m, x) in enumerate(zip(meas, e)) if not m <= 3 * x + 1e-3}
    assert not bad, f"case {run['name']}: y4 per layer (relF against fp64, bound 3 e_model + 1e-3): {bad}"


# ------------------------------------------------------------------------------------------------------------------ backward
def test_backward_teacher_forced(run):
    """p = 0: stage by stage from the launch's own exports"""
    if run["c"]["p"] > 0:
        assert run["tf_bwd"] == {}
        return
    assert len(run["tf_bwd"]) == 4 + 12
    bad = {n: v for n, v in run["tf_bwd"].items() if not max(v) <= 0}
    assert not bad, f"case {run['name']}: worst excess over the tolerance, per layer (top layer first): {bad}"


def test_backward_against_autograd(run):
    """every exported tensor against fp64 autograd of forward() with the same masks"""
    c = run["c"]
    want = set(xr.GRADS) | {"gx_proj"} | ({"gx_res"} if c["p"] == 0 else set())
    assert set(run["got"]) == want
    bad = {}
    for n in sorted(want):
        for l, (m, x) in enumerate(zip(run["meas"][n], run["e"][n])):
            if not m <= 3 * x + 1e-3:
                bad[f"{n}[{l}]"] = (m, 3 * x + 1e-3)
    assert not bad, f"case {run['name']}: relF against fp64 autograd beyond 3 e_model + 1e-3: {bad}"


def test_backward_wrote_what_it_exports_and_nothing_else(run):
    c, bw = run["c"], run["bw"]
    L = c["L"]
    for n, t in bw.items():
        assert bool(torch.isfinite(t).all()), f"{n}: not every element was written"
    for wide, width in ((run["sink_wide"], L * 4 * D), (run["dkv_wide"], L * 2 * D)):          # the 32 columns on either side of the slices
        assert bool(torch.isnan(wide[:, :32]).all()) and bool(torch.isnan(wide[:, 32 + width:]).all())
    if c["key_pad"] is not None:
        dead = c["key_pad"].bool().view(-1)
        assert float(bw["dkv"][dead].abs().max()) == 0.0           # padded keys: exactly no gradient
        assert float(bw["dkv"][~dead].abs().max()) > 0.0
    first_unused = run["splits_c"] if run["splits_c"] > 1 else 0
    assert bool(torch.isnan(run["dq_part"][first_unused:]).all())          # neither read (the results above are finite) nor written
    assert bool(torch.isfinite(run["dq_part"][:first_unused]).all())
