"""The hand-written TRAIN-MODE programs of toist_amd.engine / tlayer / transformer.py -- dropout 0.1, as the recipe trains -- against fp64 autograd of
oracle/train_ref.py with the SAME masks: the masks come from the host hashes (oracle/xdec_ref.py, oracle/train_ref.py) and the seeds from
train_ref.tape_seeds, the restated engine.Tape.  Every block runs through functions.run_program(training=True, drop_p, seed) on small named parameters
with a fixed random linear functional of its output as the loss; the output, every input gradient and every parameter gradient are compared.

What fails here and nowhere else in the suite: a backward that masks with another element index than its forward (a row pitch off by one), that applies
1 / (1 - p) twice or not at all, that drops the residual share of a gradient, or that draws its seeds in another order than the forward.

  blocks      linear_chain ReLU FFN (dropout_after + final_drop) + residual + layernorm (Var.drop / gdrop through the LayerNorm backward), the GELU chain with
              final_drop (take_branch_grad's own launch), engine.dropout (exact), engine.attention on the per-op core (cross attention 33 x 52 and packed
              self attention, head dim 64) and on the flash-style core (head dim 32), text_attention_block
  programs    two layers each: Transformer.encode_tokens on its two routes (tlayer.encoder_program, the per-op program), Transformer.encode_text on
              a tiny RoBERTa; for every route the seeds the tape drew must be the seeds the reference consumed, one per site of train_ref.ROUTES

Bounds (none is fitted to what the kernels give):
  free-running  every output and every gradient: relF(device, fp64) <= 3 e_model + 1e-3, e_model = relF(reference(round_stores=True), reference()), the rule of
              tests/test_gpu_xdec_reference.py; where the fp64 value is exactly zero (rms < 1e-12: the key bias of a softmax) relF takes 1e-4 per element as
              the norm, as there
  per-op, elementwise  every block output against the fp64 block at the suite's bound for its arithmetic: GEMM + LayerNorm outputs rtol 4e-3 / atol 1e-3
              (tests/test_gpu_tlayer.py), the rows leaving an attention block 1.2e-2 |ref| + 6e-3 (tests/test_gpu_attn2.py).  Those are bounds on ONE stage
              fed the device's own inputs; a block chains several bf16 stores, and for three blocks the reference's own rounding model -- a quantity of the
              reference alone -- exceeds them: by 8.9e-3 on the ReLU FFN + LayerNorm output, by 2.9e-3 on the GELU chain (two chained GEMMs, a bf16 hidden
              tensor), by 1.1e-3 on the cross-attention rows.  The rule is therefore: where the rounding model's worst excess is <= 0 the device's must be
              <= 0 (the bound as the issue states it: the self-attention blocks on both cores, both text_attention_blocks); elsewhere the device's worst
              excess may reach the model's plus one bf16 ulp at the largest output magnitude (2^-7 max |ref|): the device makes the model's stores, and
              where its f32 value and the model's fp64 value fall on different sides of a rounding boundary the stored element -- the output itself, or the
              pre-norm element (z - mean) rstd gamma that a LayerNorm output is proportional to -- differs by one ulp.  Both figures and the allowance are
              in the JSON ("out_elementwise_excess").  The FFN block's LayerNorm is ALSO held to rtol 4e-3 / atol 1e-3 as a single stage, on the pre-norm
              rows the device stored (the program body hands them out).
  engine.dropout  bit-exact, forward and backward
Where a block's e_model exceeds 2 % at p = 0.1 (ReLU gates flipped by a rounding) the bound is loose: the same case runs at p = 0 as well ("<name>@p0"),
so the chain is held tightly once; the JSON marks the loose cases.  e_model and the measured errors go to train_mode_reference.json (beside the b8 oracle
parity test's measurements) before any assertion; the last run is committed as profiles/train_mode_reference.json.

Element indices at or above 2^32 are not covered (the host hash handles lower indices only); no tensor here is that large."""
import math
from collections import OrderedDict

import pytest
import torch

from oracle import train_ref as tr
from oracle import xdec_ref as xr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
FLOOR = 1e-4
P = 0.1
GEMM_LN = (4e-3, 1e-3)
ATTN_ROWS = (1.2e-2, 6e-3)


def _report(case, val):
    from test_gpu_b8_oracle_parity import _report as report
    report(case, val, name="train_mode_reference.json")


@pytest.fixture(scope="module")
def state():
    """process-wide switches the cases touch: restored after the module"""
    from toist_amd import engine, tlayer
    from toist_amd import kernels as k
    old = (k.SEED_DEV, tlayer.ENABLED, engine.FUSED_BLOCKS)
    k.SEED_DEV = None
    yield
    k.SEED_DEV, tlayer.ENABLED, engine.FUSED_BLOCKS = old


# ------------------------------------------------------------------------------------------------------------------ synthetic parameters
def _w(g, o, i):
    """a weight matrix that IS its bf16 compute copy"""
    return (torch.randn(o, i, generator=g) / math.sqrt(i)).to(BF).float()


def _b(g, n):
    return torch.randn(n, generator=g) * 0.1


def _gamma(g, n):
    return torch.rand(n, generator=g) + 0.5


def _rows(g, m, n):
    return torch.randn(m, n, generator=g).to(BF)


def _tail_pad(B, S):
    kp = torch.zeros(B, S, dtype=torch.uint8)
    for b in range(B):
        kp[b, S - 1 - 3 * b:] = 1
    return kp


# ------------------------------------------------------------------------------------------------------------------ cases
# A case: params {name: f32}, inputs {name: bf16 rows}, body(dev) -> program body, ref(lv, rs, masks) -> fp64 output from the leaves lv, masks(p, seed) ->
# ({site: keep}, seeds consumed), out_tol = the per-op elementwise bound whose excess is reported for the output, stash = tensors the body hands out
def _case_ffn_relu():
    d, ff, M = 256, 512, 200
    g = torch.Generator().manual_seed(11)
    params = OrderedDict([("linear1.weight", _w(g, ff, d)), ("linear1.bias", _b(g, ff)), ("linear2.weight", _w(g, d, ff)), ("linear2.bias", _b(g, d)),
                          ("norm.weight", _gamma(g, d)), ("norm.bias", _b(g, d))])
    inputs = OrderedDict(x=_rows(g, M, d))
    stash = {}

    def body(dev):
        from toist_amd import engine
        from toist_amd import kernels as k

        def prog(tape, ps, x):
            z = engine.linear_chain(tape, x, [(ps["linear1.weight"], ps["linear1.bias"], k.ACT_RELU, True), (ps["linear2.weight"], ps["linear2.bias"], k.ACT_NONE, False)],
                                    res=x, final_drop=True)
            stash["z"] = z.data         # the stored pre-norm sum (not a program output: the LayerNorm backward must find z.grad empty to emit gdrop)
            return [engine.layernorm(tape, z, ps["norm.weight"], ps["norm.bias"], 1e-5)], None
        return prog

    def ref(lv, rs, masks, p):
        z = tr.ffn_relu_block(lv["x"], lv["linear1.weight"], lv["linear1.bias"], lv["linear2.weight"], lv["linear2.bias"], p, masks.get("hidden"), masks.get("out"), rs)
        return tr._modes(rs)[0](tr.layer_norm(z, lv["norm.weight"], lv["norm.bias"], 1e-5))

    def masks(p, seed):
        s = tr.tape_seeds(seed)
        used = [next(s), next(s)]
        return dict(hidden=xr.elem_keep(M, ff, p, used[0]), out=xr.elem_keep(M, d, p, used[1])), used

    return dict(params=params, inputs=inputs, body=body, ref=ref, masks=masks, out_tol=GEMM_LN, g_shape=(M, d), stash=stash)


def _case_ffn_gelu():
    D, ff, M = 128, 512, 48
    g = torch.Generator().manual_seed(12)
    params = OrderedDict([("intermediate.weight", _w(g, ff, D)), ("intermediate.bias", _b(g, ff)), ("output.weight", _w(g, D, ff)), ("output.bias", _b(g, D))])
    inputs = OrderedDict(x=_rows(g, M, D))

    def body(dev):
        from toist_amd import engine
        from toist_amd import kernels as k

        def prog(tape, ps, x):
            return [engine.linear_chain(tape, x, [(ps["intermediate.weight"], ps["intermediate.bias"], k.ACT_GELU, False),
                                                  (ps["output.weight"], ps["output.bias"], k.ACT_NONE, False)], res=x, final_drop=True)], None
        return prog

    def ref(lv, rs, masks, p):
        return tr.ffn_gelu_block(lv["x"], lv["intermediate.weight"], lv["intermediate.bias"], lv["output.weight"], lv["output.bias"], p, masks.get("out"), rs)

    def masks(p, seed):
        used = [next(tr.tape_seeds(seed))]
        return dict(out=xr.elem_keep(M, D, p, used[0])), used

    return dict(params=params, inputs=inputs, body=body, ref=ref, masks=masks, out_tol=GEMM_LN, g_shape=(M, D))


def _case_attention(kind):
    """engine.attention: "cross" (d 128, 2 heads of 64, 33 queries x 52 keys, three separate projections), "self" (the same heads, packed q | k, S = 40),
    "fused" (d 256, 8 heads of 32: the flash-style core, packed q | k, S = 40); padded keys in every one"""
    d, H = (256, 8) if kind == "fused" else (128, 2)
    B = 2
    Sq, Sk = (33, 52) if kind == "cross" else (40, 40)
    core = "flash" if kind == "fused" else "softmax"
    g = torch.Generator().manual_seed(20 + len(kind))
    key_pad = _tail_pad(B, Sk)
    if kind == "cross":
        params = OrderedDict([(n + s, f(g)) for n in ("q", "k", "v", "o") for s, f in ((".weight", lambda g_: _w(g_, d, d)), (".bias", lambda g_: _b(g_, d)))])
        inputs = OrderedDict(q_in=_rows(g, B * Sq, d), k_in=_rows(g, B * Sk, d), v_in=_rows(g, B * Sk, d))
    else:
        params = OrderedDict([("in_proj_weight", _w(g, 3 * d, d)), ("in_proj_bias", _b(g, 3 * d)), ("o.weight", _w(g, d, d)), ("o.bias", _b(g, d))])
        inputs = OrderedDict(xe=_rows(g, B * Sq, d), x=_rows(g, B * Sq, d))

    def body(dev):
        from toist_amd import engine
        kp = key_pad.to(dev)

        def prog_cross(tape, ps, q_in, k_in, v_in):
            return [engine.attention(tape, q_in, k_in, v_in, (ps["q.weight"], ps["q.bias"]), (ps["k.weight"], ps["k.bias"]), (ps["v.weight"], ps["v.bias"]),
                                     ps["o.weight"], ps["o.bias"], q_in, kp, B, Sq, Sk, H)], None

        def prog_self(tape, ps, xe, x):
            Wi, bi = ps["in_proj_weight"], ps["in_proj_bias"]
            return [engine.attention(tape, xe, xe, x, None, None, (Wi.rows(2 * d, 3 * d), bi.rows(2 * d, 3 * d)), ps["o.weight"], ps["o.bias"], x, kp, B, Sq, Sk, H,
                                     packed_qk=(Wi.rows(0, 2 * d), bi.rows(0, 2 * d)))], None
        return prog_cross if kind == "cross" else prog_self

    def ref(lv, rs, masks, p):
        rnd, rg = tr._modes(rs)
        if kind == "cross":
            q, k_, v = (rg(rnd(lv[i] @ lv[n + ".weight"].t() + lv[n + ".bias"])) for i, n in (("q_in", "q"), ("k_in", "k"), ("v_in", "v")))
            resid = lv["q_in"]
        else:
            W, b = lv["in_proj_weight"], lv["in_proj_bias"]
            qk = rg(rnd(lv["xe"] @ W[:2 * d].t() + b[:2 * d]))
            q, k_, v = qk[:, :d], qk[:, d:], rg(rnd(lv["x"] @ W[2 * d:].t() + b[2 * d:]))
            resid = lv["x"]
        ctx = rg(rnd(tr.attention_core(q, k_, v, key_pad.bool(), B, H, Sq, Sk, p, masks.get("attn"), core, rs)))
        return tr.out_proj_block(ctx, lv["o.weight"], lv["o.bias"], resid, p, masks.get("out"), rs)

    def masks(p, seed):
        s = tr.tape_seeds(seed)
        used = [next(s), next(s)]
        keep = xr.attn_keep(B * H, Sq, Sk, p, used[0]) if core == "flash" else tr.softmax_keep(B * H * Sq, Sk, p, used[0])
        return dict(attn=keep.view(B, H, Sq, Sk), out=xr.elem_keep(B * Sq, d, p, used[1])), used

    return dict(params=params, inputs=inputs, body=body, ref=ref, masks=masks, out_tol=ATTN_ROWS, g_shape=(B * Sq, d))


def _case_text_attention(B, L, H, D):
    g = torch.Generator().manual_seed(B * 100 + L)
    names = ("query", "key", "value")
    params = OrderedDict()
    for n in names + ("dense",):
        params[n + ".weight"], params[n + ".bias"] = _w(g, D, D), _b(g, D)
    inputs = OrderedDict(x=_rows(g, B * L, D))
    key_pad = _tail_pad(B, L)

    def body(dev):
        from toist_amd import engine
        kp = key_pad.to(dev)
        buf = torch.zeros(3 * D, D, dtype=BF, device=dev)

        def prog(tape, ps, x):
            proj = [(ps[n + ".weight"], ps[n + ".bias"]) for n in names]
            return [engine.text_attention_block(tape, x, proj, buf, ps["dense.weight"], ps["dense.bias"], kp, B, L, H)], None
        prog.transforms = {n + ".weight": engine.packed_cast(buf[j * D:(j + 1) * D]) for j, n in enumerate(names)}
        return prog

    def ref(lv, rs, masks, p):
        rnd, rg = tr._modes(rs)
        q, k_, v = (rg(rnd(lv["x"] @ lv[n + ".weight"].t()) + lv[n + ".bias"]) for n in names)
        ctx = rg(rnd(tr.attention_core(q, k_, v, key_pad.bool(), B, H, L, L, p, masks.get("attn"), "small", rs)))
        return tr.out_proj_block(ctx, lv["dense.weight"], lv["dense.bias"], lv["x"], p, masks.get("out"), rs)

    def masks(p, seed):
        s = tr.tape_seeds(seed)
        used = [next(s), next(s)]
        return dict(attn=tr.small_attn_keep(B, H, L, p, used[0]), out=xr.elem_keep(B * L, D, p, used[1])), used

    return dict(params=params, inputs=inputs, body=body, ref=ref, masks=masks, out_tol=ATTN_ROWS, g_shape=(B * L, D))


BLOCKS = {
    "ffn_relu_ln": _case_ffn_relu,
    "ffn_gelu": _case_ffn_gelu,
    "attention_cross_per_op": lambda: _case_attention("cross"),
    "attention_self_per_op": lambda: _case_attention("self"),
    "attention_self_fused_core": lambda: _case_attention("fused"),
    "text_attention_3x11": lambda: _case_text_attention(3, 11, 4, 128),
    "text_attention_2x40": lambda: _case_text_attention(2, 40, 2, 128),
}


# ------------------------------------------------------------------------------------------------------------------ running a case
class _count_seeds:
    """records every draw of engine.Tape.next_seed inside the with block"""

    def __enter__(self):
        from toist_amd import engine
        self.drawn, self.orig = [], engine.Tape.next_seed
        orig, drawn = self.orig, self.drawn

        def next_seed(tape):
            s = orig(tape)
            drawn.append(s)
            return s
        engine.Tape.next_seed = next_seed
        return self.drawn

    def __exit__(self, *exc):
        from toist_amd import engine
        engine.Tape.next_seed = self.orig
        return False


def _device_run(case, dev, p, seed, g_out):
    from toist_amd import functions
    named = OrderedDict((n, torch.nn.Parameter(t.to(dev))) for n, t in case["params"].items())
    ins = [t.to(dev).requires_grad_(True) for t in case["inputs"].values()]
    prog = case["body"](dev)
    with _count_seeds() as drawn:
        (out,) = functions.run_program(prog, named, ins, cache={}, training=True, drop_p=p, seed=seed, transforms=getattr(prog, "transforms", None))
        (out.float() * g_out.to(dev).float()).sum().backward()
        torch.cuda.synchronize()
    got = {"out": out.detach().double().cpu()}
    got.update({n: t.grad.double().cpu() for n, t in zip(case["inputs"], ins) if t.grad is not None})
    got.update({n: q.grad.double().cpu() for n, q in named.items() if q.grad is not None})
    return got, drawn


def _reference(case, p, seed, g_out):
    masks, used = case["masks"](p, seed) if p > 0 else ({}, [])
    leaves = dict(case["inputs"])
    leaves.update(case["params"])
    ref = tr.run(lambda lv, rs: case["ref"](lv, rs, masks, p), leaves, g_out)
    mod = tr.run(lambda lv, rs: case["ref"](lv, rs, masks, p), leaves, g_out, round_stores=True)
    return ref, tr.errors(mod, ref, FLOOR), used, mod["out"]


def _excess(got, ref, rtol, atol):
    x = (got - ref).abs() - (rtol * ref.abs() + atol)
    return float(torch.nan_to_num(x, nan=float("inf")).max())


def _evaluate(name, case, dev, p, seed):
    g = torch.Generator().manual_seed(seed)
    g_out = torch.randn(*case["g_shape"], generator=g).to(BF)
    ref, e, used, mod_out = _reference(case, p, seed, g_out)
    got, drawn = _device_run(case, dev, p, seed, g_out)
    assert set(got) == set(ref), (sorted(set(got) ^ set(ref)))
    meas = tr.errors(got, ref, FLOOR)
    r3 = lambda v: float("%.3e" % v)
    rec = {"p": p, "e_model": {n: r3(v) for n, v in e.items()}, "device": {n: r3(v) for n, v in meas.items()}, "seeds_drawn": len(drawn),
           "loose": sorted(n for n, v in e.items() if v > 2e-2)}
    # the block output, elementwise, at the per-op bound of its arithmetic: worst excess of the device and of the reference's own rounding model
    model_x, device_x = _excess(mod_out, ref["out"], *case["out_tol"]), _excess(got["out"], ref["out"], *case["out_tol"])
    allowed = 0.0 if model_x <= 0 else model_x + 2.0 ** -7 * float(ref["out"].abs().max())
    rec["out_elementwise_excess"] = {"rtol": case["out_tol"][0], "atol": case["out_tol"][1], "device": r3(device_x), "rounding_model": r3(model_x), "allowed": r3(allowed)}
    if "stash" in case:                 # the LayerNorm stage alone, fed the pre-norm rows the device stored
        z = case["stash"].pop("z").double().cpu()
        y = tr.layer_norm(z, case["params"]["norm.weight"].double(), case["params"]["norm.bias"].double(), 1e-5)
        rec["layernorm_stage_excess"] = r3(_excess(got["out"], y, *GEMM_LN))
    _report(name if p > 0 else name + "@p0", rec)
    return dict(ref=ref, e=e, got=got, meas=meas, used=used, drawn=drawn, rec=rec, out_excess=(device_x, allowed))


def _assert_output_elementwise(name, r):
    device_x, allowed = r["out_excess"]
    assert device_x <= allowed, f"{name}: worst excess of the output over its per-op elementwise bound {device_x:.3e}, allowed {allowed:.3e} ({r['rec']['out_elementwise_excess']})"


def _assert_free_running(name, r):
    bad = {n: (m, 3 * r["e"][n] + 1e-3) for n, m in r["meas"].items() if not m <= 3 * r["e"][n] + 1e-3}
    assert not bad, f"{name}: relF against fp64 autograd beyond 3 e_model + 1e-3: {bad}"


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_with_dropout(dev, state, name):
    case = BLOCKS[name]()
    r = _evaluate(name, case, dev, P, seed=5)
    r0 = _evaluate(name, case, dev, 0.0, seed=5) if r["rec"]["loose"] else None          # the tight run of a case whose bound is loose at p = 0.1
    assert r["drawn"] == r["used"], f"{name}: the tape drew {len(r['drawn'])} seeds, the reference consumed {len(r['used'])}"
    assert r["rec"].get("layernorm_stage_excess", 0.0) <= 0, f"{name}: LayerNorm of the stored rows beyond rtol 4e-3 / atol 1e-3 by {r['rec']['layernorm_stage_excess']}"
    _assert_output_elementwise(name, r)
    _assert_free_running(name, r)
    if r0 is not None:
        assert r0["drawn"] == [] and r0["rec"].get("layernorm_stage_excess", 0.0) <= 0
        _assert_output_elementwise(name + "@p0", r0)
        _assert_free_running(name + "@p0", r0)


def test_engine_dropout_is_exact_both_ways(dev, state):
    from toist_amd import engine
    M, D, seed = 130, 256, 9
    g = torch.Generator().manual_seed(3)
    x, g_out = _rows(g, M, D), _rows(g, M, D)
    case = dict(params=OrderedDict(), inputs=OrderedDict(x=x), body=lambda dev_: (lambda tape, ps, xv: ([engine.dropout(tape, xv)], None)))
    got, drawn = _device_run(case, dev, P, seed, g_out)
    want_seed = next(tr.tape_seeds(seed))
    assert drawn == [want_seed]
    keep = xr.elem_keep(M, D, P, want_seed)
    sc = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(P))
    for n, src in (("out", x), ("x", g_out)):
        want = torch.where(keep, (src.float() * sc).to(BF), torch.zeros((), dtype=BF))
        assert torch.equal(got[n].to(BF).view(torch.int16), want.view(torch.int16)), n


# ------------------------------------------------------------------------------------------------------------------ programs
TEXT = dict(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, max_position_embeddings=64)


@pytest.fixture(scope="module")
def model(dev):
    """Transformer(d 256, 8 heads, 2 encoder layers, FFN 512) around a tiny RoBERTa; every parameter random (biases and LayerNorm affines too), matrices
    bf16-representable"""
    from toist_amd import transformer
    orig = transformer.roberta_config
    transformer.roberta_config = lambda **kw: orig(**dict(TEXT, **kw))
    try:
        torch.manual_seed(0)
        m = transformer.Transformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=1, dim_feedforward=512, dropout=P)
    finally:
        transformer.roberta_config = orig
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, q in m.named_parameters():
            if "embeddings" in n and q.dim() == 2:
                q.copy_(torch.randn(q.shape, generator=g))
            elif q.dim() == 2:
                q.copy_(_w(g, *q.shape))
            elif n.endswith("weight"):
                q.copy_(_gamma(g, q.numel()))
            else:
                q.copy_(_b(g, q.numel()))
    return m.to(dev).train()


def _program_check(name, route, p, got, ref_fn, leaves, g_out, used, drawn, zero_rows=()):
    """reports, then asserts the seed count and the free-running rule; returns the tensors whose bound is loose (e_model > 2 %)"""
    ref = tr.run(lambda lv, rs: ref_fn(lv, rs), leaves, g_out)
    mod = tr.run(lambda lv, rs: ref_fn(lv, rs), leaves, g_out, round_stores=True)
    for n, row in zero_rows:                # nn.Embedding(padding_idx): the padding row never receives a gradient
        ref[n][row] = 0
        mod[n][row] = 0
    e = tr.errors(mod, ref, FLOOR)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    meas = tr.errors(got, ref, FLOOR)
    r3 = lambda v: float("%.3e" % v)
    loose = sorted(n for n, v in e.items() if v > 2e-2)
    _report(name if p > 0 else name + "@p0", {"p": p, "route": route, "e_model": {n: r3(v) for n, v in e.items()}, "device": {n: r3(v) for n, v in meas.items()},
                                              "seeds_drawn": len(drawn), "loose": loose})
    assert drawn == used, f"{name}: the tape drew {len(drawn)} seeds, the reference consumed {len(used)} ({tr.route_sites(route, 2)})"
    bad = {n: (m, 3 * e[n] + 1e-3) for n, m in meas.items() if not m <= 3 * e[n] + 1e-3}
    assert not bad, f"{name} p={p}: relF against fp64 autograd beyond 3 e_model + 1e-3: {bad}"
    return loose


def _encoder_route(dev, model, route, p):
    from toist_amd import engine, tlayer
    B, S, d, H, L = 2, 40, 256, 8, 2
    g = torch.Generator().manual_seed(40)
    x, pos, g_out = _rows(g, B * S, d), _rows(g, B * S, d), _rows(g, B * S, d)
    key_pad = _tail_pad(B, S)
    tlayer.ENABLED, engine.FUSED_BLOCKS = {"tlayer.encoder_program": (True, True), "per_op_encoder": (False, False)}[route]
    assert tlayer.supported(d, H, S) == (route == "tlayer.encoder_program")
    model.zero_grad(set_to_none=True)
    seed = model._step + 1
    xd = x.to(dev).requires_grad_(True)
    model.dropout = p
    try:
        with _count_seeds() as drawn:
            out = model.encode_tokens(xd, pos.to(dev), key_pad.to(dev), B, S)
            (out.float() * g_out.to(dev).float()).sum().backward()
            torch.cuda.synchronize()
    finally:
        model.dropout = P
    got = {"out": out.detach().double().cpu(), "x": xd.grad.double().cpu()}
    got.update({n: q.grad.double().cpu() for n, q in model.encoder.named_parameters() if q.grad is not None})
    masks, used = tr.route_masks(route, L, seed, p, B=B, S=S, H=H, d=d, ff=512) if p > 0 else ({}, [])
    leaves = {n: q.detach().cpu() for n, q in model.encoder.named_parameters()}
    leaves["x"] = x
    fn = lambda lv, rs: tr.encoder_program(lv, lv["x"], pos.double(), key_pad.bool(), B, S, H, L, p, masks, "flash", rs)
    return _program_check("encode_tokens/" + route, route, p, got, fn, leaves, g_out, used, drawn)


@pytest.mark.parametrize("route", ["tlayer.encoder_program", "per_op_encoder"])
def test_encoder_program_with_dropout(dev, state, model, route):
    if _encoder_route(dev, model, route, P):          # loose at p = 0.1 (ReLU gates flipped by a rounding): the same program at p = 0
        _encoder_route(dev, model, route, 0.0)


def _text_route(dev, model, p):
    from toist_amd import engine
    B, L, H = 3, 11, TEXT["num_attention_heads"]
    g = torch.Generator().manual_seed(41)
    ids = torch.randint(2, TEXT["vocab_size"], (B, L), generator=g)
    att = torch.ones(B, L, dtype=torch.int64)
    for b in range(1, B):
        att[b, L - 2 * b:] = 0
        ids[b, L - 2 * b:] = 1
    g_out = _rows(g, B * L, 256)
    engine.FUSED_BLOCKS = True
    model.zero_grad(set_to_none=True)
    seed = model._step + 1
    cfg = model.text_encoder.config
    cfg.hidden_dropout_prob = p
    try:
        with _count_seeds() as drawn:
            out, _ = model.encode_text({"input_ids": ids.to(dev), "attention_mask": att.to(dev)})
            (out.float() * g_out.to(dev).float()).sum().backward()
            torch.cuda.synchronize()
    finally:
        cfg.hidden_dropout_prob = P
    named = OrderedDict(("text_encoder." + n, q) for n, q in model.text_encoder.named_parameters())
    named.update(("resizer." + n, q) for n, q in model.resizer.named_parameters())
    got = {"out": out.detach().double().cpu()}
    got.update({n: q.grad.double().cpu() for n, q in named.items() if q.grad is not None})
    masks, used = tr.route_masks("text", 2, seed, p, B=B, S=L, H=H, d=TEXT["hidden_size"], d_out=256) if p > 0 else ({}, [])
    leaves = {n: q.detach().cpu() for n, q in named.items() if "pooler" not in n}
    fn = lambda lv, rs: tr.text_program(lv, ids, att, H, 1e-12, 2, p, masks, round_stores=rs)
    zero = (("text_encoder.embeddings.word_embeddings.weight", 1), ("text_encoder.embeddings.position_embeddings.weight", 1))
    return _program_check("encode_text", "text", p, got, fn, leaves, g_out, used, drawn, zero_rows=zero)


def test_text_program_with_dropout(dev, state, model):
    if _text_route(dev, model, P):
        _text_route(dev, model, 0.0)
