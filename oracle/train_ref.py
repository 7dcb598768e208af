"""Plain fp64 restatements of the TRAIN-MODE sub-layers the programs of toist_amd.engine / tlayer / transformer.py run with dropout on: test
infrastructure, CPU torch, built on oracle/xdec_ref.py (its counter hashes, its bf16 rounding model, relF).  Written from the programs' comments and
oracle/model_ref.py (encoder_layer, roberta), not from the kernels' code; tests/test_cpu_train_ref.py pins it to model_ref at p = 0.

Dropout masks are never drawn here: every function takes them as bool tensors (None = that site does not drop), so a test decides where a mask
comes from.  The masks of the product are functions of (seed, element index):

  elem_keep(M, N, p, seed)            xdec_ref: GEMM epilogues, toist_dropout_bf16, layernorm_bwd dx_drop, rowgemm -- element m * N + n
  attn_keep(BH, Sq, Sk, p, seed)      xdec_ref: the flash-style core (csrc/attn2.hip), 16-bit fields of a pair hash
  softmax_keep(rows, Sk, p, seed)     toist_softmax_fwd / bwd (the per-op core, any head dimension): element row * round8(Sk) + k
  small_attn_keep(B, H, S, p, seed)   csrc/attn_small.hip (the text encoder's whole-head attention): element ((b * H + h) * S + i) * S + j

and the seeds of a program are the draws of engine.Tape.next_seed in program order: tape_seeds(seed) restates the generator, ROUTES lists per
program route which site takes which draw (data, read off the programs: a wrong table makes the device test fail loudly).

Every restatement takes round_stores: the same graph with a straight-through bf16 rounding wherever the product stores a bf16 tensor (and a bf16
rounding of the gradient wherever its backward stores one).  That model only sizes tolerances: e = relF(f(round_stores=True), f()).

Element indices at or above 2^32 are not covered (xdec_ref.hash_u32 handles lower indices only); no tensor of the tests is that large.
"""
import math

import torch

from .xdec_ref import _RoundGrad, _same, _Ste, attn_keep, bf16, elem_keep, hash_u32, relF, st_norm  # noqa: F401  (re-exported for the tests)

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------ masks and seeds
def _thresh(p):
    """(unsigned)(p * 2^32) of a C float p, as xdec_ref.elem_keep forms it"""
    return int(float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0)


def small_attn_keep(B, H, S, p, seed):
    """keep mask [B, H, S, S] of csrc/attn_small.hip: hash of element ((b * H + h) * S + i) * S + j >= (unsigned)(p * 2^32)"""
    idx = torch.arange(B * H * S * S, dtype=torch.int64).view(B, H, S, S)
    return hash_u32(seed, idx) >= _thresh(p)


def softmax_keep(rows, Sk, p, seed):
    """keep mask [rows, Sk] of toist_softmax_fwd / bwd: hash of element row * round8(Sk) + k (the score rows' pitch, not Sk)"""
    ld = (Sk + 7) // 8 * 8
    idx = torch.arange(rows, dtype=torch.int64).view(rows, 1) * ld + torch.arange(Sk, dtype=torch.int64).view(1, Sk)
    return hash_u32(seed, idx) >= _thresh(p)


def tape_seeds(seed):
    """the draws of engine.Tape(training, p, seed).next_seed(), in order"""
    s = seed * 1000003 + 12345
    while True:
        s += 7919
        yield s & 0x7FFFFFFFFFFF


# per program route: the dropout sites in the order the route draws their seeds (`head` once, `layer` per layer, `tail` once) and the mask of the
# attention probabilities ("by_head_dim": the flash-style core at head dimension 32, the per-op softmax kernels otherwise)
_ENC = dict(head=(), layer=("attn", "out", "hidden", "ffn_out"), tail=())
ROUTES = {
    "tlayer.encoder_program": dict(_ENC, attn="flash"),       # engine.flash_core, _ln_fwd (out_proj), _ffn_fwd, _ln_fwd (linear2)
    "per_op_encoder": dict(_ENC, attn="by_head_dim"),         # engine.attention (probabilities, out_proj), linear_chain (hidden, final)
    "text": dict(head=("emb",), layer=("attn", "out", "ffn_out"), tail=("resizer",), attn="small"),   # engine.dropout, text_attention_block, linear_chain (final), engine.dropout
}


def route_sites(route, n_layers):
    r = ROUTES[route]
    return list(r["head"]) + [f"layers.{i}.{s}" for i in range(n_layers) for s in r["layer"]] + list(r["tail"])


def route_masks(route, n_layers, seed, p, B, S, H, d, ff=0, d_out=0):
    """{site: keep mask} of a program of `route` run with engine.Tape(True, p, seed), and the seeds consumed (in order)"""
    kind = ROUTES[route]["attn"]
    if kind == "by_head_dim":
        kind = "flash" if d // H == 32 else "softmax"
    M = B * S
    masks, used = {}, []
    for site, s in zip(route_sites(route, n_layers), tape_seeds(seed)):
        used.append(s)
        what = site.split(".")[-1]
        if what == "attn":
            if kind == "flash":
                masks[site] = attn_keep(B * H, S, S, p, s).view(B, H, S, S)
            elif kind == "softmax":
                masks[site] = softmax_keep(B * H * S, S, p, s).view(B, H, S, S)
            else:
                masks[site] = small_attn_keep(B, H, S, p, s)
        else:
            masks[site] = elem_keep(M, {"hidden": ff, "resizer": d_out}.get(what, d), p, s)
    return masks, used


# ------------------------------------------------------------------------------------------------------------------ building blocks
def _modes(round_stores):
    """(rnd: a stored bf16 tensor, rg: a tensor whose GRADIENT the backward stores as bf16)"""
    return (_Ste.apply, _RoundGrad.apply) if round_stores else (_same, _same)


def drop(t, keep, p):
    """dropout with a given keep mask (None: off)"""
    return t if keep is None else t * keep / (1.0 - p)


def layer_norm(z, gamma, beta, eps):
    mean = z.mean(1)
    rstd = ((z - mean[:, None]) ** 2).mean(1).add(eps).rsqrt()
    return st_norm(z, mean, rstd, gamma, beta)


def _heads(t, B, S, H):
    return t.view(B, S, H, t.shape[1] // H).permute(0, 2, 1, 3)


def attention_core(q, k, v, dead, B, H, Sq, Sk, p, keep, core="flash", round_stores=False):
    """softmax(q k^T / sqrt(dh), padded keys at -inf) -> dropout(keep [B, H, Sq, Sk]) -> P v.  q [B*Sq, d], k / v [B*Sk, d], dead [B, Sk] bool or None.
    core names the rounding model only: "flash" (csrc/attn2.hip, as xdec_ref.st_attn: the exponentials enter P v as bf16, the score gradients are
    bf16), "softmax" (the per-op core: scores, probabilities, dropped-out probabilities and their three gradients are bf16 tensors), "small"
    (csrc/attn_small.hip: nothing between q / k / v and the context is stored)."""
    rnd, rg = _modes(round_stores)
    d = q.shape[1]
    scale = 1.0 / math.sqrt(d // H)
    qh, kh, vh = _heads(q, B, Sq, H), _heads(k, B, Sk, H), _heads(v, B, Sk, H)
    raw = qh @ kh.transpose(-1, -2)
    if core == "softmax":
        raw = rg(rnd(raw * scale)) / scale
    elif core == "flash":
        raw = rg(raw)
    if dead is not None:
        raw = raw.masked_fill(dead.view(B, 1, 1, Sk), float("-inf"))
    m = raw.detach().amax(-1, keepdim=True)
    e = torch.exp((raw - m) * scale)
    l = e.sum(-1, keepdim=True)
    if core == "softmax":
        pu = rg(rnd(drop(rnd(e / l), keep, p)))
        ctx = pu @ vh
    else:
        e = drop(e, keep, 0.0)
        ctx = ((rnd(e) if core == "flash" else e) @ vh) / l / (1.0 - (p if keep is not None else 0.0))
    return ctx.permute(0, 2, 1, 3).reshape(B * Sq, d)


def out_proj_block(ctx, w, b, resid, p, keep, round_stores=False):
    """resid + dropout(ctx w^T + b): the sum is a stored tensor, so are its gradient and the masked branch gradient"""
    rnd, rg = _modes(round_stores)
    return rg(rnd(drop(rg(ctx @ w.t() + b), keep, p) + resid))


def ffn_relu_block(x1, w1, b1, w2, b2, p, keep_h, keep_o, round_stores=False):
    """x1 + dropout(linear2(dropout(relu(linear1(x1)))))  (engine.linear_chain with dropout_after, final_drop and res; tlayer._ffn_fwd + _ln_fwd)"""
    rnd, rg = _modes(round_stores)
    h = rnd(drop(torch.relu(rg(x1 @ w1.t() + b1)), keep_h, p))
    return rg(rnd(drop(rg(h @ w2.t() + b2), keep_o, p) + x1))


def ffn_gelu_block(x1, w1, b1, w2, b2, p, keep_o, round_stores=False):
    """x1 + dropout(linear2(gelu(linear1(x1))))  (engine.linear_chain with a GELU layer and final_drop; exact erf GELU)"""
    rnd, rg = _modes(round_stores)
    h = rnd(torch.nn.functional.gelu(rg(x1 @ w1.t() + b1)))
    return rg(rnd(drop(rg(h @ w2.t() + b2), keep_o, p) + x1))


# ------------------------------------------------------------------------------------------------------------------ layers
def encoder_layer(sd, lp, x, pos, dead, B, S, H, p, masks, core="flash", round_stores=False):
    """Post-norm encoder layer on batch-major rows x [B*S, d] (model_ref.encoder_layer with dropout): q = k = x + pos, v = x; out_proj + dropout +
    residual + norm1; linear1 + ReLU + dropout; linear2 + dropout + residual + norm2.  sd: reference-named fp64 tensors under the prefix lp;
    masks: {"attn" [B, H, S, S], "out" [M, d], "hidden" [M, ff], "ffn_out" [M, d]} (missing / None = no dropout there)."""
    rnd, rg = _modes(round_stores)
    d = x.shape[1]
    W, b = sd[lp + "self_attn.in_proj_weight"], sd[lp + "self_attn.in_proj_bias"]
    xe = rnd(x + pos)
    qk = rg(rnd(xe @ W[:2 * d].t() + b[:2 * d]))
    v = rg(rnd(x @ W[2 * d:].t() + b[2 * d:]))
    ctx = rg(rnd(attention_core(qk[:, :d], qk[:, d:], v, dead, B, H, S, S, p, masks.get("attn"), core, round_stores)))
    z1 = out_proj_block(ctx, sd[lp + "self_attn.out_proj.weight"], sd[lp + "self_attn.out_proj.bias"], x, p, masks.get("out"), round_stores)
    y1 = rnd(layer_norm(z1, sd[lp + "norm1.weight"], sd[lp + "norm1.bias"], 1e-5))
    z2 = ffn_relu_block(y1, sd[lp + "linear1.weight"], sd[lp + "linear1.bias"], sd[lp + "linear2.weight"], sd[lp + "linear2.bias"], p,
                        masks.get("hidden"), masks.get("ffn_out"), round_stores)
    return rnd(layer_norm(z2, sd[lp + "norm2.weight"], sd[lp + "norm2.bias"], 1e-5))


def encoder_program(sd, x, pos, dead, B, S, H, n_layers, p, masks, core="flash", round_stores=False):
    """n_layers encoder layers (Transformer.encode_tokens); masks: {f"layers.{i}.{site}": keep} as route_masks returns them"""
    for i in range(n_layers):
        lp = f"layers.{i}."
        x = encoder_layer(sd, lp, x, pos, dead, B, S, H, p, {n[len(lp):]: m for n, m in masks.items() if n.startswith(lp)}, core, round_stores)
    return x


def roberta_layer(sd, lp, x, dead, B, L, H, eps, p, masks, core="small", round_stores=False):
    """HF RobertaLayer on rows x [B*L, D] (model_ref.roberta's loop body with dropout): biased q / k / v, probability dropout, dense + dropout +
    residual + LayerNorm, GELU intermediate, output dense + dropout + residual + LayerNorm.  masks: {"attn" [B, H, L, L], "out", "ffn_out" [M, D]}.
    The product stores the three projections WITHOUT their biases (they are added when the attention kernel loads them)."""
    rnd, rg = _modes(round_stores)
    q, k, v = (rg(rnd(x @ sd[lp + f"attention.self.{n}.weight"].t()) + sd[lp + f"attention.self.{n}.bias"]) for n in ("query", "key", "value"))
    ctx = rg(rnd(attention_core(q, k, v, dead, B, H, L, L, p, masks.get("attn"), core, round_stores)))
    z = out_proj_block(ctx, sd[lp + "attention.output.dense.weight"], sd[lp + "attention.output.dense.bias"], x, p, masks.get("out"), round_stores)
    x1 = rnd(layer_norm(z, sd[lp + "attention.output.LayerNorm.weight"], sd[lp + "attention.output.LayerNorm.bias"], eps))
    z2 = ffn_gelu_block(x1, sd[lp + "intermediate.dense.weight"], sd[lp + "intermediate.dense.bias"], sd[lp + "output.dense.weight"],
                        sd[lp + "output.dense.bias"], p, masks.get("ffn_out"), round_stores)
    return rnd(layer_norm(z2, sd[lp + "output.LayerNorm.weight"], sd[lp + "output.LayerNorm.bias"], eps))


def embedding_norm(sd, pre, ids, pos_ids, eps, p, keep, round_stores=False):
    """dropout(LayerNorm(word[ids] + type[0] + position[pos_ids])) in front of the text encoder; rows [B*L, D]"""
    rnd, rg = _modes(round_stores)
    e = sd[pre + "embeddings.word_embeddings.weight"][ids.reshape(-1)] + sd[pre + "embeddings.token_type_embeddings.weight"][0] \
        + sd[pre + "embeddings.position_embeddings.weight"][pos_ids.reshape(-1)]
    y = rnd(layer_norm(rg(rnd(e)), sd[pre + "embeddings.LayerNorm.weight"], sd[pre + "embeddings.LayerNorm.bias"], eps))
    return y if keep is None else rg(rnd(drop(rg(y), keep, p)))          # engine.dropout: the masked gradient is a bf16 tensor too


def resizer(sd, pre, x, p, keep, round_stores=False):
    """FeatureResizer behind the text encoder: dropout(LayerNorm_1e-12(x fc^T + b))"""
    rnd, rg = _modes(round_stores)
    r = rg(rnd(x @ sd[pre + "fc.weight"].t() + sd[pre + "fc.bias"]))
    y = rnd(layer_norm(r, sd[pre + "layer_norm.weight"], sd[pre + "layer_norm.bias"], 1e-12))
    return y if keep is None else rg(rnd(drop(rg(y), keep, p)))          # engine.dropout: the masked gradient is a bf16 tensor too


def roberta_position_ids(ids, pad_id):
    keep = ids.ne(pad_id).long()
    return torch.cumsum(keep, dim=1) * keep + pad_id


def text_program(sd, ids, attention_mask, H, eps, n_layers, p, masks, pad_id=1, round_stores=False):
    """Transformer.encode_text: embeddings -> n_layers RoBERTa layers -> resizer; sd holds "text_encoder.*" and "resizer.*"; masks as route_masks
    returns them for the route "text".  Returns rows [B*L, d_model]."""
    B, L = ids.shape
    dead = attention_mask.ne(1)
    x = embedding_norm(sd, "text_encoder.", ids, roberta_position_ids(ids, pad_id), eps, p, masks.get("emb"), round_stores)
    for i in range(n_layers):
        lp = f"layers.{i}."
        x = roberta_layer(sd, f"text_encoder.encoder.layer.{i}.", x, dead, B, L, H, eps, p, {n[len(lp):]: m for n, m in masks.items() if n.startswith(lp)},
                          "small", round_stores)
    return resizer(sd, "resizer.", x, p, masks.get("resizer"), round_stores)


# ------------------------------------------------------------------------------------------------------------------ reference runs
def run(fn, leaves, g_out, round_stores=False):
    """fn(leaves: {name: fp64 leaf}, round_stores) -> output; returns {"out": output, name: d <output, g_out> / d leaf} (a leaf the output does not
    depend on has no entry)"""
    lv = {n: t.detach().clone().to(F64).requires_grad_(True) for n, t in leaves.items()}
    out = fn(lv, round_stores)
    (out * g_out.to(F64)).sum().backward()
    res = {"out": out.detach()}
    res.update({n: t.grad for n, t in lv.items() if t.grad is not None})
    return res


def errors(got, ref, floor=0.0):
    """{name: relF(got[name], ref[name])} over the reference's tensors (xdec_ref.relF; floor: its rule for an exactly zero reference)"""
    return {n: relF(got[n].to(F64), r, floor) for n, r in ref.items()}
