"""Pins oracle/train_ref.py, the fp64 train-mode reference that tests/test_gpu_dropout_parity.py and tests/test_gpu_train_mode_reference.py hold the
dropout paths against: at p = 0 its layers must be the project's oracle of the reference model (oracle/model_ref.py encoder_layer / roberta), its masks
must drop the fraction p at the sizes the device tests use, its seed generator must be engine.Tape's, and its rounding model must round exactly the
tensors it lists, each by one bf16 ulp at most."""
import pytest
import torch

from oracle import model_ref
from oracle import train_ref as tr
from oracle import xdec_ref as xr

F64 = torch.float64


def _rn(g, *s):
    return torch.randn(*s, generator=g, dtype=F64)


def _encoder_sd(g, d, ff, n_layers):
    sd = {}
    for i in range(n_layers):
        lp = f"layers.{i}."
        for n, (o, k) in (("self_attn.in_proj_weight", (3 * d, d)), ("self_attn.out_proj.weight", (d, d)), ("linear1.weight", (ff, d)), ("linear2.weight", (d, ff))):
            sd[lp + n] = _rn(g, o, k) / k ** 0.5
        for n, o in (("self_attn.in_proj_bias", 3 * d), ("self_attn.out_proj.bias", d), ("linear1.bias", ff), ("linear2.bias", d), ("norm1.bias", d), ("norm2.bias", d)):
            sd[lp + n] = _rn(g, o) * 0.1
        for n in ("norm1.weight", "norm2.weight"):
            sd[lp + n] = torch.rand(d, generator=g, dtype=F64) + 0.5
    return sd


def _roberta_sd(g, D, ff, n_layers, vocab=50, max_pos=40):
    sd = {"embeddings.word_embeddings.weight": _rn(g, vocab, D), "embeddings.position_embeddings.weight": _rn(g, max_pos, D),
          "embeddings.token_type_embeddings.weight": _rn(g, 1, D), "embeddings.LayerNorm.weight": torch.rand(D, generator=g, dtype=F64) + 0.5,
          "embeddings.LayerNorm.bias": _rn(g, D) * 0.1}
    for i in range(n_layers):
        lp = f"encoder.layer.{i}."
        for n, (o, k) in (("attention.self.query", (D, D)), ("attention.self.key", (D, D)), ("attention.self.value", (D, D)), ("attention.output.dense", (D, D)),
                          ("intermediate.dense", (ff, D)), ("output.dense", (D, ff))):
            sd[lp + n + ".weight"], sd[lp + n + ".bias"] = _rn(g, o, k) / k ** 0.5, _rn(g, o) * 0.1
        for n in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[lp + n + ".weight"], sd[lp + n + ".bias"] = torch.rand(D, generator=g, dtype=F64) + 0.5, _rn(g, D) * 0.1
    return sd


@pytest.mark.parametrize("core", ["flash", "softmax", "small"])
def test_encoder_layer_without_dropout_is_the_oracle_encoder_layer(core):
    g = torch.Generator().manual_seed(1)
    B, S, H, d, ff, L = 3, 13, 4, 64, 96, 2
    sd = _encoder_sd(g, d, ff, L)
    x, pos = _rn(g, B * S, d), _rn(g, B * S, d)
    dead = torch.zeros(B, S, dtype=torch.bool)
    dead[0, S - 4:] = True
    dead[2, S - 1:] = True
    got = tr.encoder_program(sd, x, pos, dead, B, S, H, L, 0.0, {}, core)
    seq = lambda t: t.view(B, S, d).transpose(0, 1)
    want = seq(x)
    for i in range(L):
        want = model_ref.encoder_layer(sd, f"layers.{i}.", want, seq(pos), dead, H)
    assert xr.relF(seq(got), want) < 1e-10


def test_roberta_layers_without_dropout_are_the_oracle_roberta():
    g = torch.Generator().manual_seed(2)
    B, L, H, D, ff, n = 3, 11, 4, 64, 128, 2
    sd = _roberta_sd(g, D, ff, n)
    ids = torch.randint(2, 50, (B, L), generator=g)
    att = torch.ones(B, L, dtype=torch.int64)
    att[1, L - 3:] = 0
    ids[1, L - 3:] = 1
    want = model_ref.roberta(sd, "", ids, att, H, 1e-12)
    x = tr.embedding_norm(sd, "", ids, tr.roberta_position_ids(ids, 1), 1e-12, 0.0, None)
    for i in range(n):
        x = tr.roberta_layer(sd, f"encoder.layer.{i}.", x, att.ne(1), B, L, H, 1e-12, 0.0, {})
    assert xr.relF(x.view(B, L, D), want) < 1e-10
    # ... and the whole text program is that followed by the oracle's resizer (model_ref.mdetr_encode: linear + LayerNorm eps 1e-12)
    full = {"text_encoder." + k: v for k, v in sd.items()}
    full.update({"resizer.fc.weight": _rn(g, 32, D) / 8, "resizer.fc.bias": _rn(g, 32) * 0.1, "resizer.layer_norm.weight": torch.rand(32, generator=g, dtype=F64) + 0.5,
                 "resizer.layer_norm.bias": _rn(g, 32) * 0.1})
    out = tr.text_program(full, ids, att, H, 1e-12, n, 0.0, {})
    ref = torch.nn.functional.layer_norm(want.view(B * L, D) @ full["resizer.fc.weight"].t() + full["resizer.fc.bias"], (32,), full["resizer.layer_norm.weight"],
                                         full["resizer.layer_norm.bias"], 1e-12)
    assert xr.relF(out, ref) < 1e-10


def test_flash_core_is_the_attention_stage_of_the_decoder_reference():
    """attention_core(core="flash") at 8 heads of 32 is xdec_ref.st_attn (one restatement of the flash-style core's arithmetic and rounding, not two)"""
    g = torch.Generator().manual_seed(3)
    B, Sq, Sk, p, seed = 2, 9, 13, 0.1, 0x123456789
    q, k, v = _rn(g, B * Sq, 256), _rn(g, B * Sk, 256), _rn(g, B * Sk, 256)
    dead = torch.zeros(B, Sk, dtype=torch.bool)
    dead[1, Sk - 5:] = True
    keep = xr.attn_keep(B * 8, Sq, Sk, p, seed).view(B, 8, Sq, Sk)
    for rs in (False, True):
        want, _ = xr.st_attn(q, k, v, dead, B, Sq, Sk, p, seed, xr._Ste.apply if rs else xr._same)
        got = tr.attention_core(q, k, v, dead, B, 8, Sq, Sk, p, keep, "flash", rs)
        assert xr.relF(got, want) < 1e-13


def test_masks_drop_the_fraction_p_at_the_sizes_of_the_device_tests():
    for p in (0.1, 0.25, 0.3):
        for seed in (7, 0x123456789ABC, 0x7FFFFFFFFFFF):
            masks = [tr.small_attn_keep(8, 12, 16, p, seed), tr.small_attn_keep(3, 4, 11, p, seed), tr.small_attn_keep(2, 2, 40, p, seed), tr.small_attn_keep(1, 3, 64, p, seed),
                     tr.softmax_keep(2 * 2 * 33, 52, p, seed), tr.softmax_keep(4 * 100, 17, p, seed), tr.softmax_keep(2 * 2 * 40, 40, p, seed)]
            for keep in masks:
                if keep.numel() < 20000:         # 3 sigma of a binomial fraction is 0.01 at 20000 draws and p = 0.3: the smaller shapes are pooled over seeds
                    fn = tr.small_attn_keep if keep.dim() == 4 else tr.softmax_keep
                    keep = torch.stack([fn(*_args_of(keep), p, seed + 17 * j) for j in range(-(-60000 // keep.numel()))])
                frac = 1.0 - float(keep.double().mean())
                assert abs(frac - p) < 0.01, (p, seed, tuple(keep.shape), frac)
    assert not torch.equal(tr.softmax_keep(64, 52, 0.1, 1), tr.softmax_keep(64, 52, 0.1, 2))
    # the pitch of a score row is round8(Sk): row r of softmax_keep(rows, 52) starts 56 elements after row r - 1, so it is the flat stream read with that stride
    flat = xr.elem_keep(1, 64 * 56, 0.1, 5).view(64, 56)
    assert torch.equal(tr.softmax_keep(64, 52, 0.1, 5), flat[:, :52])
    assert torch.equal(tr.small_attn_keep(2, 3, 5, 0.1, 9).view(-1), xr.elem_keep(1, 2 * 3 * 25, 0.1, 9).view(-1))


def _args_of(keep):
    return tuple(keep.shape[:3]) if keep.dim() == 4 else (keep.shape[0], keep.shape[1])


def test_tape_seeds_are_the_draws_of_the_engine_tape():
    from toist_amd import engine
    for seed in (0, 1, 7, 123456789, 2 ** 40 + 3):
        tape = engine.Tape(True, 0.1, seed)
        gen = tr.tape_seeds(seed)
        assert [next(gen) for _ in range(64)] == [tape.next_seed() for _ in range(64)]


def test_route_tables_name_one_site_per_seed():
    assert tr.route_sites("tlayer.encoder_program", 2) == ["layers.0.attn", "layers.0.out", "layers.0.hidden", "layers.0.ffn_out",
                                                           "layers.1.attn", "layers.1.out", "layers.1.hidden", "layers.1.ffn_out"]
    assert tr.route_sites("text", 2) == ["emb", "layers.0.attn", "layers.0.out", "layers.0.ffn_out", "layers.1.attn", "layers.1.out", "layers.1.ffn_out", "resizer"]
    masks, used = tr.route_masks("text", 2, 5, 0.1, B=3, S=11, H=4, d=128, d_out=256)
    gen = tr.tape_seeds(5)
    assert used == [next(gen) for _ in range(8)] and list(masks) == tr.route_sites("text", 2)
    assert masks["emb"].shape == (33, 128) and masks["layers.1.attn"].shape == (3, 4, 11, 11) and masks["resizer"].shape == (33, 256)
    assert torch.equal(masks["layers.0.attn"], tr.small_attn_keep(3, 4, 11, 0.1, used[1]))
    masks, used = tr.route_masks("per_op_encoder", 1, 5, 0.1, B=2, S=40, H=2, d=128, ff=512)
    assert torch.equal(masks["layers.0.attn"].view(-1, 40), tr.softmax_keep(2 * 2 * 40, 40, 0.1, used[0])) and masks["layers.0.hidden"].shape == (80, 512)
    masks, used = tr.route_masks("per_op_encoder", 1, 5, 0.1, B=2, S=40, H=8, d=256, ff=512)
    assert torch.equal(masks["layers.0.attn"].view(16, 40, 40), xr.attn_keep(16, 40, 40, 0.1, used[0]))


class _Recorder:
    """stands in for xdec_ref._Ste inside oracle.train_ref: records every store of the rounding model"""

    def __init__(self):
        self.stores = []

    def apply(self, x):
        y = xr._Ste.apply(x)
        self.stores.append((x.detach(), y.detach()))
        return y


@pytest.mark.parametrize("what,n_stores", [("encoder_flash", 10), ("encoder_softmax", 12), ("roberta", 9), ("embedding", 3), ("resizer", 3)])
def test_round_stores_rounds_the_listed_tensors_by_one_bf16_ulp_at_most(monkeypatch, what, n_stores):
    g = torch.Generator().manual_seed(4)
    rec = _Recorder()
    monkeypatch.setattr(tr, "_Ste", rec)
    bfr = lambda t: t.to(torch.bfloat16).double()
    B, S, H = 2, 9, 2
    dead = torch.zeros(B, S, dtype=torch.bool)
    dead[1, S - 2:] = True
    if what.startswith("encoder"):
        d, ff = 64, 96
        core = what.split("_")[1]
        sd = _encoder_sd(g, d, ff, 1)
        keep = {"flash": xr.attn_keep(B * H, S, S, 0.1, 3), "softmax": tr.softmax_keep(B * H * S, S, 0.1, 3)}[core].view(B, H, S, S)
        masks = dict(attn=keep, out=xr.elem_keep(B * S, d, 0.1, 4), hidden=xr.elem_keep(B * S, ff, 0.1, 5), ffn_out=xr.elem_keep(B * S, d, 0.1, 6))
        out = tr.encoder_layer(sd, "layers.0.", bfr(_rn(g, B * S, d)), bfr(_rn(g, B * S, d)), dead, B, S, H, 0.1, masks, core, round_stores=True)
    else:
        D, ff = 64, 128
        sd = _roberta_sd(g, D, ff, 1)
        ids = torch.randint(2, 50, (B, S), generator=g)
        if what == "roberta":
            masks = dict(attn=tr.small_attn_keep(B, H, S, 0.1, 3), out=xr.elem_keep(B * S, D, 0.1, 4), ffn_out=xr.elem_keep(B * S, D, 0.1, 6))
            out = tr.roberta_layer(sd, "encoder.layer.0.", bfr(_rn(g, B * S, D)), dead, B, S, H, 1e-12, 0.1, masks, round_stores=True)
        elif what == "embedding":
            out = tr.embedding_norm(sd, "", ids, tr.roberta_position_ids(ids, 1), 1e-12, 0.1, xr.elem_keep(B * S, D, 0.1, 4), round_stores=True)
        else:
            rz = {"fc.weight": _rn(g, 32, D) / 8, "fc.bias": _rn(g, 32) * 0.1, "layer_norm.weight": torch.rand(32, generator=g, dtype=F64) + 0.5, "layer_norm.bias": _rn(g, 32) * 0.1}
            out = tr.resizer(rz, "", bfr(_rn(g, B * S, D)), 0.1, xr.elem_keep(B * S, 32, 0.1, 4), round_stores=True)
    assert len(rec.stores) == n_stores
    assert torch.equal(out, bfr(out))
    moved = 0
    for x, y in rec.stores:
        assert torch.equal(y, bfr(y))
        _, e = torch.frexp(x.abs().clamp_min(1e-300))
        ulp = torch.ldexp(torch.ones_like(x), e - 8)
        assert bool(((y - x).abs() <= ulp).all())
        moved += int(((y - x).abs() > 0).sum())
    assert moved > 0


def test_run_returns_the_gradients_of_the_leaves_and_errors_compares_them():
    g = torch.Generator().manual_seed(5)
    w, x, go = _rn(g, 4, 3), _rn(g, 5, 3), _rn(g, 5, 4)
    ref = tr.run(lambda lv, rs: lv["x"] @ lv["w"].t(), dict(x=x, w=w), go)
    assert set(ref) == {"out", "x", "w"} and xr.relF(ref["x"], go @ w) < 1e-14 and xr.relF(ref["w"], go.t() @ x) < 1e-14
    e = tr.errors({n: t * (1 + 1e-3) for n, t in ref.items()}, ref)
    assert set(e) == set(ref) and all(abs(v - 1e-3) < 1e-9 for v in e.values())
