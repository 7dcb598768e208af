"""Pins oracle/xdec_ref.py, the fp64 decoder stack that tests/test_gpu_xdec_reference.py holds the XCD-resident launches against: it must itself
agree with the project's oracle of the reference model (oracle/model_ref.py decoder_layer), its teacher-forced stages must be the free-running graph cut
at the saved tensors, its rounding model must move every saved tensor by one bf16 ulp at most, and its dropout masks must drop the fraction p."""
import pytest
import torch

from oracle import model_ref
from oracle import xdec_ref as xr

D = xr.D


def _small(B, Q, S, L, p, x0_zero, single_live, seed=0):
    """a small fp64 problem + the reference-compatible state dict of its layers (the cross-attention K / V projections are the test's own)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x0 = torch.zeros(B * Q, D, dtype=torch.float64) if x0_zero else rn(B * Q, D)
    qe = rn(Q, D)
    qpos = qe.unsqueeze(0).expand(B, Q, D).reshape(B * Q, D)
    mem, pos = rn(B * S, D), rn(B * S, D)
    key_pad = torch.zeros(B, S, dtype=torch.uint8)
    key_pad[0, S - 3:] = 1
    key_pad[1, 2] = 1
    if single_live:
        key_pad[B - 1] = 1
        key_pad[B - 1, S // 2] = 0
    layers, sd, kv = [], {}, []
    for l in range(L):
        P = {}
        for w, (n_out, n_in) in (("w_in", (3 * D, D)), ("w_os", (D, D)), ("w_q", (D, D)), ("w_oc", (D, D)), ("w1", (xr.FF, D)), ("w2", (D, xr.FF))):
            P[w] = rn(n_out, n_in) / n_in ** 0.5
        for b_, n in (("b_in", 3 * D), ("b_os", D), ("b_q", D), ("b_oc", D), ("b1", xr.FF), ("b2", D), ("be1", D), ("be3", D), ("be4", D)):
            P[b_] = rn(n) * 0.1
        for g_ in ("g1", "g3", "g4"):
            P[g_] = torch.rand(D, generator=g, dtype=torch.float64) + 0.5
        P["seed"] = [1000 * l + 7 * j + 12345678901 for j in range(6)]
        wkv, bkv = rn(2 * D, D) / D ** 0.5, rn(2 * D) * 0.1
        kv.append(torch.cat([(mem + pos) @ wkv[:D].t() + bkv[:D], mem @ wkv[D:].t() + bkv[D:]], dim=1))
        lp = f"layers.{l}."
        sd.update({lp + "self_attn.in_proj_weight": P["w_in"], lp + "self_attn.in_proj_bias": P["b_in"], lp + "self_attn.out_proj.weight": P["w_os"],
                   lp + "self_attn.out_proj.bias": P["b_os"], lp + "norm1.weight": P["g1"], lp + "norm1.bias": P["be1"],
                   lp + "cross_attn_image.in_proj_weight": torch.cat([P["w_q"], wkv]), lp + "cross_attn_image.in_proj_bias": torch.cat([P["b_q"], bkv]),
                   lp + "cross_attn_image.out_proj.weight": P["w_oc"], lp + "cross_attn_image.out_proj.bias": P["b_oc"], lp + "norm3.weight": P["g3"],
                   lp + "norm3.bias": P["be3"], lp + "linear1.weight": P["w1"], lp + "linear1.bias": P["b1"], lp + "linear2.weight": P["w2"],
                   lp + "linear2.bias": P["b2"], lp + "norm4.weight": P["g4"], lp + "norm4.bias": P["be4"]})
        layers.append(P)
    seq = lambda t, n: t.view(B, n, D).transpose(0, 1)          # [B*n, d] rows (b, i) -> the reference's [n, B, d]
    return dict(B=B, Q=Q, S=S, L=L, p=p, x0=x0, qpos=qpos, kv=torch.cat(kv, dim=1), key_pad=key_pad, layers=layers, sd=sd, tgt=seq(x0, Q), memory=seq(mem, S),
                pos=seq(pos, S), query_pos=seq(qpos, Q))


@pytest.mark.parametrize("x0_zero,single_live", [(True, False), (False, False), (False, True)])
def test_forward_is_the_oracle_decoder_layer_applied_L_times(x0_zero, single_live):
    c = _small(3, 9, 13, 3, 0.0, x0_zero, single_live, seed=1 + x0_zero + 2 * single_live)
    out, _ = xr.forward(c["x0"], c["qpos"], c["kv"], c["key_pad"], c["layers"], 0.0, c["B"], c["Q"], c["S"])
    tgt = c["tgt"]
    for l in range(c["L"]):
        tgt = model_ref.decoder_layer(c["sd"], f"layers.{l}.", tgt, c["memory"], c["pos"], c["query_pos"], c["key_pad"].bool(), 8)
        got = out["y4"][l].view(c["B"], c["Q"], D).transpose(0, 1)
        assert xr.relF(got, tgt) < 1e-10, (l, xr.relF(got, tgt))


def _stages_of(c, out, round_partials):
    B, Q, S = c["B"], c["Q"], c["S"]
    for l, P in enumerate(c["layers"]):
        sv = {n: out[n][l] for n in xr.SAVED}
        x_in = c["x0"] if l == 0 else out["y4"][l - 1]
        xe_in = (xr.bf16 if round_partials else (lambda t: t))(c["x0"] + c["qpos"]) if l == 0 else out["y4e"][l - 1]
        kv_l = (c["kv"][:, l * 512:l * 512 + D], c["kv"][:, l * 512 + D:(l + 1) * 512])
        yield l, sv, xr.layer_stages(sv, x_in, xe_in, c["qpos"], kv_l, c["key_pad"], P, c["p"], B, Q, S, last=False, round_partials=round_partials,
                                     round_probs=round_partials)


def test_layer_stages_is_the_forward_graph_cut_at_the_saved_tensors():
    c = _small(3, 9, 13, 2, 0.1, False, True, seed=5)
    out, _ = xr.forward(c["x0"], c["qpos"], c["kv"], c["key_pad"], c["layers"], c["p"], c["B"], c["Q"], c["S"])
    for l, sv, st in _stages_of(c, out, False):
        assert set(st) == set(xr.SAVED)
        for n in xr.SAVED:
            assert torch.equal(st[n], sv[n]), (l, n, float((st[n] - sv[n]).abs().max()))


def test_round_stores_moves_every_saved_tensor_by_one_bf16_ulp_at_most():
    c = _small(3, 9, 13, 2, 0.1, False, True, seed=6)
    bfr = lambda t: t.to(torch.bfloat16).double()
    c["x0"], c["qpos"], c["kv"] = bfr(c["x0"]), bfr(c["qpos"]), bfr(c["kv"])
    out, _ = xr.forward(c["x0"], c["qpos"], c["kv"], c["key_pad"], c["layers"], c["p"], c["B"], c["Q"], c["S"], round_stores=True)
    moved = 0
    for l, sv, st in _stages_of(c, out, True):
        for n in xr.SAVED:
            if n.startswith(("lse", "mean", "rstd")):        # f32 stores: not rounded by the model
                assert xr.relF(sv[n], st[n]) < 1e-12, (l, n)
                continue
            assert torch.equal(sv[n], bfr(sv[n])), (l, n, "not a bf16 value")
            _, e = torch.frexp(st[n].abs().clamp_min(1e-300))
            ulp = torch.ldexp(torch.ones_like(st[n]), e - 8)          # |v| in [2^(e-1), 2^e): 8 significant bits
            d = (sv[n] - st[n]).abs()
            assert bool((d <= ulp).all()), (l, n, float((d / ulp).max()))
            moved += int((d > 0).sum())
    assert moved > 0


def test_dropout_masks_drop_the_fraction_p():
    for p in (0.1, 0.25):
        for seed in (0x1234567, 0x7FEDCBA987654321):
            for keep in (xr.attn_keep(16, 100, 416, p, seed), xr.attn_keep(24, 30, 17, p, seed), xr.elem_keep(800, 256, p, seed), xr.elem_keep(300, 2048, p, seed)):
                frac = 1.0 - float(keep.float().mean())
                assert abs(frac - p) < 0.01, (p, seed, tuple(keep.shape), frac)
    assert not torch.equal(xr.elem_keep(64, 256, 0.1, 1), xr.elem_keep(64, 256, 0.1, 2))


def test_hash_u32_is_the_32_bit_arithmetic_it_restates():
    """the int64 tensor form against unsigned 32-bit arithmetic in Python integers (the C of csrc/common.h read line by line)"""
    M = 0xFFFFFFFF

    def scalar(seed, idx):
        x = (idx ^ seed) & M
        key = (((seed >> 32) ^ ((seed & M) * 0x9E3779B9)) + (idx >> 32) * 0x85EBCA6B) & M
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M
        x ^= key
        x ^= x >> 15
        x = (x * 0x846CA68B) & M
        x ^= x >> 16
        return x
    idx = [0, 1, 255, 256, 65535, 65536, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 204800 * 2048 - 1]
    for seed in (0, 1, 0xFFFFFFFF, 0x123456789ABCDEF, 0x3FFFFFFFFFFFFFFF):
        got = xr.hash_u32(seed, torch.tensor(idx, dtype=torch.int64)).tolist()
        assert got == [scalar(seed, i) for i in idx], seed


def test_rounding_model_and_reference_run_on_the_smallest_cases():
    """e_model (the reference-only quantity the device test's bounds are made of) exists and is small for the forward outputs"""
    for name in ("a", "b"):
        c = xr.make_case(name)
        ref, mod = xr.run_reference(c), xr.run_reference(c, round_stores=True)
        e = xr.e_model(ref, mod)
        assert set(e) == {"y4", "gx_proj", "gx_res"} | set(xr.GRADS)
        assert all(len(v) == (1 if n.startswith("gx_") else c["L"]) for n, v in e.items())
        assert all(0 < x < 2e-2 for x in e["y4"]), e["y4"]
        if c["key_pad"] is not None:        # padded keys receive an exactly zero gradient
            dead = c["key_pad"].bool().view(-1)
            assert all(float(t[dead].abs().max()) == 0.0 for n in ("dk_c", "dv_c") for t in ref[1][n])


def test_case_h_pads_the_second_image_of_an_xcd_differently_from_the_first():
    """images 8 and 9 share XCDs 0 and 1 with images 0 and 1: a launch that indexed key_pad by the XCD must not get away with it"""
    c = xr.CASES["h"]
    kp = xr.make_key_pad(c["B"], c["S"], c["pad"])
    assert not torch.equal(kp[8], kp[0]) and not torch.equal(kp[9], kp[1])
    assert int(kp[8].sum()) != int(kp[0].sum()) and int(kp[9].sum()) != int(kp[1].sum())
    c = xr.CASES["i"]
    kp = xr.make_key_pad(c["B"], c["S"], c["pad"])
    assert len({int(kp[b].sum()) for b in (0, 8, 16)}) == 3          # case i: three images on XCD 0
