"""The attention cores -- attn2_fwd_kernel (csrc/attn2.hip), the key-owning backward (csrc/attn2_bwd_body.h) and the whole-head text kernels
(csrc/attn_small.hip) -- called directly through toist_amd.kernels against the fp64 references of tests/attn_bounds.py: EVERY output element within
the derived bound, no share of the elements excused, at the shapes that sit on the kernels' seams (the forward's 64-query workgroup, 128-key block and
512-key stage; the backward's 32-key wave, 128-key split, active-wave count and two-group tile deal; attn_small's 16 / 32 / 64-lane row groups), with
key padding that masks a first key, a last key, a block edge, a whole leading block or stage.  The backward is held as a function of ITS inputs: the
context and the row statistics are built on the host, and every share of dq_part is compared on its own.  Operands sit in column slices of packed
buffers with different row pitches; spare columns and rows of the inputs hold NaN (a stray read shows), outputs start as NaN (an unwritten element
fails) and their spare columns and rows must still be NaN afterwards.  tests/test_cpu_attn_bounds.py shows that the bounds hold for a correct
implementation and catch the usual mistakes.  The largest err / bound of each check goes to attn_core_parity.json (attn_bounds.record) before it is
asserted (committed as profiles/attn_core_parity.json)."""
import pytest
import torch

import attn_bounds as ab
from rounding_bounds import BF, F32

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 3                 # spare rows behind every packed buffer


@pytest.fixture(scope="module")
def kern():
    """kernels.SEED_DEV is process-wide: None for this module (the seed-word case sets it itself), restored afterwards"""
    from toist_amd import kernels as k
    seed_dev = k.SEED_DEV
    k.SEED_DEV = None
    yield k
    k.SEED_DEV = seed_dev


class Packed:
    """a [rows + TAIL, width] bf16 buffer full of NaN and named column slices of its first `rows` rows"""

    def __init__(self, dev, rows, width, **cols):
        self.rows, self.buf = rows, torch.full((rows + TAIL, width), NAN, dtype=BF, device=dev)
        self.cols = cols
        self.spare = torch.ones(rows + TAIL, width, dtype=torch.bool)
        for off, n in cols.values():
            self.spare[:rows, off:off + n] = False

    def __getitem__(self, name):
        off, n = self.cols[name]
        return self.buf[:self.rows, off:off + n]

    def put(self, name, value):
        self[name].copy_(value)
        return self

    def untouched(self):
        """every element outside the named slices is still NaN"""
        return bool(torch.isnan(self.buf.cpu()[self.spare]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


# ------------------------------------------------------------------------------------------------------------------ attn2
def a2_buffers(dev, t):
    """q | k, v | ctx | dctx | dq | dk, dv in six packed buffers: row pitches 288, 208, 100, 104, 108 and 200 elements"""
    d, nq, nk = ab.A2_D, t["B"] * t["Sq"], t["B"] * t["Sk"]
    bufs = dict(q=Packed(dev, nq, 3 * d, q=(d, d)).put("q", t["q"]),
                kv=Packed(dev, nk, 2 * d + 16, k=(8, d), v=(d + 16, d)).put("k", t["k"]).put("v", t["v"]),
                ctx=Packed(dev, nq, d + 4, ctx=(4, d)), dctx=Packed(dev, nq, d + 8, dctx=(8, d)).put("dctx", t["dctx"]),
                dq=Packed(dev, nq, d + 12, dq=(4, d)), dkv=Packed(dev, nk, 2 * d + 8, dk=(4, d), dv=(d + 8, d)))
    bufs["key_pad"] = t["key_pad"].to(dev) if t["key_pad"] is not None else None
    return bufs


def a2_forward(k, dev, t, bufs):
    lse = torch.full((t["B"] * t["H"], t["Sq"], 2), NAN, dtype=F32, device=dev)
    k.attn2_fwd(bufs["q"]["q"], bufs["kv"]["k"], bufs["kv"]["v"], bufs["key_pad"], t["B"], t["H"], t["Sq"], t["Sk"], t["dh"], t["scale"], t["p"], t["seed"],
                bufs["ctx"]["ctx"], lse)
    torch.cuda.synchronize()
    return bufs["ctx"]["ctx"].cpu(), lse.cpu()


def a2_backward(k, dev, t, bufs, ctx, lse):
    """from the GIVEN (ctx, lse): -> (list of dq shares, dk, dv) on the host"""
    splits = k.attn2_splits(t["Sk"])
    assert splits == ab.a2_splits(t["Sk"])
    bufs["ctx"].put("ctx", ctx)
    part = torch.full((splits, t["B"] * t["Sq"], ab.A2_D), NAN, dtype=BF, device=dev) if splits > 1 else None
    k.attn2_bwd(bufs["q"]["q"], bufs["kv"]["k"], bufs["kv"]["v"], bufs["ctx"]["ctx"], bufs["dctx"]["dctx"], lse.to(dev), bufs["key_pad"], t["B"], t["H"],
                t["Sq"], t["Sk"], t["dh"], t["scale"], t["p"], t["seed"], bufs["dq"]["dq"] if splits == 1 else None, bufs["dkv"]["dk"], bufs["dkv"]["dv"],
                dq_part=part)
    torch.cuda.synchronize()
    dq = [bufs["dq"]["dq"].cpu()] if splits == 1 else [part[s].cpu() for s in range(splits)]
    if splits > 1:
        assert bufs["dq"].all_nan(), "dq was written although the key count has several splits"
    return dq, bufs["dkv"]["dk"].cpu(), bufs["dkv"]["dv"].cpu()


def a2_untouched(bufs):
    return all(b.untouched() for b in bufs.values() if isinstance(b, Packed))


@pytest.mark.parametrize("Sq,Sk", ab.A2_SHAPES)
def test_attn2_every_element(dev, kern, Sq, Sk):
    """forward: ctx, the row maximum and 1 / row sum; backward from host-built (ctx, lse): every dq share on its own, dk, dv, exactly 0 at padded keys"""
    for case in ab.a2_cases():
        if case[:2] != (Sq, Sk):
            continue
        name = ab.a2_name(*case)
        t = ab.a2_inputs(*case)
        fwd = ab.a2_fwd_ref(t)
        bufs = a2_buffers(dev, t)
        ctx, lse = a2_forward(kern, dev, t, bufs)
        ab.check("attn2_fwd.ctx", name, ctx, *fwd["ctx"])
        ab.check("attn2_fwd.lse_max", name, lse[..., 0], *fwd["lse_max"])
        ab.check("attn2_fwd.lse_rsum", name, lse[..., 1], *fwd["lse_rsum"])
        host_ctx, host_lse = fwd["host"]
        bwd = ab.a2_bwd_ref(t, host_ctx, host_lse)
        dq, dk, dv = a2_backward(kern, dev, t, bufs, host_ctx, host_lse)
        ab.check_parts("attn2_bwd.dq", name, dq, [r for r, _ in bwd["dq"]], [b for _, b in bwd["dq"]])
        ab.check("attn2_bwd.dk", name, dk, *bwd["dk"])
        ab.check("attn2_bwd.dv", name, dv, *bwd["dv"])
        if t["key_pad"] is not None:
            dead = t["key_pad"].bool().view(-1)
            assert float(dk[dead].float().abs().max()) == 0.0 and float(dv[dead].float().abs().max()) == 0.0, f"[{name}] a padded key has a gradient"
        assert a2_untouched(bufs), f"[{name}] a kernel wrote outside its column slices"


POISON = 2.0 ** 100                   # finite: 0 * x = 0


def _same(a, b):
    """the same numbers everywhere (torch.equal: a NaN equals nothing; an exact zero's sign is no part of the value)"""
    return a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_attn2_padded_keys_contribute_exactly_nothing(dev, kern, direction):
    """k and v of every padded key set to 2^100 (their dots with q and dctx stay finite): each output is what it was -- a masked probability is an exact
    zero, not a small number.  (Keys past Sk and the buffers' spare rows and columns hold NaN in every test of this file: those must never be read.)"""
    t = ab.a2_inputs(65, 641, 0.1, "per_image")
    fwd = ab.a2_fwd_ref(t)
    dead = t["key_pad"].bool().view(-1)
    tp = dict(t, k=t["k"].clone(), v=t["v"].clone())
    tp["k"][dead] = POISON
    tp["v"][dead] = POISON
    outs = []
    for tt in (t, tp):
        bufs = a2_buffers(dev, tt)
        if direction == "forward":
            outs.append(a2_forward(kern, dev, tt, bufs))
        else:
            dq, dk, dv = a2_backward(kern, dev, tt, bufs, *fwd["host"])
            outs.append(dq + [dk, dv])
    assert len(outs[0]) == len(outs[1])
    for i, (a, b) in enumerate(zip(*outs)):
        assert _same(a, b), f"{direction} output {i} moved: {int((a != b).sum())} elements"
    if direction == "forward":
        ab.check("attn2_fwd.ctx", "65x641 p=0.1 pad=per_image poisoned", outs[1][0], *fwd["ctx"])


def test_attn2_bad_arguments_launch_nothing(dev, kern):
    """dh != 32, a misaligned row pitch, B * H * Sq * round8(Sk) >= 2^32 (reached through the sizes alone: no buffer of that size exists) and a missing
    dq for one split: an error, and every output still NaN"""
    k = kern
    t = ab.a2_inputs(17, 17, 0.1, "none")
    bufs = a2_buffers(dev, t)
    B, H, d = t["B"], t["H"], ab.A2_D
    q, kk, v, ctx, dctx, dq, dk, dv = bufs["q"]["q"], bufs["kv"]["k"], bufs["kv"]["v"], bufs["ctx"]["ctx"], bufs["dctx"]["dctx"], bufs["dq"]["dq"], bufs["dkv"]["dk"], bufs["dkv"]["dv"]
    lse = torch.full((B * H, 17, 2), NAN, dtype=F32, device=dev)
    part = torch.full((4, B * 17, d), NAN, dtype=BF, device=dev)
    odd = torch.zeros(B * 17, d + 4, dtype=BF, device=dev)[:, :d]            # row pitch 100: not a multiple of 8
    fwd = lambda **kw: k.attn2_fwd(kw.get("q", q), kk, v, None, B, H, kw.get("Sq", 17), kw.get("Sk", 17), kw.get("dh", 32), t["scale"], 0.1, 5, ctx, lse)
    bwd = lambda **kw: k.attn2_bwd(kw.get("q", q), kk, v, ctx, dctx, lse, None, B, H, kw.get("Sq", 17), kw.get("Sk", 17), kw.get("dh", 32), t["scale"], 0.1, 5,
                                   kw.get("dq", dq), dk, dv, dq_part=kw.get("part"))
    big = dict(Sq=1 << 23, Sk=512)                                            # 2 * 3 * 2^23 * 512 = 3 * 2^33
    assert B * H * big["Sq"] * ab.round8(big["Sk"]) >= 1 << 32
    for call, kw, what in ((fwd, dict(dh=16), "head dim"), (bwd, dict(dh=16), "head dim"), (fwd, dict(q=odd), "row strides"), (bwd, dict(q=odd), "row strides"),
                           (fwd, big, "below 2"), (bwd, dict(big, part=part), "below 2"), (bwd, dict(dq=None), "key splits")):
        with pytest.raises(RuntimeError, match=what):
            call(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lse).all()) and bool(torch.isnan(part).all())
    assert all(bufs[n].all_nan() for n in ("ctx", "dq", "dkv")), "a refused call wrote an output"


# ------------------------------------------------------------------------------------------------------------------ attn_small
def as_buffers(dev, t):
    """q | k | v in one packed buffer (k and v 8 columns apart from their neighbours), ctx, dctx and dq | dk | dv in three more"""
    d, n = t["H"] * t["dh"], t["B"] * t["S"]
    bufs = dict(qkv=Packed(dev, n, 3 * d + 16, q=(0, d), k=(d + 8, d), v=(2 * d + 16, d)).put("q", t["q"]).put("k", t["k"]).put("v", t["v"]),
                ctx=Packed(dev, n, d + 4, ctx=(4, d)), dctx=Packed(dev, n, d + 8, dctx=(8, d)).put("dctx", t["dctx"]),
                grads=Packed(dev, n, 3 * d + 12, dq=(4, d), dk=(d + 8, d), dv=(2 * d + 12, d)))
    bufs["key_pad"] = t["key_pad"].to(dev) if t["key_pad"] is not None else None
    bufs["bias"] = [None if t[b] is None else t[b].to(dev) for b in ("bq", "bk", "bv")]
    return bufs


def as_run_and_check(k, dev, t, name, keep=None):
    B, H, S, dh = t["B"], t["H"], t["S"], t["dh"]
    fwd = ab.as_fwd_ref(t, keep)
    bwd = ab.as_bwd_ref(t, fwd["host"], keep)
    bufs = as_buffers(dev, t)
    g = bufs["grads"]
    bq, bk, bv = bufs["bias"]
    stats = torch.full((B * H, S, 2), NAN, dtype=F32, device=dev)
    k.attn_small_fwd(bufs["qkv"]["q"], bufs["qkv"]["k"], bufs["qkv"]["v"], bufs["key_pad"], B, H, S, dh, t["scale"], t["p"], t["seed"], bufs["ctx"]["ctx"], stats,
                     bq=bq, bk=bk, bv=bv)
    k.attn_small_bwd(bufs["qkv"]["q"], bufs["qkv"]["k"], bufs["qkv"]["v"], bufs["key_pad"], B, H, S, dh, t["scale"], t["p"], t["seed"], fwd["host"].to(dev),
                     bufs["dctx"]["dctx"], g["dq"], g["dk"], g["dv"], bq=bq, bk=bk, bv=bv)
    torch.cuda.synchronize()
    stats = stats.cpu()
    ab.check("attn_small_fwd.ctx", name, bufs["ctx"]["ctx"].cpu(), *fwd["ctx"])
    ab.check("attn_small_fwd.stat_max", name, stats[..., 0], *fwd["stat_max"])
    ab.check("attn_small_fwd.stat_rsum", name, stats[..., 1], *fwd["stat_rsum"])
    for out in ("dq", "dk", "dv"):
        ab.check(f"attn_small_bwd.{out}", name, g[out].cpu(), *bwd[out])
    assert all(b.untouched() for b in bufs.values() if isinstance(b, Packed)), f"[{name}] a kernel wrote outside its column slices"


@pytest.mark.parametrize("S", ab.AS_S)
def test_attn_small_every_element(dev, kern, S):
    """ctx and the row statistics; dq, dk, dv from host-built statistics; the projection biases given and absent"""
    for case in ab.as_cases():
        if case[0] == S:
            as_run_and_check(kern, dev, ab.as_inputs(*case), ab.as_name(*case))


def test_attn_small_device_seed_word_carries_past_32_bits(dev, kern):
    """the mask is that of host seed + device word as ONE 64-bit sum: the low words carry into the high one"""
    from oracle.train_ref import small_attn_keep
    seed, word = ab.AS_SEED_WORD
    assert (seed & 0xFFFFFFFF) + word >= 1 << 32
    t = dict(ab.as_inputs(17, 16, 0.5, True, "middle"), seed=seed)
    keep = small_attn_keep(t["B"], t["H"], 17, 0.5, seed + word)
    assert not torch.equal(keep, small_attn_keep(t["B"], t["H"], 17, 0.5, (seed + word) & 0xFFFFFFFF)), "the carry does not show in this mask"
    try:
        kern.SEED_DEV = torch.full((1,), word, dtype=torch.int64, device=dev)
        as_run_and_check(kern, dev, t, "S=17 dh=16 p=0.5 bias=yes pad=middle seed word carries", keep=keep)
    finally:
        kern.SEED_DEV = None
