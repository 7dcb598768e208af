"""The three kernels behind a task sweep with the mask head, called directly through toist_amd.kernels: mask_stage_fwd_pairs (csrc/maskstage.hip),
resize_add_pairs (csrc/segm.hip) and sweep_gather (csrc/sweep.hip).  A map's image is pair_image[map // Q], a DEVICE table: B = 3 distinct image terms,
Q = 3 and the table [2, 0, 2, 1, 0] -- a repeat, non-monotone, the first and the last image.  The convolution stages are held to the derived bounds
of tests/rounding_bounds.py (reference: mask_stage_ref on fpn_conv = images[table]) AND to bit equality with the existing kernel fed the gathered
term; the resize and the gather are exact.  Every output sits between sentinel guards.  A table entry outside [0, n_images) is never an index: the
image arrays are carved out of a larger allocation with a guard image on each side, so a launch without the check would read valid memory and fail
BY VALUE.  The largest err / bound of each case goes to mask_sweep_kernel_parity.json (committed as profiles/mask_sweep_kernel_parity.json)."""
import pytest
import torch
import torch.nn.functional as F

import rounding_bounds as rb
from rounding_bounds import BF, F32, F64, G

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
PAD = 1024
FILE = "mask_sweep_kernel_parity.json"
TABLE = [2, 0, 2, 1, 0]
B, Q, P = 3, 3, len(TABLE)


def _guarded(shape, dtype, dev, fill=None):
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


def _table(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _between_guard_images(images, dev, fill=55.0):
    """`images` [n, ...] as a slice of a larger allocation with one guard image in front and one behind, both full of `fill`: index -1 and index n are
    valid memory, and what they hold shows in the output of a launch that uses them"""
    n = images.shape[0]
    big = torch.full((n + 2,) + tuple(images.shape[1:]), fill, dtype=images.dtype, device=dev)
    big[1:n + 1].copy_(images)
    return big[1:n + 1]


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(torch.int32) if t.dtype == F32 else t


# ------------------------------------------------------------------------------------------------------------------ mask_stage_fwd_pairs
def _stage_case(stage, H, W):
    """stage_inputs for the 15 maps of 5 pairs; three image terms, the reference's fpn_conv = images[table]"""
    t = rb.stage_inputs(stage, H, W, B=P, Q=Q)
    images = t["fpn_conv"][:B].clone()
    t["fpn_conv"] = images[torch.tensor(TABLE)]
    return t, images


def _launch_stage(k, t, dev, fpn_conv, table=None):
    cin, cout, gn_in, up = rb.STAGES[t["stage"]]
    H, W = t["H"], t["W"]
    N = t["src"].shape[0]
    obuf, out = _guarded((N, H, W, cout), BF, dev)
    sbuf, st = _guarded((N, G, 2), F32, dev)
    dv = lambda x: None if x is None else x.to(dev)
    args = (t["src"].to(dev), dv(t["stats"]), dv(t["gamma"]), dv(t["beta"]), fpn_conv, t["w"].to(dev), None, out, st, N, Q, H, W, cin, cout, cout, gn_in, up)
    if table is None:
        k.mask_stage_fwd(*args)
    else:
        k.mask_stage_fwd_pairs(*args, table)
    torch.cuda.synchronize()
    return out, st, (obuf, sbuf)


@pytest.mark.parametrize("stage,H,W", [(s, h, w) for s in ("lay4", "lay5") for h, w in rb.STAGE_SHAPES[s]], ids=lambda v: str(v))
def test_mask_stage_pairs_elementwise_and_bit_equal_to_the_gathered_term(dev, stage, H, W):
    from toist_amd import kernels as k
    t, images = _stage_case(stage, H, W)
    assert k.sweep_check(raise_on_failure=False) == 0
    out, st, bufs = _launch_stage(k, t, dev, images.to(dev), _table(TABLE, dev))
    old, _, old_bufs = _launch_stage(k, t, dev, t["fpn_conv"].to(dev))
    ref, bound, _ = rb.mask_stage_ref(t)
    case = f"{H}x{W} table {TABLE}"
    r = rb.record("mask_stage_fwd_pairs." + stage, case, rb.ratio(out.cpu().reshape(ref.shape), ref, bound), file=FILE)
    rs = rb.record("mask_stage_fwd_pairs." + stage + ".out_stats", case, rb.ratio(st.cpu(), *rb.stage_stats_ref(out.cpu())), file=FILE)
    _guards_untouched(*bufs, *old_bufs)
    assert r <= 1.0 and rs <= 1.0, (case, r, rs)
    assert torch.equal(_bits(out), _bits(old)), "the same arithmetic as mask_stage_fwd on the gathered term: bit for bit"
    assert k.sweep_check(raise_on_failure=False) == 0


@pytest.mark.parametrize("bad", [-1, B], ids=["minus_one", "n_images"])
@pytest.mark.parametrize("stage", ["lay4", "lay5"])
def test_mask_stage_pairs_a_bad_entry_is_never_an_index(dev, stage, bad):
    from toist_amd import kernels as k
    H, W = 18, 34
    t, images = _stage_case(stage, H, W)
    carved = _between_guard_images(images, dev)
    table = list(TABLE)
    table[3] = bad
    assert k.sweep_check(raise_on_failure=False) == 0
    out, st, bufs = _launch_stage(k, t, dev, carved, _table(table, dev))
    assert int(k.sweep_status(dev).item()) == 4                                  # the refused pair + 1
    zero_term = t["fpn_conv"].clone()
    zero_term[3] = 0
    want, want_st, _ = _launch_stage(k, t, dev, zero_term.to(dev))               # the existing kernel, pair 3's image term zero
    assert torch.equal(_bits(out), _bits(want))                                  # pair 3: the zero-term result; the others unaffected
    assert rb.ratio(st.cpu(), *rb.stage_stats_ref(out.cpu())) <= 1.0
    _guards_untouched(*bufs)
    with pytest.raises(ValueError, match="pair 3"):
        k.sweep_check()
    assert k.sweep_check(raise_on_failure=False) == 0                            # read and cleared


def test_mask_stage_pairs_refuses_bad_shapes(dev):
    from toist_amd import kernels as k
    t, images = _stage_case("lay4", 16, 16)
    cin, cout = 64, 32
    N = t["src"].shape[0]
    out = torch.empty(N, 16, 16, cout, dtype=BF, device=dev)
    st = torch.empty(N, G, 2, dtype=F32, device=dev)
    src, w, fpn, tab = t["src"].to(dev), t["w"].to(dev), images.to(dev), _table(TABLE, dev)
    call = lambda **kw: k.mask_stage_fwd_pairs(kw.get("src", src), None, None, None, kw.get("fpn", fpn), w, None, kw.get("out", out), st, N, Q, 16, 16, cin, cout,
                                               cout, False, kw.get("up", True), kw.get("tab", tab))
    with pytest.raises(ValueError):
        call(tab=tab[:4])                                    # one entry per pair
    with pytest.raises(ValueError):
        call(tab=tab.long())
    with pytest.raises(ValueError):
        call(fpn=fpn[:, :8])                                 # not [n_images, H, W, c_out]
    with pytest.raises(ValueError):
        call(up=False)                                       # out_lay has no image term
    with pytest.raises(ValueError):
        call(out=out[:, :, :, :16])
    with pytest.raises(ValueError):
        call(src=src.transpose(1, 2))


# ------------------------------------------------------------------------------------------------------------------ resize_add_pairs
RESIZE = [((1, 1), (1, 1)), ((4, 6), (8, 12)), ((8, 12), (15, 23)), ((15, 23), (30, 45))]


def _resize_inputs(hw, ohw, C):
    (H, W), (OH, OW) = hw, ohw
    g = torch.Generator().manual_seed(17 * H + 5 * OW + C)
    return torch.randn(P * Q, H, W, C, generator=g).to(BF), torch.randn(B, OH, OW, C, generator=g).to(BF)


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("hw,ohw", RESIZE, ids=lambda v: "x".join(map(str, v)))
def test_resize_add_pairs_is_exact(dev, hw, ohw, C):
    from toist_amd import kernels as k
    (H, W), (OH, OW) = hw, ohw
    inp, images = _resize_inputs(hw, ohw, C)
    gathered = images[torch.tensor(TABLE)]
    obuf, out = _guarded((P * Q, OH, OW, C), BF, dev)
    k.resize_add_pairs(inp.to(dev), images.to(dev), _table(TABLE, dev), P * Q, Q, H, W, OH, OW, C, out)
    wbuf, want = _guarded((P * Q, OH, OW, C), BF, dev)
    k.resize_add(inp.to(dev), gathered.to(dev), None, P * Q, Q, H, W, OH, OW, C, want)
    torch.cuda.synchronize()
    # F.interpolate(mode="nearest") + the FPN term, formed in f32 and rounded once
    up = F.interpolate(inp.to(F32).permute(0, 3, 1, 2), size=(OH, OW), mode="nearest").permute(0, 2, 3, 1)
    ref = (up + gathered.to(F32).repeat_interleave(Q, 0)).to(BF)
    exact = torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(out.cpu()), _bits(ref))
    rb.record("resize_add_pairs", f"{H}x{W}->{OH}x{OW} C{C}", 0.0 if exact else float("inf"), file=FILE)
    _guards_untouched(obuf, wbuf)
    assert torch.equal(_bits(out), _bits(want)), "resize_add on the gathered FPN term"
    assert torch.equal(_bits(out.cpu()), _bits(ref)), "F.interpolate(nearest) + add, rounded once"
    assert k.sweep_check(raise_on_failure=False) == 0


@pytest.mark.parametrize("bad", [-1, B], ids=["minus_one", "n_images"])
@pytest.mark.parametrize("hw,ohw", [((4, 6), (8, 12)), ((8, 12), (15, 23))], ids=lambda v: "x".join(map(str, v)))
def test_resize_add_pairs_a_bad_entry_is_never_an_index(dev, hw, ohw, bad):
    from toist_amd import kernels as k
    (H, W), (OH, OW), C = hw, ohw, 64
    inp, images = _resize_inputs(hw, ohw, C)
    table = list(TABLE)
    table[1] = bad
    assert k.sweep_check(raise_on_failure=False) == 0
    obuf, out = _guarded((P * Q, OH, OW, C), BF, dev)
    k.resize_add_pairs(inp.to(dev), _between_guard_images(images, dev), _table(table, dev), P * Q, Q, H, W, OH, OW, C, out)
    assert int(k.sweep_status(dev).item()) == 2
    zero_term = images[torch.tensor(TABLE)].clone()
    zero_term[1] = 0
    want = torch.empty(P * Q, OH, OW, C, dtype=BF, device=dev)
    k.resize_add(inp.to(dev), zero_term.to(dev), None, P * Q, Q, H, W, OH, OW, C, want)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    _guards_untouched(obuf)
    with pytest.raises(ValueError, match="pair 1"):
        k.sweep_check()
    assert k.sweep_check(raise_on_failure=False) == 0


def test_resize_add_pairs_refuses_bad_shapes(dev):
    from toist_amd import kernels as k
    inp, images = _resize_inputs((4, 6), (8, 12), 32)
    inp, images, tab = inp.to(dev), images.to(dev), _table(TABLE, dev)
    out = torch.empty(P * Q, 8, 12, 32, dtype=BF, device=dev)
    with pytest.raises(ValueError):
        k.resize_add_pairs(inp, images, tab[:3], P * Q, Q, 4, 6, 8, 12, 32, out)
    with pytest.raises(ValueError):
        k.resize_add_pairs(inp, images[:, :, :5], tab, P * Q, Q, 4, 6, 8, 12, 32, out)
    with pytest.raises(ValueError):
        k.resize_add_pairs(inp, images, tab, P * Q, Q, 4, 6, 3, 12, 32, out)           # a target smaller than the source
    with pytest.raises(ValueError):
        k.resize_add_pairs(inp, images, tab, P * Q, 4, 4, 6, 8, 12, 32, out)           # 15 maps are not a multiple of Q = 4
    with pytest.raises(ValueError):
        k.resize_add_pairs(inp, images, tab.cpu(), P * Q, Q, 4, 6, 8, 12, 32, out)


# ------------------------------------------------------------------------------------------------------------------ sweep_gather
ROW_BYTES = [1, 7, 16, 35, 4099, 211200]          # key-padding rows are h * w bytes, lay1 terms h * w * 264 * 2 (211 200 at 20 x 20)


def _gather_case(rows, row_bytes, table, dev, offset=0):
    """src [rows, row_bytes] bytes starting `offset` bytes into its allocation; the poisoned, guarded destination"""
    g = torch.Generator().manual_seed(row_bytes + rows)
    host = torch.randint(1, 256, (rows, row_bytes), generator=g, dtype=torch.int32).to(torch.uint8)
    store = torch.zeros(rows * row_bytes + offset + 16, dtype=torch.uint8, device=dev)
    src = store[offset:offset + rows * row_bytes].view(rows, row_bytes)
    src.copy_(host)
    obuf = torch.full((len(table) * row_bytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    out = obuf[PAD:PAD + len(table) * row_bytes].view(len(table), row_bytes)
    return src, obuf, out


def _byte_guards_untouched(obuf):
    assert bool((obuf[:PAD] == 0xA5).all()) and bool((obuf[-PAD:] == 0xA5).all()), "guard bytes were written"


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_sweep_gather_equals_index_select(dev, row_bytes):
    from toist_amd import kernels as k
    tab = _table(TABLE, dev)
    for offset in (0, 1) if row_bytes < 5000 else (0,):            # an allocation's start, and one byte into it (PAD is a multiple of 16)
        src, obuf, out = _gather_case(B, row_bytes, TABLE, dev, offset)
        got = k.sweep_gather(src, tab, out=out)
        torch.cuda.synchronize()
        assert got is out and torch.equal(out, src.index_select(0, tab.long())), (row_bytes, offset)
        _byte_guards_untouched(obuf)
    assert k.sweep_check(raise_on_failure=False) == 0


def test_sweep_gather_typed_rows_and_more_than_one_trip_of_the_grid(dev):
    """bf16 rows as the mask head passes them ([B, h * w * 264]), and 700 pairs of 4099 bytes: 2.9 M one-byte elements against the 262 144 threads of the
    largest grid, so every thread takes several trips of the stride loop"""
    from toist_amd import kernels as k
    g = torch.Generator().manual_seed(3)
    y = torch.randn(B, 5 * 7 * 264, generator=g).to(BF).to(dev)
    tab = _table(TABLE, dev)
    assert torch.equal(_bits(k.sweep_gather(y, tab)), _bits(y.index_select(0, tab.long())))
    many = torch.randint(0, B, (700,), generator=g).tolist()
    src, obuf, out = _gather_case(B, 4099, many, dev, offset=1)
    k.sweep_gather(src, _table(many, dev), out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, src.index_select(0, torch.tensor(many, device=dev)))
    _byte_guards_untouched(obuf)
    assert k.sweep_check(raise_on_failure=False) == 0


@pytest.mark.parametrize("bad", [-1, B], ids=["minus_one", "n_images"])
@pytest.mark.parametrize("row_bytes", [7, 16, 4100])            # the 1-, 16- and 4-byte element paths
def test_sweep_gather_a_bad_entry_is_never_an_index(dev, row_bytes, bad):
    from toist_amd import kernels as k
    g = torch.Generator().manual_seed(row_bytes)
    images = torch.randint(1, 256, (B, row_bytes), generator=g, dtype=torch.int32).to(torch.uint8)
    src = _between_guard_images(images.to(dev), dev, fill=0x3C)
    table = list(TABLE)
    table[4] = bad
    obuf = torch.full((P * row_bytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    out = obuf[PAD:PAD + P * row_bytes].view(P, row_bytes)
    assert k.sweep_check(raise_on_failure=False) == 0
    k.sweep_gather(src, _table(table, dev), out=out)
    assert int(k.sweep_status(dev).item()) == 5
    assert not bool(out[4].any())                                                 # the refused pair: zeros
    assert torch.equal(out[:4], src.index_select(0, torch.tensor(TABLE[:4], device=dev)))
    _byte_guards_untouched(obuf)
    with pytest.raises(ValueError, match="pair 4"):
        k.sweep_check()
    assert k.sweep_check(raise_on_failure=False) == 0


def test_sweep_gather_refuses_bad_arguments(dev):
    from toist_amd import kernels as k
    src = torch.zeros(B, 8, dtype=torch.uint8, device=dev)
    tab = _table(TABLE, dev)
    with pytest.raises(ValueError):
        k.sweep_gather(src, tab.long())
    with pytest.raises(ValueError):
        k.sweep_gather(src.t(), tab)
    with pytest.raises(ValueError):
        k.sweep_gather(src, tab, out=torch.zeros(P, 9, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        k.sweep_gather(src, tab, out=torch.zeros(P, 8, dtype=torch.int8, device=dev))
