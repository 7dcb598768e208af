"""The two launches behind the mask program's backward over (image, caption) pairs, called directly through toist_amd.kernels: resize_add_rows_pairs
and sum_maps_by_image (csrc/segm.hip).  Every assertion is bit equality: the first adds two bf16 values in fp32 and rounds once, the second is a
sequential fp32 sum in ascending pair and map order, rounded once.  n_images = 3, Q = 3 and the table [2, 0, 2, 0, 2]: unsorted, image 1 without a
pair.  Outputs are pre-poisoned with bf16 NaN patterns; the image arrays of the bad-entry cases sit between guard images, so an entry used as an
index would read valid memory and fail BY VALUE.
(The file sorts behind every older GPU test file on purpose: DESIGN 8 item 6.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
N_IMAGES, Q = 3, 3
TABLE = [2, 0, 2, 0, 2]
P = len(TABLE)
BAD_TABLE = [2, 0, 3, 0, -1]                               # pair 2 names image n_images, pair 4 image -1: status = 5
ROWS = [14, 0, 7, 7, 3, 12]                                # pairs 4, 0, 2, 2, 1, 4: a repeat, unsorted, n = 6 is no multiple of Q
SIZES = [(2, 3, 4, 6), (3, 5, 7, 9), (1, 1, 1, 1)]          # an exact doubling (the shift form), a non-doubling (nearest_src), one pixel


def _poisoned(shape, dev):
    return torch.full(shape, 0x7FC1, dtype=torch.int16, device=dev).view(BF16)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


def _table(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _between_guard_images(images, dev, fill=55.0):
    n = images.shape[0]
    big = torch.full((n + 2,) + tuple(images.shape[1:]), fill, dtype=images.dtype, device=dev)
    big[1:n + 1].copy_(images)
    return big[1:n + 1]


# ------------------------------------------------------------------------------------------------------------------ resize_add_rows_pairs
def _nearest(dst, n_in, n_out):
    """F.interpolate(mode="nearest")'s source index, in fp32 as the kernel computes it"""
    s = np.floor(np.arange(dst, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64)
    return torch.from_numpy(np.minimum(s, n_in - 1))


def _resize_case(C, H, W, OH, OW, seed=0):
    g = torch.Generator().manual_seed(seed + C + 7 * OH)
    inp = torch.randn(len(ROWS), H, W, C, generator=g).to(BF16)
    fpn = torch.randn(N_IMAGES, OH, OW, C, generator=g).to(BF16)
    return inp, fpn


def _resize_host(inp, fpn, rows, table, OH, OW):
    """the definition: fp32 add of two bf16 values, one rounding; a refused pair's image term is zero"""
    H, W = inp.shape[1:3]
    ys, xs = _nearest(OH, H, OH), _nearest(OW, W, OW)
    if (OH, OW) == (2 * H, 2 * W):
        assert torch.equal(ys, torch.arange(OH) // 2) and torch.equal(xs, torch.arange(OW) // 2)
    out = inp.float()[:, ys][:, :, xs]
    for i, r in enumerate(rows):
        pair = r // Q
        img = table[pair] if 0 <= pair < len(table) else -1
        if 0 <= img < fpn.shape[0]:
            out[i] += fpn[img].float()
    return out.to(BF16)


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("C", [8, 16, 64])
def test_resize_add_rows_pairs_is_the_host_formula_and_resize_add_on_the_gathered_term(dev, C, hw):
    from toist_amd import kernels as k
    H, W, OH, OW = hw
    inp, fpn = _resize_case(C, *hw)
    want = _resize_host(inp, fpn, ROWS, TABLE, OH, OW)
    rows = torch.tensor(ROWS, dtype=torch.int64, device=dev)
    assert k.sweep_check(raise_on_failure=False) == 0
    out = _poisoned((len(ROWS), OH, OW, C), dev)
    k.resize_add_rows_pairs(inp.to(dev), fpn.to(dev), rows, _table(TABLE, dev), len(ROWS), Q, H, W, OH, OW, C, out)
    old = _poisoned((len(ROWS), OH, OW, C), dev)
    k.resize_add(inp.to(dev), fpn[torch.tensor(TABLE)].contiguous().to(dev), rows, len(ROWS), Q, H, W, OH, OW, C, old)      # image p = fpn[table[p]]
    torch.cuda.synchronize()
    assert _bits_equal(out, want), "the host formula, bit for bit"
    assert _bits_equal(out, old), "toist_resize_add(rows=) on fpn[pair_image], bit for bit"
    assert k.sweep_check(raise_on_failure=False) == 0


@pytest.mark.parametrize("hw", SIZES[:2], ids=lambda v: "x".join(map(str, v)))
def test_resize_add_rows_pairs_a_bad_entry_is_never_an_index(dev, hw):
    from toist_amd import kernels as k
    H, W, OH, OW = hw
    C = 16
    inp, fpn = _resize_case(C, *hw)
    want = _resize_host(inp, fpn, ROWS, BAD_TABLE, OH, OW)
    alone = _resize_host(inp, torch.zeros_like(fpn), ROWS, TABLE, OH, OW)                    # `in` resized alone
    rows = torch.tensor(ROWS, dtype=torch.int64, device=dev)
    assert k.sweep_check(raise_on_failure=False) == 0
    out = _poisoned((len(ROWS), OH, OW, C), dev)
    k.resize_add_rows_pairs(inp.to(dev), _between_guard_images(fpn, dev), rows, _table(BAD_TABLE, dev), len(ROWS), Q, H, W, OH, OW, C, out)
    torch.cuda.synchronize()
    assert int(k.sweep_status(dev).item()) == 5
    assert k.sweep_check(raise_on_failure=False) == 5 and k.sweep_check(raise_on_failure=False) == 0
    assert _bits_equal(out, want)
    refused = [i for i, r in enumerate(ROWS) if r // Q in (2, 4)]
    assert refused == [0, 2, 3, 5]
    for i in refused:
        assert _bits_equal(out[i], alone[i]), i
    # a map index outside the P * Q maps is no index into the table either
    far = torch.tensor([P * Q + 1, -2, 4], dtype=torch.int64, device=dev)
    out = _poisoned((3, OH, OW, C), dev)
    k.resize_add_rows_pairs(inp[:3].contiguous().to(dev), _between_guard_images(fpn, dev), far, _table(TABLE, dev), 3, Q, H, W, OH, OW, C, out)
    torch.cuda.synchronize()
    assert k.sweep_check(raise_on_failure=False) == P + 1
    assert _bits_equal(out[:2], alone[:2]) and _bits_equal(out[2], _resize_host(inp[2:3], fpn, [4], TABLE, OH, OW)[0])


# ------------------------------------------------------------------------------------------------------------------ sum_maps_by_image
def _sum_host(x, seg, table, n_images, q):
    """the definition: per image an fp32 accumulator, pairs in ascending order, a pair's maps in ascending order, one rounding (host tensors)"""
    rows, per = x.shape
    out = torch.zeros(n_images, per, dtype=torch.float32)
    for p, img in enumerate(table):
        if not 0 <= img < n_images:
            continue
        lo, hi = (p * q, (p + 1) * q) if seg is None else (seg[p], seg[p + 1])
        for s in range(max(lo, 0), min(hi, rows)):
            out[img] += x[s].float()
    return out.to(BF16)


SEG = [0, 2, 2, 7, 7, 11]                                  # pairs 1 and 3 are empty; five maps (one unrolled group + a remainder) and four


@pytest.mark.parametrize("per", [8, 104])
@pytest.mark.parametrize("seg", [None, SEG], ids=["q_maps_per_pair", "segments"])
def test_sum_maps_by_image_is_the_sequential_fp32_sum(dev, seg, per):
    from toist_amd import kernels as k
    rows = P * Q if seg is None else SEG[-1]
    x = torch.randn(rows, per, generator=torch.Generator().manual_seed(per + rows)).to(BF16)
    want = _sum_host(x, seg, TABLE, N_IMAGES, Q)
    assert not bool(want[1].view(torch.int16).any()) and bool(want[0].view(torch.int16).any()) == (seg is None)       # image 1: no pair -> zero bits
    assert bool(want[2].view(torch.int16).any())
    seg_dev = None if seg is None else _table(seg, dev)
    assert k.sweep_check(raise_on_failure=False) == 0
    runs = []
    for _ in range(2):
        out = _poisoned((N_IMAGES, per), dev)
        assert k.sum_maps_by_image(x.to(dev), seg_dev, _table(TABLE, dev), Q, N_IMAGES, per, out) is out
        runs.append(out)
    torch.cuda.synchronize()
    assert _bits_equal(runs[0], want)
    assert not bool(runs[0][1].view(torch.int16).any())
    assert runs[0].data_ptr() != runs[1].data_ptr() and _bits_equal(runs[0], runs[1])
    assert k.sweep_check(raise_on_failure=False) == 0


def test_sum_maps_by_image_skips_and_reports_a_bad_entry(dev):
    from toist_amd import kernels as k
    per = 104
    x = torch.randn(P * Q, per, generator=torch.Generator().manual_seed(5)).to(BF16)
    want = _sum_host(x, None, BAD_TABLE, N_IMAGES, Q)
    assert bool(want[2].view(torch.int16).any()) and not bool(want[1].view(torch.int16).any())
    assert k.sweep_check(raise_on_failure=False) == 0
    buf = torch.full((N_IMAGES + 2, per), 0x7FC1, dtype=torch.int16, device=dev).view(BF16)          # rows -1 and n_images exist: written = seen
    out = buf[1:N_IMAGES + 1]
    k.sum_maps_by_image(x.to(dev), None, _table(BAD_TABLE, dev), Q, N_IMAGES, per, out)
    torch.cuda.synchronize()
    assert k.sweep_check(raise_on_failure=False) == 5
    assert _bits_equal(out, want)
    assert bool((buf[0].view(torch.int16) == 0x7FC1).all()) and bool((buf[-1].view(torch.int16) == 0x7FC1).all())


def _long_case():
    """P = 40 pairs of Q = 1 on 2 images, per = 8, values chosen as tests/test_gpu_zz_pair_train.py::_case_d chooses them: random 8-bit mantissas
    and signs; pair p + 18 (same image) carries the NEGATED values of pair p < 18, and the four pairs without a partner have the smallest magnitude:
    the exact sum of an image is that of its last two pairs.  That test's 5000 terms climb to 2^13 over magnitudes 2^-8 .. 2^8; 40 terms climb far
    less, so the magnitudes span 2^-12 .. 2^12 here -- more than an fp32 accumulator holds beside 8-bit mantissas: what the small terms lose on the
    way depends on the order of the additions."""
    n, half, E = 40, 18, 12
    g = torch.Generator().manual_seed(11)
    mag = torch.exp2(torch.randint(-E, E + 1, (n, 8), generator=g).float()) * (1 + torch.randint(0, 128, (n, 8), generator=g).float() / 128)
    val = mag * (torch.randint(0, 2, (n, 8), generator=g).float() * 2 - 1)
    val[half:2 * half] = -val[:half]
    val[2 * half:] *= torch.exp2(-E - val[2 * half:].abs().log2().floor())
    x = val.to(BF16)
    assert torch.equal(x.float(), val)
    return x, [p % 2 for p in range(n)]


def test_sum_maps_by_image_adds_in_pair_order_over_a_long_table(dev):
    from toist_amd import kernels as k
    x, table = _long_case()
    want = _sum_host(x, None, table, 2, 1)
    exact = torch.zeros(2, 8, dtype=torch.float64).index_add_(0, torch.tensor(table), x.double()).to(BF16)
    assert not _bits_equal(exact, want)                                            # the exactly rounded sum is NOT what the sequential fp32 sum gives
    rev = _sum_host(x.flip(0), None, table[::-1], 2, 1)
    assert not _bits_equal(rev, want)                                              # nor what the descending order gives
    outs = []
    for _ in range(2):
        out = _poisoned((2, 8), dev)
        k.sum_maps_by_image(x.to(dev), None, _table(table, dev), 1, 2, 8, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert _bits_equal(outs[0], want) and _bits_equal(outs[0], outs[1])
    assert k.sweep_check(raise_on_failure=False) == 0


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_bad_arguments(dev):
    import ctypes
    from toist_amd import _lib, kernels as k
    H, W, OH, OW, C = 2, 3, 4, 6, 16
    inp, fpn = _resize_case(C, H, W, OH, OW)
    inp, fpn = inp.to(dev), fpn.to(dev)
    rows, table = torch.tensor(ROWS, dtype=torch.int64, device=dev), _table(TABLE, dev)
    out = _poisoned((len(ROWS), OH, OW, C), dev)
    good = dict(inp=inp, fpn=fpn, rows=rows, pair_image=table, n=len(ROWS), Q=Q, H=H, W=W, OH=OH, OW=OW, C=C, out=out)
    call = lambda **over: k.resize_add_rows_pairs(**{**good, **over})
    for over in (dict(C=12), dict(n=0), dict(Q=0), dict(H=0), dict(OH=1), dict(inp=None), dict(rows=None), dict(out=None), dict(pair_image=None),
                 dict(rows=rows[:5]), dict(rows=rows.to(torch.int32)), dict(pair_image=table.long()), dict(pair_image=table.cpu()), dict(out=out[:5]),
                 dict(inp=inp.transpose(1, 2))):
        with pytest.raises(ValueError):
            call(**over)
    per = 104
    x = torch.randn(P * Q, per).to(BF16).to(dev)
    sums = _poisoned((N_IMAGES, per), dev)
    good = dict(inp=x, seg=None, pair_image=table, Q=Q, n_images=N_IMAGES, per=per, out=sums)
    call = lambda **over: k.sum_maps_by_image(**{**good, **over})
    for over in (dict(per=100), dict(per=0), dict(Q=0), dict(n_images=0), dict(inp=None), dict(out=None), dict(pair_image=None), dict(out=sums[:2]),
                 dict(seg=_table(SEG[:5], dev)), dict(seg=torch.tensor(SEG, dtype=torch.int64, device=dev)), dict(pair_image=table[:0]),
                 dict(inp=x.t())):
        with pytest.raises(ValueError):
            call(**over)
    assert bool((out.view(torch.int16) == 0x7FC1).all()) and bool((sums.view(torch.int16) == 0x7FC1).all())          # nothing was launched
    # the C entry points refuse the same on their own (an error code and a message, no launch)
    lib, null = _lib.lib(), ctypes.c_void_p(None)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    status = k.sweep_status(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    resize = lambda i, f, r, t, o, s, c=C, n=len(ROWS): lib.toist_resize_add_rows_pairs(i, f, r, t, N_IMAGES, P, n, Q, H, W, OH, OW, c, o, s, stream)
    full = (ptr(inp), ptr(fpn), ptr(rows), ptr(table), ptr(out), ptr(status))
    for hole in range(6):
        assert resize(*[null if j == hole else a for j, a in enumerate(full)]) != 0, hole
    assert resize(*full, c=12) != 0 and resize(*full, n=0) != 0
    total = lambda i, t, o, s, per_=per, p=P: lib.toist_sum_maps_by_image(i, null, t, p, Q, N_IMAGES, P * Q, per_, o, s, stream)
    full = (ptr(x), ptr(table), ptr(sums), ptr(status))
    for hole in range(4):
        assert total(*[null if j == hole else a for j, a in enumerate(full)]) != 0, hole
    assert total(*full, per_=100) != 0 and total(*full, p=0) != 0 and total(*full, per_=0) != 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == 0x7FC1).all()) and bool((sums.view(torch.int16) == 0x7FC1).all())
    assert k.sweep_check(raise_on_failure=False) == 0
