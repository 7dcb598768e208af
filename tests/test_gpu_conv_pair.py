"""kernels.conv_pair (csrc/gemm.hip conv_pair_kernel: conv3 of a layer-3 bottleneck + conv1 of the next one in one launch, forward and data
gradient) against the two per-op calls it replaces -- bit for bit -- and, independently, against fp64 CPU math.

Shapes (N, H, W) at C = 256 / 1024: one full 64-row block, a single partial block, two full blocks and a partial one, three full blocks, and
the bench shape (8, 40, 40) = 12 800 rows, the only one where the replaced conv1 / conv3-dgrad call runs on gemm128_kernel and the pair kernel
therefore sums its second product in two accumulators (SPLIT instantiations)."""
import ctypes

import pytest
import torch

from test_gpu_gemm import _close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
C, C4 = 256, 1024
SENTINEL = -77.0
SHAPES = [(1, 8, 8), (1, 5, 7), (2, 9, 9), (3, 8, 8), (8, 40, 40)]


def _guarded(M, width, dev, ld=None):
    """[M, width] view with 64 sentinel rows before and after (and sentinel columns behind every row when ld > width)"""
    buf = torch.full((M + 128, ld or width), SENTINEL, dtype=BF, device=dev)
    return buf, buf[64:64 + M, :width]


def _guards_untouched(buf, M, width):
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + M:] == SENTINEL).all()), "guard rows were written"
    if buf.shape[1] > width:
        assert bool((buf[:, width:] == SENTINEL).all()), "the columns behind a row were written"


def _inputs(shape, dev, seed=0):
    N, H, W = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(dev)
    # randn + 0.6745 is <= 0 for a quarter of the values: the masks matter
    pos = lambda *s: (torch.randn(*s, generator=g) + 0.6745).to(BF).to(dev)
    return dict(a=r(N, H, W, C), w3=r(C4, 1, 1, C, scale=0.05), w1=r(C, 1, 1, C4, scale=0.05), res=r(N, H, W, C4),
                t3=torch.randn(C4, generator=g).to(dev), t1=torch.randn(C, generator=g).to(dev),
                aux_mid=pos(N, H, W, C4), aux_out=pos(N, H, W, C))


def _per_op(t, dgrad):
    from toist_amd import kernels as k, ops
    hw = t["a"].shape[1:3]
    if dgrad:      # a = g1 of block j, res = its g3, aux_mid = its input x; then conv3's data gradient of block j - 1 masked by its a2
        mid = ops.conv2d_dgrad(t["a"], t["w1"], hw, res=t["res"], act=k.ACT_MASK_POS, aux=t["aux_mid"])
        return mid, ops.conv2d_dgrad(mid, t["w3"], hw, act=k.ACT_MASK_POS, aux=t["aux_out"])
    mid = ops.conv2d(t["a"], t["w3"], shift=t["t3"], res=t["res"], act=k.ACT_RELU)
    return mid, ops.conv2d(mid, t["w1"], shift=t["t1"], act=k.ACT_RELU)


def _pair(t, dgrad, mid, out):
    from toist_amd import kernels as k
    M = t["a"].numel() // C
    v = lambda x, w: x if x.dim() == 2 else x.view(M, w)
    if dgrad:
        k.conv_pair(v(t["a"], C), t["w1"].view(C, C4), t["w3"].view(C4, C), v(t["res"], C4), mid, out, dgrad=True,
                    aux_mid=v(t["aux_mid"], C4), aux_out=v(t["aux_out"], C))
    else:
        k.conv_pair(v(t["a"], C), t["w3"].view(C4, C), t["w1"].view(C, C4), v(t["res"], C4), mid, out, shift_mid=t["t3"], shift_out=t["t1"])


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_equals_the_per_op_calls(dev, shape, dgrad):
    t = _inputs(shape, dev)
    M = shape[0] * shape[1] * shape[2]
    ref_mid, ref_out = _per_op(t, dgrad)
    mbuf, mid = _guarded(M, C4, dev)
    obuf, out = _guarded(M, C, dev)
    _pair(t, dgrad, mid, out)
    torch.cuda.synchronize()
    assert torch.equal(mid, ref_mid.view(M, C4)), f"mid differs in {int((mid != ref_mid.view(M, C4)).sum())} of {mid.numel()} elements"
    assert torch.equal(out, ref_out.view(M, C)), f"out differs in {int((out != ref_out.view(M, C)).sum())} of {out.numel()} elements"
    _guards_untouched(mbuf, M, C4)
    _guards_untouched(obuf, M, C)


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
def test_pair_on_views_into_wider_buffers(dev, dgrad):
    """Every leading dimension larger than its row.  The per-op calls (ops.conv2d / ops.conv2d_dgrad) take contiguous tensors only, so the
    comparator is the per-op result on contiguous copies of the same values."""
    shape = (2, 9, 9)
    M = 162
    t = _inputs(shape, dev, seed=1)
    ref_mid, ref_out = _per_op(t, dgrad)
    wide = {}
    for name, width, ld in (("a", C, C + 8), ("res", C4, C4 + 16), ("aux_mid", C4, C4 + 24), ("aux_out", C, C + 40)):
        buf = torch.full((M, ld), SENTINEL, dtype=BF, device=dev)
        buf[:, :width] = t[name].view(M, width)
        wide[name] = buf[:, :width]
    mbuf, mid = _guarded(M, C4, dev, ld=C4 + 32)
    obuf, out = _guarded(M, C, dev, ld=C + 8)
    _pair({**t, **wide}, dgrad, mid, out)
    torch.cuda.synchronize()
    assert torch.equal(mid, ref_mid.view(M, C4)) and torch.equal(out, ref_out.view(M, C))
    _guards_untouched(mbuf, M, C4)
    _guards_untouched(obuf, M, C)


def test_forward_pair_against_fp64(dev):
    """independent of the per-op path: fp64 CPU math on the same bf16 inputs, test_gpu_gemm's bound at K = 256 (mid) and K = 1024 (out)"""
    shape, M = (2, 9, 9), 162
    t = _inputs(shape, dev)
    _, mid = _guarded(M, C4, dev)
    _, out = _guarded(M, C, dev)
    _pair(t, False, mid, out)
    d = lambda x, *s: x.detach().cpu().double().view(*s)
    mid_ref = torch.relu(d(t["a"], M, C) @ d(t["w3"], C4, C).t() + d(t["t3"], C4) + d(t["res"], M, C4))
    _close(mid, mid_ref.float(), 256, "mid")
    out_ref = torch.relu(mid_ref.to(BF).double() @ d(t["w1"], C, C4).t() + d(t["t1"], C))
    _close(out, out_ref.float(), 1024, "out")


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
def test_pair_in_a_captured_graph(dev, dgrad):
    shape, M = (2, 9, 9), 162
    t = _inputs(shape, dev)
    mid = torch.empty(M, C4, dtype=BF, device=dev)
    out = torch.empty(M, C, dtype=BF, device=dev)
    _pair(t, dgrad, mid, out)          # first launch outside the capture (one-time kernel attributes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _pair(t, dgrad, mid, out)
    for seed in (5, 6):
        fresh = _inputs(shape, dev, seed=seed)
        for name in ("a", "res", "aux_mid", "aux_out"):
            t[name].copy_(fresh[name])            # new contents at the captured addresses
        mid.fill_(SENTINEL), out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        ref_mid, ref_out = _per_op(t, dgrad)
        assert torch.equal(mid, ref_mid.view(M, C4)) and torch.equal(out, ref_out.view(M, C)), f"replay with seed {seed}"


def test_refusals(dev):
    from toist_amd import _lib, kernels as k
    M = 64
    t = _inputs((1, 8, 8), dev)
    mid = torch.full((M, C4), SENTINEL, dtype=BF, device=dev)
    out = torch.full((M, C), SENTINEL, dtype=BF, device=dev)

    def desc(**kw):
        d = k.ConvPair()
        d.M, d.C, d.dgrad, d.lda = M, C, 0, C
        d.a, d.w_first, d.w_second, d.res = t["a"].data_ptr(), t["w3"].data_ptr(), t["w1"].data_ptr(), t["res"].data_ptr()
        d.mid, d.out, d.ldr, d.ldmid, d.ldout = mid.data_ptr(), out.data_ptr(), C4, C4, C
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    for what, d, needle in (("NULL res", desc(res=None), "res is required"), ("C = 128", desc(C=128), "bad shape"),
                            ("misaligned a", desc(a=t["a"].data_ptr() + 2), "16-byte aligned"),
                            ("aux in the forward direction", desc(aux_mid=t["aux_mid"].data_ptr()), "belong to the data gradient"),
                            ("no aux in the data gradient", desc(dgrad=1), "needs aux_mid and aux_out")):
        rc = _lib.lib().toist_conv_pair_bf16(ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), k._stream())
        assert rc == _lib.CONSTANTS["TOIST_EINVAL"], what
        assert needle in _lib.last_error(), (what, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((mid == SENTINEL).all()) and bool((out == SENTINEL).all()), "a refused call launched"


class _View:
    """what engine.bottleneck reads of a ParamView: the bf16 compute copy, the fp32 gradient slot (both channels_last), store-once state"""

    def __init__(self, w):
        self.w = w.contiguous(memory_format=torch.channels_last)
        self.g = torch.zeros_like(self.w, dtype=torch.float32, memory_format=torch.channels_last)
        self.fresh, self.written = False, False

    def mark_written(self):
        self.written = True


def _run_stage(dev, paired):
    """three layer-3-shaped bottlenecks (the first with a downsample, stride 1) on (2, 6, 6), forward + backward with a fixed output gradient"""
    from toist_amd import engine, kernels as k
    g = torch.Generator().manual_seed(11)
    r = lambda *s, scale: (torch.randn(*s, generator=g) * scale).to(BF).to(dev)
    blocks = []
    for bi in range(3):
        cin = 512 if bi == 0 else C4
        W = {"conv1": _View(r(C, cin, 1, 1, scale=0.05)), "conv2": _View(r(C, C, 3, 3, scale=0.03)), "conv3": _View(r(C4, C, 1, 1, scale=0.05))}
        bn = {n: (torch.ones(c, device=dev), torch.randn(c, generator=g).to(dev) * 0.1) for n, c in (("bn1", C), ("bn2", C), ("bn3", C4))}
        if bi == 0:
            W["down"] = _View(r(C4, cin, 1, 1, scale=0.05))
            bn["down"] = (torch.ones(C4, device=dev), torch.randn(C4, generator=g).to(dev) * 0.1)
        blocks.append((W, bn))
    x = engine.Var(torch.relu(r(2, 6, 6, 512, scale=1.0)))
    gout = r(2, 6, 6, C4, scale=1.0)
    before = list(k.CONV_PAIR_CALLS)
    tape = engine.Tape(training=True)
    cur, take = x, None
    for bi, (W, bn) in enumerate(blocks):
        give = engine.pair_link(blocks[bi + 1][0]["conv1"], blocks[bi + 1][1]["bn1"][1]) if paired and bi + 1 < len(blocks) else None
        cur = engine.bottleneck(tape, cur, W, bn, 1, bi == 0, True, take=take, give=give)
        take = give
    y = cur.data
    cur.grad = torch.where(y > 0, gout, torch.zeros_like(gout))       # w.r.t. the pre-ReLU sum
    tape.backward()
    torch.cuda.synchronize()
    calls = [b - a for a, b in zip(before, k.CONV_PAIR_CALLS)]
    grads = [W[n].g for W, _ in blocks for n in sorted(W)]
    return y, x.grad, grads, calls


def test_mini_stage_knob_on_equals_knob_off(dev, monkeypatch):
    from toist_amd import kernels as k
    monkeypatch.setattr(k, "CONV_PAIR", 3)       # both directions, whatever the shipped default
    y0, gx0, grads0, calls0 = _run_stage(dev, paired=False)
    y1, gx1, grads1, calls1 = _run_stage(dev, paired=True)
    assert calls0 == [0, 0] and calls1 == [2, 2], (calls0, calls1)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert len(grads0) == len(grads1) == 10
    for i, (a, b) in enumerate(zip(grads0, grads1)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b), f"weight gradient {i}"
