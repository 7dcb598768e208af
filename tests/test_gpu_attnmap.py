"""toist_attnmap_softmax_fwd / _bwd (csrc/segm.hip: the per-head softmax over the H x W keys of MHAttentionMap, channels-last output) called
directly, element-wise against the fp64 references of tests/rounding_bounds.py.  HW on both sides of the 64-lane wave (1, 63, 64, 65, 130, 300),
row stride ld = HW rounded up to 8 and 8 more, key padding absent / first key / last key / a middle run (never a whole image); padded keys
must be exactly 0, the columns [HW, ld) of dscores exactly 0, the guards around every output untouched.  The largest err / bound per case goes to
mask_head_kernel_parity.json (rounding_bounds.RECORD) before it is asserted."""
import pytest
import torch

import rounding_bounds as rb
from rounding_bounds import BF, F32, F64

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
PAD = 1024


def _guarded(shape, dev):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=BF, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def _guards_untouched(buf):
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), "guard elements were written"


@pytest.mark.parametrize("pad", rb.ATT_PADS)
@pytest.mark.parametrize("extra_ld", [0, 8])
@pytest.mark.parametrize("HW", rb.ATT_HW)
def test_attnmap_softmax_forward_and_backward(dev, HW, extra_ld, pad):
    from toist_amd import kernels as k
    t = rb.attnmap_inputs(HW, extra_ld, pad)
    B, Q, H, ld = t["B"], t["Q"], t["H"], t["ld"]
    case = f"HW{HW} ld{ld} pad {pad}"
    pbuf, prob = _guarded((B * Q, HW, H), dev)
    k.attnmap_softmax_fwd(t["scores"].to(dev), None if t["key_pad"] is None else t["key_pad"].to(dev), B, Q, H, HW, ld, prob)
    dbuf, ds = _guarded((B * Q, H, ld), dev)
    k.attnmap_softmax_bwd(prob, t["dprob"].to(dev), B * Q, H, HW, ld, ds)         # on the device's own probabilities
    torch.cuda.synchronize()
    p = prob.cpu()
    rf = rb.record("attnmap_softmax_fwd", case, rb.ratio(p, *rb.attnmap_fwd_ref(t)))
    rbw = rb.record("attnmap_softmax_bwd", case, rb.ratio(ds, *rb.attnmap_bwd_ref(p, t["dprob"], ld)))
    _guards_untouched(pbuf)
    _guards_untouched(dbuf)
    assert rf <= 1.0 and rbw <= 1.0, (case, rf, rbw)
    if t["key_pad"] is not None:
        assert float(p.to(F32)[t["key_pad"].bool().repeat_interleave(Q, 0)].abs().max()) == 0.0, "a padded key has a non-zero probability"
    assert float(ds.cpu().to(F32)[..., HW:].abs().max() if ld > HW else 0.0) == 0.0, "columns [HW, ld) of dscores are not zero"
