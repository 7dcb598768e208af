"""toist_amd/staging.py on the device: a Staging's round trip, the number of pinned host-to-device copies each table's upload issues (the counts
the tables had when each wrote its own wait / copy / record), and the mailbox with real events.  No model is built."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu


def test_round_trip_through_one_staging_buffer(dev):
    from toist_amd import staging
    st = staging.Staging(torch.zeros(4096, dtype=torch.uint8), dev)
    assert st.pinned and st.host.is_pinned()
    dst = torch.zeros(4096, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(3)
    a, b = (torch.randint(0, 256, (4096,), dtype=torch.uint8, generator=g) for _ in range(2))
    st.open().copy_(a)
    st.upload((dst, st.host))
    aside = dst.clone()
    st.open().copy_(b)                          # waits for the first upload: the device must still receive A
    st.upload((dst, st.host))
    assert torch.equal(aside.cpu(), a) and torch.equal(dst.cpu(), b) and not torch.equal(a, b)
    st.open_np()[:16] = 7                       # the used head alone
    st.upload_head(dst, 16)
    assert dst[:16].cpu().tolist() == [7] * 16 and torch.equal(dst[16:].cpu(), b[16:])


class _PinnedUploads(TorchDispatchMode):
    """Counts aten.copy_ calls from a pinned host tensor to a device tensor."""

    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func is torch.ops.aten.copy_.default and args[0].is_cuda and not args[1].is_cuda and args[1].is_pinned():
            self.count += 1
        return func(*args, **(kwargs or {}))


def _count(call):
    with _PinnedUploads() as mode:
        call()
    torch.cuda.synchronize()
    return mode.count


def test_every_upload_issues_the_copies_it_always_did(dev):
    """Batch 2, at most 2 targets, 16 x 16 images, 8 tokens, one triangle per object.  The expected counts were measured with this test on the commit
    before the tables moved onto staging.Staging."""
    from toist_amd.distill import DistillTables, FillTables
    from toist_amd.harness import SyntheticCaptions
    from toist_amd.matcher import LiveStaticTargets, StaticTargets
    from toist_amd.preprocess import DevicePolygonMasks, DevicePreprocessor, DeviceTargetMasks, PrepPlan
    B, per, Q, K, L = 2, 2, 5, 8, 8
    g = torch.Generator().manual_seed(5)
    sizes = [2, 1]
    targets = [{"boxes": torch.rand(n, 4, generator=g), "masks": torch.rand(n, 16, 16, generator=g) > 0.5, "dataset_name": f"task_{i + 1}_train.json",
                "noun_tokens_positive": [[(8, 16)]] * n} for i, n in enumerate(sizes)]
    pm, tmask = torch.rand(3, K, generator=g), torch.tensor([[6, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]], dtype=torch.int64)
    tok = SyntheticCaptions({"input_ids": torch.arange(B * L).view(B, L) + 3, "attention_mask": torch.ones(B, L, dtype=torch.int64)})
    captions = ["use the something to cut"] * B
    plans = [PrepPlan(16, 16, final=(16, 16))] * B
    images = [np.full((16, 16, 3), 40 * (i + 1), dtype=np.uint8) for i in range(B)]
    tri = [1, 1, 12, 2, 6, 13]
    segs = [[[tri]] * n for n in sizes]
    counts = {}
    bare = [{"boxes": t["boxes"]} for t in targets]
    counts["StaticTargets.load"] = _count(lambda: StaticTargets(B, per, Q, K, dev).load(bare, pm, tmask))
    counts["StaticTargets.load, masks"] = _count(lambda: StaticTargets(B, per, Q, K, dev, mask_hw=(16, 16)).load(targets, pm, tmask))
    counts["LiveStaticTargets.load"] = _count(lambda: LiveStaticTargets(B, per, Q, K, dev).load(bare, pm, tmask, live_tokens=L))
    counts["DistillTables.load"] = _count(lambda: DistillTables(B, L, dev, pronoun_side=True).load(tok, targets, captions))
    rows = np.full((B, 3), -1, dtype=np.int32)
    counts["FillTables.load"] = _count(lambda: FillTables(B, 3, 8, dev).load(rows, rows))
    prep = DevicePreprocessor(dev, max_batch=B, max_src_pixels=B * 16 * 16, max_out_hw=(16, 16))
    counts["DevicePreprocessor.pack"] = _count(lambda: prep.pack(images, plans))
    tm = DeviceTargetMasks(dev, max_batch=B, max_targets_per_image=per, max_src_pixels=B * per * 16 * 32, max_out_hw=(16, 16))
    counts["DeviceTargetMasks.pack"] = _count(lambda: tm.pack([t["masks"] for t in targets], plans))
    poly = DevicePolygonMasks(dev, max_objects=B * per, max_polygons=B * per, max_vertices=3 * B * per, max_hw=(16, 16), max_trace_steps=1 << 12)
    flat = [[tri]] * 3
    counts["DevicePolygonMasks.pack"] = _count(lambda: poly.pack(flat, [(16, 16)] * 3))
    dst = torch.zeros(4 * 16 * 4, dtype=torch.uint8, device=dev)                       # three objects of 16 rows x one word, moved one slot up
    counts["DevicePolygonMasks.rasterise(offsets)"] = _count(lambda: poly.rasterise(dst, offsets=[64, 128, 192]))
    counts["DeviceTargetMasks.pack_polygons"] = _count(lambda: tm.pack_polygons(segs, plans, polygons=poly))
    assert not dst[:64].any() and dst[64:].any()
    assert counts == {"StaticTargets.load": 1, "StaticTargets.load, masks": 2, "LiveStaticTargets.load": 1, "DistillTables.load": 1, "FillTables.load": 1,
                      "DevicePreprocessor.pack": 1, "DeviceTargetMasks.pack": 1, "DevicePolygonMasks.pack": 1, "DevicePolygonMasks.rasterise(offsets)": 1,
                      "DeviceTargetMasks.pack_polygons": 2}, counts


def test_mailbox_on_the_device(dev):
    from toist_amd import matcher, staging
    mail = staging.Mailbox()
    mail.post(torch.zeros(3, dtype=torch.int32, device=dev))
    got = list(mail.drain(wait=True))
    assert len(got) == 1 and got[0].is_pinned() and got[0].tolist() == [0, 0, 0] and len(mail) == 0
    mail.post(torch.zeros(3, dtype=torch.int32))                     # a host tensor: nothing to wait for, nothing queued
    assert len(mail) == 0
    matcher._LSAP_MAIL.clear()                                       # (whatever an earlier test file left in flight is not this test's)
    matcher.check_lsap_status(torch.tensor([0, 1], dtype=torch.int32, device=dev), defer=True)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        matcher.check_lsap_pending()
    matcher.check_lsap_pending()
