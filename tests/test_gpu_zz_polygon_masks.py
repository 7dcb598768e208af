"""Polygon annotations rasterised on the device (csrc/poly.hip: toist_polygon_masks through preprocess.DevicePolygonMasks) against the host function
they replace: coco_eval.polygon_to_mask, and convert_coco_poly_to_mask where an object is the union of several polygons.  Equality is exact: packed
bits, pad bits, the bytes around them; dense bytes; from a replayed graph; through DeviceTargetMasks.pack_polygons into a StaticTargets; in the segm
evaluator's ground-truth planes.  The yardstick runs on the host inside each test.  (The file sorts behind every older GPU test file on purpose:
DESIGN.md section 8 item 6.  No test here builds a captured step or runs a model.)"""
import random

import numpy as np
import pytest
import torch
from test_cpu_polygon_masks import golden_polygons, random_polygon

pytestmark = pytest.mark.gpu

DEGENERATE = [([1, 1, 1, 1], 5, 5), ([2.5, 2.5], 4, 4), ([0, 0, 5, 0, 5, 5, 0, 5], 5, 5), ([0, 0, 4, 4], 6, 6), ([1, 1, 3, 3, 5, 5], 7, 7),
              ([1, 1, 4, 4, 4, 1, 1, 4], 6, 6), ([0.5, 0.5], 1, 1), ([0, 0, 1, 0, 1, 1, 0, 1], 1, 1)]


def _host(polygons, h, w):
    """The yardstick: bool [h, w], polygon_to_mask of one polygon, convert_coco_poly_to_mask (the union) otherwise."""
    from toist_amd.coco_eval import convert_coco_poly_to_mask, polygon_to_mask
    if len(polygons) == 1:
        return polygon_to_mask(polygons[0], h, w)
    if not polygons:
        return np.zeros((h, w), dtype=bool)
    return convert_coco_poly_to_mask([polygons], h, w)[0].numpy().astype(bool)


def _rasteriser(dev, objects, **more):
    from toist_amd.preprocess import DevicePolygonMasks
    caps = dict(max_objects=max(len(objects), 1), max_polygons=max(sum(len(o[0]) for o in objects), 1),
                max_vertices=max(sum(len(p) // 2 for o in objects for p in o[0]), 1), max_hw=(max(o[1] for o in objects), max(o[2] for o in objects)),
                max_trace_steps=1 << 20)
    caps.update(more)
    return DevicePolygonMasks(dev, **caps)


def _check_packed(r, objects, margin=64, wants=None):
    """One pack + one rasterise launch into a 0xFF-filled destination: every live row's bytes are pack_mask_bits(host mask), pad bits included, and
    every other byte is still 0xFF.  -> the host masks."""
    from toist_amd.preprocess import pack_mask_bits
    packed = r.pack([o[0] for o in objects], [(o[1], o[2]) for o in objects])
    dst = torch.full((packed.packed_bytes + margin,), 0xFF, dtype=torch.uint8, device=r.device)
    r.rasterise(dst)
    got = dst.cpu().numpy()
    want_all = np.full_like(got, 0xFF)
    masks = []
    for i, ((polygons, h, w), off) in enumerate(zip(objects, packed.offsets)):
        if h == 0:
            masks.append(None)
            continue
        m = _host(polygons, h, w) if wants is None else wants[i]
        rows = pack_mask_bits(m[None])[0]
        assert rows.shape == (h, 4 * ((w + 31) // 32))
        assert np.array_equal(got[off:off + rows.size].reshape(rows.shape), rows), (i, h, w, polygons)
        want_all[off:off + rows.size] = rows.reshape(-1)
        masks.append(m)
    assert np.array_equal(got, want_all)                                          # nothing outside the live rows is written
    return masks


def test_the_contraction_sensitive_fixture(dev):
    """Every polygon of tests/golden/polygon_masks.npz: the packed bits equal the stored bytes (a fused multiply-add in `ys + s * t` changes them)."""
    cases = golden_polygons()
    objects = [([xy], h, w) for xy, h, w, _ in cases]
    r = _rasteriser(dev, objects)
    packed = r.pack([o[0] for o in objects], [(o[1], o[2]) for o in objects])
    dst = torch.zeros(packed.packed_bytes, dtype=torch.uint8, device=dev)
    got = r.rasterise(dst).cpu().numpy()
    for (xy, h, w, bits), off in zip(cases, packed.offsets):
        assert np.array_equal(got[off:off + bits.size].reshape(bits.shape[1:]), bits[0]), (xy, h, w)
    _check_packed(r, objects)


def test_96_seeded_polygons_in_one_launch(dev):
    rng = random.Random(2024)
    objects = []
    for _ in range(96):
        h, w = rng.randint(5, 130), rng.randint(5, 130)
        objects.append(([random_polygon(rng, h, w)], h, w))
    masks = _check_packed(_rasteriser(dev, objects), objects)
    empty = sum(not m.any() for m in masks)
    partly = 0
    for (polygons, h, w), m in zip(objects, masks):
        a = np.asarray(polygons[0]).reshape(-1, 2)
        partly += bool(((a[:, 0] < 0) | (a[:, 0] > w) | (a[:, 1] < 0) | (a[:, 1] > h)).any() and m.any())
    assert empty >= 2 and partly >= 10, (empty, partly)                          # (15 and 70 with this seed)


def test_degenerate_polygons_an_empty_object_a_dead_slot_and_one_pixel(dev):
    live = ([[1, 1, 6, 1, 6, 5, 1, 5]], 7, 9)
    objects = [([xy], h, w) for xy, h, w in DEGENERATE] + [([], 9, 33), live, ([], 0, 0), live, ([[0, 0, 1, 0, 1, 1, 0, 1]], 1, 1), ([[0.2, 0.2, 0.9, 0.3, 0.5, 0.9]], 1, 1)]
    r = _rasteriser(dev, objects, max_objects=len(objects) + 2)
    masks = _check_packed(r, objects)
    assert not masks[8].any() and masks[9].any() and masks[10] is None and masks[12].all()
    # the same batch as dense bytes: the dead slot, the slots behind the batch and everything outside a live region keep their poison
    out = torch.full((len(objects) + 2, 9, 33), 0xFF, dtype=torch.uint8, device=dev)
    got = r.dense_into(out).cpu().numpy()
    for i, ((polygons, h, w), m) in enumerate(zip(objects, masks)):
        if h:
            assert np.array_equal(got[i, :h, :w], m.astype(np.uint8)), i
        assert (got[i, h:] == 0xFF).all() and (got[i, :, w:] == 0xFF).all(), i
    assert (got[len(objects):] == 0xFF).all()
    listed = r.dense(r.last)
    assert tuple(listed[10].shape) == (0, 0) and listed[9].dtype == torch.bool and np.array_equal(listed[9].cpu().numpy(), masks[9])


def test_an_objects_polygons_are_merged_by_union(dev):
    a, b = [2, 2, 12, 2, 12, 12, 2, 12], [8, 8, 20, 8, 20, 20, 8, 20]
    objects = [([a, b], 24, 40), ([a], 24, 40), ([b], 24, 40)]
    both, ma, mb = _check_packed(_rasteriser(dev, objects), objects)
    assert np.array_equal(both, ma | mb) and (ma & mb).sum() >= 9 and both[(ma & mb)].all()         # the overlap is set: a parity would clear it
    assert not np.array_equal(both, ma ^ mb)


@pytest.mark.parametrize("h", [1, 2])
def test_widths_around_a_word_with_a_polygon_on_the_last_column(dev, h):
    objects = [([[w - 3, 0, w, 0, w, h, w - 3, h]], h, w) for w in (31, 32, 33, 64, 65)]
    masks = _check_packed(_rasteriser(dev, objects, max_hw=(2, 300)), objects)         # (a grid of five strips: most own no word of a row)
    assert all(m[:, -1].all() and not m[:, 0].any() for m in masks)


def test_strip_boundaries_and_the_tallest_plane(dev):
    from toist_amd import kernels
    S, R = kernels.POLYGON_STRIP, kernels.POLYGON_MAX_ROWS
    w = 2 * S + S // 2 + 3                                                       # two and a half strips and a bit
    wide = [2, 1, S, 4, S + 10, 1, 2 * S, 5, 2 * S + 20, 1, w, 3, w, 17, 2 * S, 12, S + 30, 18, S, 11, 20, 18, 0, 10]
    tall = [3, 0, 36, 0, 30, R // 5, 38, 2 * R // 5, 31, 3 * R // 5, 37, 4 * R // 5, 33, R, 5, R, 9, 4 * R // 5, 2, 3 * R // 5, 8, 2 * R // 5, 4, R // 5]
    assert len(wide) == len(tall) == 24
    objects = [([wide], 20, w), ([tall], R, 40)]
    masks = _check_packed(_rasteriser(dev, objects), objects)
    for x in (S - 1, S, 2 * S - 1, 2 * S, w - 1):
        assert masks[0][:, x].any(), x                                           # the mask runs through every strip boundary
    assert masks[1][0].any() and masks[1][R - 1].any() and masks[1][R // 2].any()
    with pytest.raises(ValueError, match="plane holds"):
        _rasteriser(dev, [([tall], R + 1, 40)])


def test_dense_mode_into_a_poisoned_capacity(dev):
    rng = random.Random(11)
    objects = []
    while len(objects) < 10:
        h, w = rng.randint(5, 70), rng.randint(40, 67)
        objects.append(([random_polygon(rng, h, w) for _ in range(rng.randint(1, 2))], h, w))
    objects += [([[1, 1, 65, 1, 65, 4, 1, 4]], 5, 65), ([[1, 1, 66, 1, 66, 4, 1, 4]], 5, 66), ([[1, 1, 67, 0, 67, 5, 1, 4]], 5, 67)]
    r = _rasteriser(dev, objects, max_hw=(70, 67))
    r.pack([o[0] for o in objects], [(o[1], o[2]) for o in objects])
    out = torch.full((len(objects), 70, 67), 0xFF, dtype=torch.uint8, device=dev)          # 67 bytes a row: rows at every alignment
    got = r.dense_into(out).cpu().numpy()
    for i, (polygons, h, w) in enumerate(objects):
        assert np.array_equal(got[i, :h, :w], _host(polygons, h, w).astype(np.uint8)), (i, h, w)
        assert (got[i, h:] == 0xFF).all() and (got[i, :, w:] == 0xFF).all(), i
    assert sum(int(got[i, :o[1], :o[2]].sum()) for i, o in enumerate(objects)) > 500


def test_one_captured_launch_serves_every_pack(dev):
    from toist_amd.preprocess import DevicePolygonMasks, pack_mask_bits
    r = DevicePolygonMasks(dev, max_objects=6, max_polygons=12, max_vertices=400, max_hw=(96, 150), max_trace_steps=1 << 18)
    rng = random.Random(5)

    def batch(sizes, counts):
        return [([random_polygon(rng, h, w) for _ in range(n)], h, w) for (h, w), n in zip(sizes, counts)]
    batches = [batch([(40, 50), (96, 150), (7, 33)], [1, 2, 1]), batch([(96, 150)] * 6, [2, 1, 3, 2, 2, 1]), batch([(12, 140), (64, 64)], [3, 0]),
               batch([(5, 5)], [1])]
    dst = torch.zeros(6 * 96 * 5 * 4 + 64, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        r.pack([o[0] for o in batches[0]], [(o[1], o[2]) for o in batches[0]])
        r.rasterise(dst)                                          # (once eagerly, then the capture of the same launch)
        with torch.cuda.graph(graph, stream=side):
            r.rasterise(dst)
    torch.cuda.current_stream().wait_stream(side)
    for objects in batches[1:]:
        dst.fill_(0xFF)
        packed = r.pack([o[0] for o in objects], [(o[1], o[2]) for o in objects])
        graph.replay()
        got = dst.cpu().numpy()
        want = np.full_like(got, 0xFF)
        for (polygons, h, w), off in zip(objects, packed.offsets):
            rows = pack_mask_bits(_host(polygons, h, w)[None])[0]
            want[off:off + rows.size] = rows.reshape(-1)
        assert np.array_equal(got, want), [(o[1], o[2], len(o[0])) for o in objects]


def _plans():
    from toist_amd.preprocess import PrepPlan
    return {"flip_first_crop_final": PrepPlan(96, 64, flip=True, first=(80, 120), crop=(7, 9, 60, 100), final=(96, 160)),
            "width_33": PrepPlan(33, 20, flip=True, final=(40, 66)), "reduce_5x_flip": PrepPlan(96, 64, flip=True, final=(16, 20)),
            "no_targets": PrepPlan(53, 37, final=(64, 91))}


def test_pack_polygons_fills_a_static_targets_like_the_host_masks(dev):
    """DeviceTargetMasks.pack_polygons + write_into against pack(host-rasterised masks) + write_into on the same plans: a ragged batch with an image
    without targets and mask rows that drop a target.  The bytes of StaticTargets.masks are equal, live slots and dead ones."""
    from toist_amd.coco_eval import convert_coco_poly_to_mask
    from toist_amd.matcher import StaticTargets
    from toist_amd.preprocess import DevicePolygonMasks, DeviceTargetMasks
    plans = _plans()
    rng = random.Random(77)
    order, counts = ["flip_first_crop_final", "no_targets", "reduce_5x_flip", "width_33"], [3, 0, 1, 2]
    batch_plans = [plans[n] for n in order]
    segs = [[[random_polygon(rng, p.height, p.width) for _ in range(rng.randint(1, 2))] for _ in range(n)] for p, n in zip(batch_plans, counts)]
    rows = [torch.tensor([0, 2]), torch.zeros(0, dtype=torch.int64), torch.arange(1), torch.tensor([1, 0])]      # one target dropped, two swapped
    host_masks = [convert_coco_poly_to_mask(s, p.height, p.width) if s else torch.zeros(0, p.height, p.width, dtype=torch.bool) for s, p in zip(segs, batch_plans)]
    assert sum(int(m.sum()) for m in host_masks) > 2000
    mask_hw = (128, 160)
    tm = DeviceTargetMasks(dev, max_batch=4, max_targets_per_image=2, max_src_pixels=6 * 64 * 96, max_out_hw=mask_hw)
    pm = DevicePolygonMasks(dev, max_objects=8, max_polygons=16, max_vertices=600, max_hw=(64, 96), max_trace_steps=1 << 18)

    def filled():
        st = StaticTargets(4, 2, 10, 256, dev, mask_hw=mask_hw)
        st.masks.fill_(0xFF)
        return st
    ref, st = filled(), filled()
    want_packed = tm.pack(host_masks, batch_plans, rows)
    tm.write_into(ref)
    want_dense = [m.cpu() for m in tm.dense(want_packed)]
    tm.blob.fill_(0xFF)                                           # nothing of the host bits is left for the second path to find
    packed = tm.pack_polygons(segs, batch_plans, rows, polygons=pm)
    tm.write_into(st)
    torch.cuda.synchronize()
    assert (packed.slots, packed.counts, packed.sizes) == (want_packed.slots, want_packed.counts, want_packed.sizes) == (5, (2, 0, 1, 2), packed.sizes)
    assert torch.equal(st.masks, ref.masks) and bool((st.masks[5:] == 0xFF).all()) and int(st.masks[:5].max()) == 1
    for got, want in zip(tm.dense(packed), want_dense):
        assert torch.equal(got.cpu(), want)
    assert packed.link_bytes == tm._desc_bytes + 4 * sum(p.final[0] + p.final[1] for p, n in zip(batch_plans, packed.counts) if n) + pm.last.link_bytes
    # single images under each plan, every target kept
    for name in order[:1] + order[2:]:
        p = plans[name]
        s = [[random_polygon(rng, p.height, p.width)] for _ in range(2)]
        ref, st = filled(), filled()
        tm.pack([convert_coco_poly_to_mask(s, p.height, p.width)], [p])
        tm.write_into(ref)
        tm.pack_polygons([s], [p], polygons=pm)
        tm.write_into(st)
        assert torch.equal(st.masks, ref.masks), name
    # refused before anything is copied: the polygons' capacities are checked with the target masks' own
    last = tm.last
    with pytest.raises(ValueError, match="max_trace_steps"):
        tm.pack_polygons([[[[1, 1, 1e6, 1]]]], [plans["width_33"]], polygons=pm)
    with pytest.raises(ValueError, match="mask rows"):
        tm.pack_polygons([s], [p], [torch.tensor([2])], polygons=pm)
    assert tm.last is last


def test_ground_truth_planes_from_device_polygons(dev):
    from toist_amd.coco_eval import CocoGroundTruth, convert_coco_poly_to_mask, polygon_to_mask
    h, w = 60, 83
    rng = random.Random(3)
    rle_mask = polygon_to_mask([10, 10, 50, 12, 40, 50], h, w)
    runs = np.diff(np.concatenate([[0], np.flatnonzero(np.diff(rle_mask.T.reshape(-1).astype(np.int8))) + 1, [h * w]])).tolist()
    anns = [{"id": 1, "image_id": 7, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100.0, "iscrowd": 0, "segmentation": [random_polygon(rng, h, w)]},
            {"id": 2, "image_id": 7, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100.0, "iscrowd": 0,
             "segmentation": [[5, 5, 30, 5, 30, 30, 5, 30], [20, 20, 70, 25, 60, 55, 15, 50]]},
            {"id": 3, "image_id": 7, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100.0, "iscrowd": 0, "segmentation": {"size": [h, w], "counts": runs}}]
    data = {"images": [{"id": 7, "height": h, "width": w}], "annotations": anns}
    want = CocoGroundTruth(data).planes(7, (1,), dev)
    got = CocoGroundTruth(data, polygons_on_device=True).planes(7, (1,), dev)
    assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want) and int((want != 0).sum()) > 0
    free = convert_coco_poly_to_mask([a["segmentation"] for a in anns[:2]], h, w, device=dev)
    assert free.is_cuda and free.dtype == torch.bool and torch.equal(free.cpu(), convert_coco_poly_to_mask([a["segmentation"] for a in anns[:2]], h, w))
    none = convert_coco_poly_to_mask([], h, w, device=dev)
    assert none.is_cuda and tuple(none.shape) == (0, h, w) and none.dtype == torch.uint8
