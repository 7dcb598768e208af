"""The host side of the device polygon rasteriser (csrc/poly.hip: toist_polygon_masks): preprocess.polygon_tables, the three int32 tables the kernel
reads, and a numpy walk of exactly those tables in the kernel's order -- per object, per strip of kernels.POLYGON_STRIP columns, per polygon: XOR the
crossings of the strip, prefix-XOR down the columns, OR into the object's plane -- held against coco_eval.convert_coco_poly_to_mask.  Every capacity
and validation error of DevicePolygonMasks is raised before a buffer is touched.  Equality is exact; CPU only."""
import random

import numpy as np
import pytest
from test_cpu_polygon_masks import golden_polygons, random_polygon

DEGENERATE = [([1, 1, 1, 1], 5, 5), ([2.5, 2.5], 4, 4), ([0, 0, 5, 0, 5, 5, 0, 5], 5, 5), ([0, 0, 4, 4], 6, 6), ([1, 1, 3, 3, 5, 5], 7, 7),
              ([1, 1, 4, 4, 4, 1, 1, 4], 6, 6), ([0.5, 0.5], 1, 1), ([0, 0, 1, 0, 1, 1, 0, 1], 1, 1)]


def walk_tables(verts, polys, desc, strip):
    """What the kernel computes from its tables, in its order and with its integer / fp64 operations: -> list of bool [h, w] (None for a dead slot)."""
    out = []
    for off, h, w, stride, first, count, _, _ in desc.tolist():
        if h == 0:
            out.append(None)
            continue
        mask = np.zeros((h, w), dtype=bool)
        for x0 in range(0, w, strip):
            acc = np.zeros((h, strip), dtype=bool)
            for p in range(first, first + count):
                vf, vn = polys[p].tolist()
                tog = np.zeros((h, strip), dtype=bool)
                for j in range(vn):
                    (xs, ys), (xe, ye) = verts[vf + j].tolist(), verts[vf + (j + 1) % vn].tolist()
                    dx, dy = abs(xe - xs), abs(ys - ye)
                    major_x = dx >= dy
                    flip = (xs > xe) if major_x else (ys > ye)
                    if flip:
                        xs, xe, ys, ye = xe, xs, ye, ys
                    length = dx if major_x else dy
                    if length == 0:
                        continue
                    s = (ye - ys) / dx if major_x else (xe - xs) / dy
                    d = np.arange(1, length + 1, dtype=np.int64)
                    tj, tp = (length - d, length - d + 1) if flip else (d, d - 1)

                    def point(t):
                        if major_x:
                            return t + xs, np.trunc(float(ys) + s * t.astype(np.float64) + .5).astype(np.int64)
                        return np.trunc(float(xs) + s * t.astype(np.float64) + .5).astype(np.int64), t + ys
                    (uj, vj), (up, vp) = point(tj), point(tp)
                    xd = (np.where(uj < up, uj, uj - 1).astype(np.float64) + .5) / 5.0 - .5
                    ok = (uj != up) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= float(w - 1))
                    bx = xd.astype(np.int64)
                    ok &= (bx >= x0) & (bx < x0 + strip)
                    yd = (np.where(vj < vp, vj, vp).astype(np.float64) + .5) / 5.0 - .5
                    by = np.ceil(np.minimum(np.maximum(yd, 0.0), float(h))).astype(np.int64)
                    ok &= by < h
                    np.logical_xor.at(tog, (by[ok], bx[ok] - x0), True)
                acc |= np.logical_xor.accumulate(tog, axis=0)
            mask[:, x0:x0 + strip] = acc[:, :w - x0]
        out.append(mask)
    return out


def _host_union(polygons, h, w):
    from toist_amd.coco_eval import convert_coco_poly_to_mask
    return convert_coco_poly_to_mask([polygons], h, w)[0].numpy().astype(bool)


def seeded_objects():
    """The 320 polygons of tests/test_cpu_polygon_masks.py, regenerated with its seed and grouped 1-3 to an object at the first polygon's image size."""
    rng = random.Random(4711)
    drawn = []
    for _ in range(320):
        h, w = rng.randint(5, 130), rng.randint(5, 130)
        drawn.append((random_polygon(rng, h, w), h, w))
    group, objects, i = random.Random(7), [], 0
    while i < len(drawn):
        n = group.randint(1, 3)
        objects.append(([xy for xy, _, _ in drawn[i:i + n]], drawn[i][1], drawn[i][2]))
        i += n
    return objects


def test_polygon_tables_against_polygon_vertices():
    from toist_amd import _lib
    from toist_amd.coco_eval import polygon_vertices
    from toist_amd.preprocess import polygon_tables
    objects = seeded_objects()[:40] + [([xy], h, w) for xy, h, w in DEGENERATE] + [([], 9, 33), ([], 0, 0)]
    verts, polys, desc, steps = polygon_tables([o[0] for o in objects], [(o[1], o[2]) for o in objects])
    assert verts.dtype == polys.dtype == desc.dtype == np.int32 and desc.shape == (len(objects), _lib.POLY_DESC_WORDS) and polys.shape[1] == 2 and verts.shape[1] == 2
    at_poly = at_vert = at_byte = total = 0
    for (polygons, h, w), row in zip(objects, desc.tolist()):
        if h == 0:
            assert row == [0] * 8                                                     # a dead slot
            continue
        stride = (w + 31) // 32
        assert row == [at_byte, h, w, stride, at_poly, len(polygons), 0, 0]
        at_byte += h * stride * 4
        for xy in polygons:
            v, n = polygon_vertices(xy)
            assert polys[at_poly].tolist() == [at_vert, len(v)]
            want = [[int(5.0 * x + .5), int(5.0 * y + .5)] for x, y in v.tolist()]    # polygon_to_mask's own expression
            assert verts[at_vert:at_vert + len(v)].tolist() == want
            at_poly, at_vert, total = at_poly + 1, at_vert + len(v), total + n
    assert (at_poly, at_vert, total) == (len(polys), len(verts), steps) and steps > 0
    # negative grid values occur, and the offsets can be the caller's
    assert verts.min() < 0
    _, _, d2, _ = polygon_tables([[[1, 1, 3, 1, 3, 3]], [[0, 0, 2, 2]]], [(4, 40), (3, 3)], offsets=[64, 0])
    assert d2[:, 0].tolist() == [64, 0] and d2[:, 3].tolist() == [2, 1]
    empty = polygon_tables([], [])
    assert empty[0].shape == (0, 2) and empty[1].shape == (0, 2) and empty[2].shape == (0, 8) and empty[3] == 0
    for segs, sizes, offsets, what in [([[[1, 2, 3]]], [(4, 4)], None, "even length"), ([[[]]], [(4, 4)], None, "non-empty"), ([[[1, float("nan")]]], [(4, 4)], None, "non-finite"),
                                       ([[[1, 2 ** 31 / 5.0]]], [(4, 4)], None, "int32"), ([[[1, 1]]], [(4, 4), (4, 4)], None, "sizes"),
                                       ([[[1, 1]]], [(0, 0)], None, "dead slot"), ([[]], [(4, 0)], None, "size"), ([[]], [(-1, 4)], None, "size"),
                                       ([[]], [(4, 4)], [2], "offset"), ([[]], [(4, 4)], [-4], "offset"), ([[]], [(4, 4)], [0, 4], "offsets")]:
        with pytest.raises(ValueError, match=what):
            polygon_tables(segs, sizes, offsets)


def test_a_walk_of_the_tables_equals_the_host_function():
    from toist_amd import kernels
    from toist_amd.preprocess import polygon_tables
    objects = seeded_objects()
    assert len(objects) >= 100 and {len(o[0]) for o in objects} == {1, 2, 3}
    verts, polys, desc, _ = polygon_tables([o[0] for o in objects], [(o[1], o[2]) for o in objects])
    assert max(o[2] for o in objects) > kernels.POLYGON_STRIP                       # some images take a second strip
    got = walk_tables(verts, polys, desc, kernels.POLYGON_STRIP)
    multi = 0
    for i, ((polygons, h, w), g) in enumerate(zip(objects, got)):
        want = _host_union(polygons, h, w)
        assert np.array_equal(g, want), (i, h, w, polygons)
        if len(polygons) > 1:
            parity = np.zeros((h, w), dtype=bool)
            for m in (_host_union([xy], h, w) for xy in polygons):
                parity ^= m
            multi += not np.array_equal(parity, want)
    assert multi >= 5                                                               # objects whose polygons overlap: the union is not the parity
    cases = [([xy], h, w) for xy, h, w, _ in golden_polygons()] + [([xy], h, w) for xy, h, w in DEGENERATE]
    verts, polys, desc, _ = polygon_tables([c[0] for c in cases], [(c[1], c[2]) for c in cases])
    for (polygons, h, w), g in zip(cases, walk_tables(verts, polys, desc, kernels.POLYGON_STRIP)):
        assert np.array_equal(g, _host_union(polygons, h, w)), (polygons, h, w)
    # a narrower strip than any image, strips that are no divisor of the width: the same masks
    few = objects[:12]
    verts, polys, desc, _ = polygon_tables([o[0] for o in few], [(o[1], o[2]) for o in few])
    for (polygons, h, w), g in zip(few, walk_tables(verts, polys, desc, 32)):
        assert np.array_equal(g, _host_union(polygons, h, w))


class _Untouchable:
    def _touched(self, *args):
        raise AssertionError("a buffer was touched before the batch was checked")
    __getattr__ = __getitem__ = __setitem__ = _touched


def _host_only_rasteriser(**caps):
    """A DevicePolygonMasks with its capacities and no buffers (host only): any touch of one raises."""
    from toist_amd.preprocess import DevicePolygonMasks
    r = object.__new__(DevicePolygonMasks)
    r._set_capacities(**caps)
    r.blob = r.desc = r.polys = r.verts = r._stage = _Untouchable()
    r.last = r._dense = None
    r._end = 0
    return r


def test_every_capacity_is_checked_before_a_buffer_is_touched():
    from toist_amd import kernels
    from toist_amd.preprocess import DevicePolygonMasks
    caps = dict(max_objects=2, max_polygons=3, max_vertices=9, max_hw=(40, 70), max_trace_steps=400)
    r = _host_only_rasteriser(**caps)
    tri = [1, 1, 9, 1, 9, 7]                                                           # 40 + 30 + 40 trace steps
    ok = r._layout([[tri], [tri, tri]], [(40, 70), (8, 8)])[0]                         # everything exactly at its capacity but the steps
    assert (ok.objects, ok.polygons, ok.vertices, ok.trace_steps) == (2, 3, 9, 330)
    assert ok.sizes == ((40, 70), (8, 8)) and ok.offsets == (0, 40 * 3 * 4) and ok.packed_bytes == 40 * 3 * 4 + 8 * 4
    for segs, sizes, what in [([[tri]] * 3, [(8, 8)] * 3, "max_objects"), ([[tri, tri], [tri, tri]], [(8, 8)] * 2, "max_polygons"),
                              ([[tri * 4]], [(8, 8)], "max_vertices"), ([[tri]], [(41, 8)], "max_hw"), ([[tri]], [(8, 71)], "max_hw"),
                              ([[[1, 1, 1e6, 1]]], [(8, 8)], "max_trace_steps"),      # legal for rleFrPoly: a vertex a million pixels outside
                              ([[tri, [0, 0, 40, 0]]], [(8, 8)], "max_trace_steps"),    # 110 + 400 summed over the batch, each within the capacity
                              ([[[1, 2, 3]]], [(8, 8)], "even length"), ([[tri]], [(8, 8), (8, 8)], "sizes")]:
        with pytest.raises(ValueError, match=what):
            r.pack(segs, sizes)
    with pytest.raises(ValueError, match="plane holds"):
        _host_only_rasteriser(**{**caps, "max_hw": (kernels.POLYGON_MAX_ROWS + 1, 8)})
    with pytest.raises(ValueError, match="positive"):
        _host_only_rasteriser(**{**caps, "max_trace_steps": 0})
    with pytest.raises(RuntimeError, match="no CPU path"):
        DevicePolygonMasks("cpu", **caps)


def test_the_free_function_checks_on_the_host_first():
    from toist_amd import coco_eval
    with pytest.raises(ValueError, match="DEVICE_TRACE_STEPS"):
        coco_eval.convert_coco_poly_to_mask([[[1, 1, 1e7, 1]]], 8, 8, device="cuda")
    with pytest.raises(ValueError, match="even length"):
        coco_eval.convert_coco_poly_to_mask([[[1, 1, 2]]], 8, 8, device="cuda")
    host = coco_eval.convert_coco_poly_to_mask([], 4, 6)
    assert host.shape == (0, 4, 6) and host.dtype == coco_eval.torch.uint8         # the empty result, as before
