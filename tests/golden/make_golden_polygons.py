"""Writes tests/golden/polygon_masks.npz: polygons whose mask CHANGES when `ys + s * t` of maskApi.c: rleFrPoly (coco_eval.polygon_to_mask) is
evaluated with a single rounding, as a fused multiply-add does.  A build of the rasteriser that lets the compiler contract the product into the
sum (a device build without -ffp-contract=off) computes those other masks; the fixture is what tells the two apart.

The fused evaluation is emulated with fractions.Fraction (exact sum, one rounding by float()).  A seeded search over random polygons keeps those
whose fused mask differs from polygon_to_mask's; the expected masks stored are polygon_to_mask's, packed by preprocess.pack_mask_bits.  CPU only.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_polygons.py"""
import os
import random
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

WANTED, SEED, TRIES = 8, 20261, 20000


def random_polygon(rng, h, w):
    """3-30 vertices around a centre that may lie outside the image, coordinates with 0-2 decimals."""
    n, decimals = rng.randint(3, 30), rng.randint(0, 2)
    cx, cy, r = rng.uniform(-.2 * w, 1.2 * w), rng.uniform(-.2 * h, 1.2 * h), rng.uniform(2.5, 65)
    xy = []
    for _ in range(n):
        xy += [round(cx + rng.uniform(-r, r), decimals), round(cy + rng.uniform(-r, r), decimals)]
    return xy


def _fused(a, s, t):
    """a + s * t + .5 with the product NOT rounded on its own (a: int, s: float, t: int)."""
    return float(Fraction(a) + Fraction(s) * Fraction(t)) + .5


def trace(xy, fused):
    """The points (u, v) of rleFrPoly's trace on the 5x grid, per edge, in the host function's order; `fused` = single-rounding `ys + s * t`."""
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    x = [int(5.0 * px + .5) for px in pts[:, 0]]
    y = [int(5.0 * py + .5) for py in pts[:, 1]]
    x.append(x[0])
    y.append(y[0])
    edges = []
    for j in range(len(pts)):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        n = max(dx, dy)
        d = np.arange(n + 1, dtype=np.int64)
        t = n - d if flip else d
        a, s = (ys, ((ye - ys) / dx if dx else 0.0)) if dx >= dy else (xs, (xe - xs) / dy)
        plain = a + s * t + .5
        minor = np.trunc(plain).astype(np.int64)
        if fused:                                           # only a sum within rounding distance of an integer can truncate differently
            near = np.abs(plain - np.round(plain)) < 1e-6
            for i in np.nonzero(near)[0]:
                minor[i] = int(_fused(a, s, int(t[i])))
        edges.append((t + xs, minor) if dx >= dy else (minor, t + ys))
    return edges


def mask_from_trace(edges, h, w):
    """Crossings of neighbouring points inside every edge -> toggles of a zeroed plane -> prefix-XOR down the columns."""
    plane = np.zeros((h, w), dtype=bool)
    for u, v in edges:
        uj, up, vj, vp = u[1:], u[:-1], v[1:], v[:-1]
        xd = (np.where(uj < up, uj, uj - 1).astype(np.float64) + .5) / 5.0 - .5
        yd = (np.where(vj < vp, vj, vp).astype(np.float64) + .5) / 5.0 - .5
        yd = np.minimum(np.maximum(yd, 0.0), float(h))
        ok = (uj != up) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
        bx, by = xd[ok].astype(np.int64), np.ceil(yd[ok]).astype(np.int64)
        inside = by < h
        np.logical_xor.at(plane, (by[inside], bx[inside]), True)
    return np.logical_xor.accumulate(plane, axis=0)


def search(wanted=WANTED, seed=SEED, tries=TRIES):
    from toist_amd.coco_eval import polygon_to_mask
    rng = random.Random(seed)
    found = []
    for _ in range(tries):
        h, w = rng.randint(5, 130), rng.randint(5, 130)
        xy = random_polygon(rng, h, w)
        plain, fused = mask_from_trace(trace(xy, False), h, w), mask_from_trace(trace(xy, True), h, w)
        if not np.array_equal(plain, fused):
            want = polygon_to_mask(xy, h, w)
            assert np.array_equal(plain, want), "the parallel formulation left the host function"
            found.append((xy, h, w, want))
            if len(found) == wanted:
                break
    return found


def main():
    from toist_amd.preprocess import pack_mask_bits
    found = search()
    assert len(found) >= 5, f"only {len(found)} contraction-sensitive polygons found"
    xy = np.concatenate([np.asarray(f[0], dtype=np.float64) for f in found])
    first = np.cumsum([0] + [len(f[0]) for f in found]).astype(np.int64)
    sizes = np.asarray([(f[1], f[2]) for f in found], dtype=np.int32)
    bits = [pack_mask_bits(f[3][None]).reshape(-1) for f in found]
    np.savez_compressed(os.path.join(HERE, "polygon_masks.npz"), xy=xy, first=first, sizes=sizes, bits=np.concatenate(bits),
                        bits_first=np.cumsum([0] + [b.size for b in bits]).astype(np.int64))
    print(f"{len(found)} polygons, sizes {sizes.tolist()}")


if __name__ == "__main__":
    main()
