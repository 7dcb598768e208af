"""Polygon annotations rasterised on one MI355X (toist_amd.preprocess.DevicePolygonMasks, csrc/poly.hip, through DeviceTargetMasks.pack_polygons)
against the host path they replace, on the workload of DESIGN.md section 8 item 6: a configs[2] batch of 8 images of 480 x 640 with 4 objects each,
1-3 polygons of 12-80 vertices per object, about 260 k trace steps, seeded; the masks prepared to 800 x 1066 inside the 832 x 1088 bucket of a captured step.

Measured, all in this one run:
  host path   : coco_eval.convert_coco_poly_to_mask per image (the pure-Python rleFrPoly), wall time per batch; what it then sends over the host link
                through DeviceTargetMasks.pack (one bit per source pixel) is counted from the copy size
  device path : DeviceTargetMasks.pack_polygons (host: polygon_tables + the index tables; two small copies; the rasterise launch) to the end of
                write_into, ending in a device synchronise: wall time per batch; host-link bytes = descriptors, tables and vertices
  kernel      : the rasterise launch alone, HIP events around replays of a graph of 20 back-to-back launches
Medians of 20 timed batches after warm-up.  The two paths are first held equal: the bytes of StaticTargets.masks.

Prints ONE JSON line and writes it to profiles/polygon_masks.json.

    python tools/bench_polygon_masks.py
"""
import json
import math
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toist_amd.coco_eval import convert_coco_poly_to_mask                                              # noqa: E402
from toist_amd.matcher import StaticTargets                                                            # noqa: E402
from toist_amd.preprocess import DevicePolygonMasks, DeviceTargetMasks, polygon_tables, val_plan      # noqa: E402

B, T, SRC_H, SRC_W = 8, 4, 480, 640
BUCKET = (832, 1088)
BATCHES, WARM = 20, 3


def workload(seed=0):
    """[B][T] lists of flat polygons: rough star shapes of 12-80 vertices (two decimals, like an annotation file), 1-3 per object, some reaching
    over the image's border."""
    rng = random.Random(seed)
    images = []
    for _ in range(B):
        objects = []
        for _ in range(T):
            cx, cy, r = rng.uniform(0.15 * SRC_W, 0.85 * SRC_W), rng.uniform(0.15 * SRC_H, 0.85 * SRC_H), rng.uniform(60, 200)
            polygons = []
            for k in range(rng.randint(1, 3)):
                n = rng.randint(12, 80)
                px, py, pr = cx + (k and rng.uniform(-r, r)), cy + (k and rng.uniform(-r, r)), r * (1.0 if k == 0 else rng.uniform(0.3, 0.7))
                xy = []
                for i in range(n):
                    a, rad = 2 * math.pi * (i + rng.uniform(-0.3, 0.3)) / n, pr * rng.uniform(0.6, 1.0)
                    xy += [round(px + rad * math.cos(a), 2), round(py + rad * math.sin(a), 2)]
                polygons.append(xy)
            objects.append(polygons)
        images.append(objects)
    return images


def wall_ms(fn, iters=BATCHES, warm=WARM):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def kernel_ms(fn, launches=20, runs=BATCHES, warm=WARM):
    """Per-launch device time: `launches` back-to-back launches captured into one hipGraph, device events around a replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(launches):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / launches)
    return statistics.median(times), min(times), max(times)


def main():
    images = workload(0)
    flat = [polygons for objects in images for polygons in objects]
    verts, polys, _, steps = polygon_tables(flat, [(SRC_H, SRC_W)] * len(flat))
    res = {"workload": f"{B} x {SRC_H}x{SRC_W} images, {T} objects each, {polys.shape[0]} polygons of 12-80 vertices ({verts.shape[0]} vertices), {steps} trace steps "
                       f"-> 800x1066 inside uint8 [{B * T}, {BUCKET[0]}, {BUCKET[1]}]",
           "polygons": int(polys.shape[0]), "vertices": int(verts.shape[0]), "trace_steps": int(steps), "timed_batches": BATCHES, "warmup_batches": WARM}
    if not torch.cuda.is_available():
        raise SystemExit("bench_polygon_masks needs the GPU: there is nothing to measure without one (" + res["workload"] + ")")
    dev = torch.device("cuda:0")
    plans = [val_plan(SRC_W, SRC_H) for _ in range(B)]
    st = StaticTargets(B, T, 100, 256, dev, mask_hw=BUCKET)
    tm = DeviceTargetMasks(dev, max_batch=B, max_targets_per_image=T, max_src_pixels=B * T * SRC_H * SRC_W, max_out_hw=BUCKET)
    pm = DevicePolygonMasks(dev, max_objects=B * T, max_polygons=3 * B * T, max_vertices=80 * 3 * B * T, max_hw=(SRC_H, SRC_W), max_trace_steps=1 << 20)

    def host_rasterise():
        return [convert_coco_poly_to_mask(objects, SRC_H, SRC_W) for objects in images]

    def host_path():
        tm.pack(host_rasterise(), plans)
        tm.write_into(st)
        torch.cuda.synchronize()

    def device_path():
        tm.pack_polygons(images, plans, polygons=pm)
        tm.write_into(st)
        torch.cuda.synchronize()

    # the two paths fill the same bytes
    st.masks.fill_(0xFF)
    host_path()
    want, host_link = st.masks.clone(), tm.last.link_bytes
    st.masks.fill_(0xFF)
    tm.blob.fill_(0xFF)
    device_path()
    assert torch.equal(st.masks, want), "the device path's masks differ from the host path's"
    res["device_path_link_bytes"], res["host_path_link_bytes"] = tm.last.link_bytes, host_link
    res["link_ratio"] = host_link / tm.last.link_bytes
    res["mask_pixels_set"] = int(want[:B * T].sum())

    med, lo, hi = wall_ms(host_rasterise, iters=BATCHES, warm=1)
    res.update(host_rasterise_wall_ms=med, host_rasterise_wall_ms_min=lo, host_rasterise_wall_ms_max=hi)
    med, lo, hi = wall_ms(host_path, iters=BATCHES, warm=1)
    res.update(host_path_wall_ms=med, host_path_wall_ms_min=lo, host_path_wall_ms_max=hi)
    med, lo, hi = wall_ms(device_path)
    res.update(device_path_wall_ms=med, device_path_wall_ms_min=lo, device_path_wall_ms_max=hi)
    med, lo, hi = wall_ms(lambda: polygon_tables(flat, [(SRC_H, SRC_W)] * len(flat)))
    res.update(device_path_tables_host_ms=med)
    res["host_over_device_wall"] = res["host_path_wall_ms"] / res["device_path_wall_ms"]
    res["device_below_host"] = bool(res["device_path_wall_ms"] < res["host_path_wall_ms"])
    tm.pack_polygons(images, plans, polygons=pm)
    torch.cuda.synchronize()
    med, lo, hi = kernel_ms(lambda: pm.rasterise(tm.blob))
    res.update(rasterise_kernel_ms_median=med, rasterise_kernel_ms_min=lo, rasterise_kernel_ms_max=hi, host_threads=torch.get_num_threads())
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "polygon_masks.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
