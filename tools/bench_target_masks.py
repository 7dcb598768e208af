"""Device-side target masks on one MI355X (toist_amd.preprocess.DeviceTargetMasks, csrc/tmask.hip) against the host path they replace, at the size a
configs[2] step runs: 8 images of 480 x 640 with 4 masks each, prepared to 800 x 1066 inside the 832 x 1088 bucket of a captured step -- once under the
validation plan (one resize) and once under a two-resize training plan (flip -> 600 x 800 -> crop 540 x 720 -> 800 x 1066).

Measured per plan:
  host path   : transform_target (F.interpolate(mode="nearest") on the CPU) + StaticTargets.load (pinned image, one copy), wall time ending in a device
                synchronise; host-link bytes counted from the copy sizes
  device path : transform_target(masks=False) + DeviceTargetMasks.pack (host time) and write_into: the kernel time from HIP events around replays of
                a graph of 50 back-to-back launches, after warm-up; host-link bytes = the used head of the blob; wall time of the whole batch ending in a synchronise
  floor       : live slots x cap_h x cap_w bytes written at the achievable HBM rate, against the kernel time

Prints ONE JSON line and writes it to profiles/target_masks.json.

    python tools/bench_target_masks.py
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toist_amd.matcher import StaticTargets                                                            # noqa: E402
from toist_amd.preprocess import DeviceTargetMasks, PrepPlan, resized_size, transform_target, val_plan  # noqa: E402

HBM_ACHIEVABLE = 6.3e12          # bytes/s: what streaming stores reach of the 8 TB/s peak
B, T, SRC_H, SRC_W = 8, 4, 480, 640
BUCKET = (832, 1088)


def host_ms(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def kernel_ms(fn, launches=50, runs=9, warm=3):
    """Per-launch device time: `launches` back-to-back launches captured into one hipGraph (no host work between them), device events around a replay,
    the median of `runs` replays after `warm` ones."""
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


def targets_of(seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        xy = torch.rand(T, 2, generator=g) * torch.tensor([SRC_W * 0.3, SRC_H * 0.3]) + torch.tensor([SRC_W * 0.2, SRC_H * 0.2])
        wh = torch.rand(T, 2, generator=g) * torch.tensor([SRC_W * 0.3, SRC_H * 0.3]) + 40.0
        boxes = torch.cat([xy, xy + wh], 1)
        masks = torch.zeros(T, SRC_H, SRC_W, dtype=torch.bool)
        for j, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
            masks[j, int(y0):int(y1), int(x0):int(x1)] = torch.rand(int(y1) - int(y0), int(x1) - int(x0), generator=g) > 0.3
        out.append({"boxes": boxes, "labels": torch.ones(T, dtype=torch.int64), "masks": masks})
    return out


def measure(name, plans, targets, dev):
    pmap = torch.zeros(B * T, 256)
    st = StaticTargets(B, T, 100, 256, dev, mask_hw=BUCKET)
    tm = DeviceTargetMasks(dev, max_batch=B, max_targets_per_image=T, max_src_pixels=B * T * SRC_H * SRC_W, max_out_hw=BUCKET)
    srcs = [t["masks"] for t in targets]

    def host_path():
        st.load([transform_target(t, p) for t, p in zip(targets, plans)], pmap)
        torch.cuda.synchronize()

    lean = [transform_target(t, p, masks=False) for t, p in zip(targets, plans)]
    rows = [t["mask_rows"] for t in lean]

    def device_path():
        ts = [transform_target(t, p, masks=False) for t, p in zip(targets, plans)]
        st.load(ts, pmap)
        tm.pack(srcs, plans, [t["mask_rows"] for t in ts])
        tm.write_into(st)
        torch.cuda.synchronize()

    res = {"plan": name}
    # the two paths fill the same bytes
    host_path()
    want = st.masks.clone()
    st.masks.fill_(0xFF)
    device_path()
    live = sum(len(r) for r in rows)
    assert torch.equal(st.masks[:live], want[:live]), "the device path's masks differ from the host path's"
    res["host_path_wall_ms"] = host_ms(host_path, iters=5, warm=1)
    res["host_path_transform_ms"] = host_ms(lambda: [transform_target(t, p) for t, p in zip(targets, plans)], iters=5, warm=1)
    res["host_path_link_bytes"] = live * BUCKET[0] * BUCKET[1] + st._dev.numel()
    res["device_path_wall_ms"] = host_ms(device_path)
    res["device_path_transform_ms"] = host_ms(lambda: [transform_target(t, p, masks=False) for t, p in zip(targets, plans)])

    def pack_only():
        tm.pack(srcs, plans, rows)
    res["device_path_pack_host_ms"] = host_ms(pack_only)
    torch.cuda.synchronize()
    packed = tm.pack(srcs, plans, rows)
    res["device_path_link_bytes"] = packed.link_bytes + st._dev.numel()
    res["mask_link_bytes_host"] = live * BUCKET[0] * BUCKET[1]
    res["mask_link_bytes_device"] = packed.link_bytes
    res["mask_link_ratio"] = res["mask_link_bytes_host"] / res["mask_link_bytes_device"]
    med, lo, hi = kernel_ms(lambda: tm.write_into(st))
    written = live * BUCKET[0] * BUCKET[1]
    res.update(live_slots=live, kernel_ms_median=med, kernel_ms_min=lo, kernel_ms_max=hi, bytes_written=written,
               write_floor_ms=written / HBM_ACHIEVABLE * 1e3, floor_over_kernel=written / HBM_ACHIEVABLE * 1e3 / med)
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_target_masks needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    targets = targets_of(0)
    one = [val_plan(SRC_W, SRC_H) for _ in range(B)]
    first = resized_size(SRC_W, SRC_H, 600, None)
    two = [PrepPlan(SRC_W, SRC_H, flip=True, first=first, crop=(30, 40, 540, 720), final=resized_size(720, 540, 800, 1333)) for _ in range(B)]
    assert one[0].final == two[0].final == (800, 1066) and first == (600, 800)
    res = {"workload": f"{B} x {SRC_H}x{SRC_W} images, {T} masks each -> {one[0].final[0]}x{one[0].final[1]} inside uint8 [{B * T}, {BUCKET[0]}, {BUCKET[1]}]",
           "hbm_write_rate_bytes_per_s": HBM_ACHIEVABLE, "host_threads": torch.get_num_threads(),
           "plans": [measure("validation (one resize)", one, targets, dev), measure("training (flip, resize, crop, resize)", two, targets, dev)]}
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "target_masks.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
