"""Device-side image preparation on one MI355X (toist_amd.preprocess.DevicePreprocessor, csrc/prep.hip), at the size a COCO evaluation runs:
a batch of 8 uint8 images of 480 x 640 under the validation plan (resize 800 / 1333 -> 800 x 1066), prepared into [8, 3, 800, 1068] fp32 + mask.

Measured: the device time of launch() (HIP events, median of 30 after warm-up), against the bytes the launch has to read and write (the share of the
HBM peak they imply); the host-link bytes of a batch against the fp32 path's; the host time of pack(); and, for attribution, the same launch on an
all-padding batch (the stores alone) and on an 800 x 1066 source (both passes the identity: the stores + one tap per pass).  Where Pillow imports,
the wall time of the host pipeline this replaces on the same machine (Pillow resize, normalise, from_tensor_list, DeviceStager), for the record only.

Prints ONE JSON line and writes it to profiles/preprocess.json.

    python tools/bench_preprocess.py
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toist_amd.misc import DeviceStager, NestedTensor                                         # noqa: E402
from toist_amd.preprocess import MEAN, STD, DevicePreprocessor, PrepPlan, val_plan            # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, spec
B, SRC_H, SRC_W = 8, 480, 640


def device_ms(fn, iters=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def host_ms(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(B)]
    plans = [val_plan(SRC_W, SRC_H) for _ in range(B)]
    oh, ow = plans[0].final
    prep = DevicePreprocessor(dev, max_batch=B, max_src_pixels=B * SRC_H * SRC_W, max_out_hw=(oh, ow), pad_hw=1)
    Hc, Wc = prep.cap_hw
    res = {"workload": f"{B} x {SRC_H}x{SRC_W} uint8 -> {oh}x{ow} (validation plan), output [{B}, 3, {Hc}, {Wc}] fp32 + mask"}

    packed = prep.pack(images, plans)
    med, lo, hi = device_ms(lambda: prep.launch())
    read = B * SRC_H * SRC_W * 3
    written = B * Hc * Wc * (3 * 4 + 1)
    res.update(launch_ms_median=med, launch_ms_min=lo, launch_ms_max=hi, bytes_read=read, bytes_written=written,
               traffic_floor_ms=(read + written) / HBM_PEAK * 1e3, hbm_peak_fraction=(read + written) / (med * 1e-3) / HBM_PEAK,
               images_per_s_launch_only=B / (med * 1e-3))

    # attribution: the stores alone (every slot empty), and the stores + identity passes (no resampling work beyond one tap)
    prep.desc.zero_()
    res["launch_ms_all_padding"] = device_ms(lambda: prep.launch(first_stage=False))[0]
    big = DevicePreprocessor(dev, max_batch=B, max_src_pixels=B * oh * ow, max_out_hw=(oh, ow), pad_hw=1)
    big.pack([rng.integers(0, 256, size=(oh, ow, 3), dtype=np.uint8) for _ in range(B)], [PrepPlan(ow, oh, final=(oh, ow)) for _ in range(B)])
    res["launch_ms_identity_passes"] = device_ms(lambda: big.launch())[0]
    del big
    # one axis at a time: a 480 x 1066 source resamples vertically only, an 800 x 640 source horizontally only
    for name, (h, w) in (("vertical_only", (SRC_H, ow)), ("horizontal_only", (oh, SRC_W))):
        one = DevicePreprocessor(dev, max_batch=B, max_src_pixels=B * h * w, max_out_hw=(oh, ow), pad_hw=1)
        one.pack([rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(B)], [PrepPlan(w, h, final=(oh, ow)) for _ in range(B)])
        res[f"launch_ms_{name}"] = device_ms(lambda: one.launch())[0]
        del one

    # host side of a batch
    res["pack_host_ms"] = host_ms(lambda: prep.pack(images, plans))
    torch.cuda.synchronize()
    used = prep._layout(images, plans, False)[4]
    fp32_path = B * (3 * oh * ow * 4 + oh * ow)
    res.update(host_link_bytes=used, host_link_bytes_fp32_path=fp32_path, host_link_ratio=fp32_path / used)

    def whole():
        nt = prep.prepare(images, plans)
        torch.cuda.synchronize()
        return nt
    res["prepare_wall_ms"] = host_ms(whole)

    try:
        from PIL import Image
    except ImportError:
        res["host_pipeline_wall_ms"] = None
    else:
        mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]
        stager = DeviceStager(dev)

        def host_pipeline():
            ts = []
            for im in images:
                r = Image.fromarray(im).resize((ow, oh), Image.BILINEAR)
                x = torch.from_numpy(np.asarray(r).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
                ts.append((x - mean) / std)
            staged = stager.stage({"samples": NestedTensor.from_tensor_list(ts), "targets": []})
            stager.wait()
            torch.cuda.synchronize()
            return staged
        res["host_pipeline_wall_ms"] = host_ms(host_pipeline, iters=5, warm=1)
        res["host_pipeline_threads"] = 1

    # the result is the fixture-checked one: spot check against the table-driven numpy emulation is the tests' job; here only sanity
    nt = prep.prepare(images, plans)
    assert tuple(nt.tensors.shape) == (B, 3, oh, ow) and bool(torch.isfinite(nt.tensors).all()) and not bool(nt.mask.any())
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "preprocess.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
