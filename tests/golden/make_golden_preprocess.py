"""Writes tests/golden/preprocess.npz: what the reference's host pipeline (datasets/transforms.py through torchvision's PIL backend) makes of small
uint8 images.  Pillow and torch only -- the oracle is exactly the calls torchvision makes on a PIL image:
    F.hflip   -> img.transpose(FLIP_LEFT_RIGHT)             F.crop(img, t, l, h, w) -> img.crop((l, t, l + w, t + h))
    F.resize  -> img.resize((w, h), BILINEAR)               F.to_tensor -> HWC uint8 -> CHW, float32, / 255
    F.normalize -> (x - mean) / std
and, for the ragged batch, the padding of NestedTensor.from_tensor_list (zeros, mask True outside each image).
Sources are seeded RGB noise (the hard case for the resampler's rounding) and one smooth ramp.

    python tests/golden/make_golden_preprocess.py
"""
import os

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)[:, None, None]
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)[:, None, None]

# name -> (source h, w), (output h, w)
SIMPLE = {
    "upscale": ((37, 53), (48, 69)),          # non-integer upscale
    "reduce": ((61, 47), (33, 25)),           # reduction with more than three taps
    "h_only": ((40, 40), (40, 64)),           # one axis unchanged: horizontal pass only
    "v_only": ((50, 70), (23, 70)),           # one axis unchanged: vertical pass only
    "reduce6": ((333, 500), (53, 80)),        # 6.3x reduction, ksize 15
    "one_pixel": ((1, 1), (3, 5)),
}
FLIP = ((44, 59), (71, 95))
# flip -> resize to `first` -> crop (top, left, h, w), aligned to nothing -> resize to `final`
CHAIN = {"src": (45, 62), "first": (67, 92), "crop": (5, 7, 53, 71), "final": (61, 82)}
# three images of one batch; the last source is a smooth ramp.  At pad_hw = 64 the batch is one 128 x 128 bucket.
RAGGED = [((30, 41), (72, 100)), ((55, 40), (90, 66)), ((64, 64), (50, 50))]


def noise(rng, hw):
    return rng.integers(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8)


def ramp(hw):
    y, x = np.mgrid[0:hw[0], 0:hw[1]]
    return np.stack([(x * 255) // max(hw[1] - 1, 1), (y * 255) // max(hw[0] - 1, 1), ((x + y) * 255) // max(hw[0] + hw[1] - 2, 1)], axis=2).astype(np.uint8)


def resize(img, hw):
    return img.resize((hw[1], hw[0]), Image.BILINEAR)


def normalised(img):
    x = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return ((x - MEAN) / STD).numpy()


def main():
    rng = np.random.default_rng(20240611)
    out = {}

    def put(name, src, img):
        out[name + "_src"] = src
        out[name + "_u8"] = np.asarray(img).copy()
        out[name + "_f32"] = normalised(img)

    for name, (src_hw, out_hw) in SIMPLE.items():
        src = noise(rng, src_hw)
        put(name, src, resize(Image.fromarray(src), out_hw))

    src = noise(rng, FLIP[0])
    put("flip", src, resize(Image.fromarray(src).transpose(Image.FLIP_LEFT_RIGHT), FLIP[1]))

    src = noise(rng, CHAIN["src"])
    mid = resize(Image.fromarray(src).transpose(Image.FLIP_LEFT_RIGHT), CHAIN["first"])
    t, l, h, w = CHAIN["crop"]
    put("chain", src, resize(mid.crop((l, t, l + w, t + h)), CHAIN["final"]))
    out["chain_mid"] = np.asarray(mid).copy()
    out["chain_plan"] = np.array([1, *CHAIN["first"], *CHAIN["crop"], *CHAIN["final"]], dtype=np.int64)      # flip, first (h, w), crop (t, l, h, w), final (h, w)

    tensors = []
    for i, (src_hw, out_hw) in enumerate(RAGGED):
        src = ramp(src_hw) if i == len(RAGGED) - 1 else noise(rng, src_hw)
        put(f"ragged{i}", src, resize(Image.fromarray(src), out_hw))
        tensors.append(torch.from_numpy(out[f"ragged{i}_f32"]))
    H, W = max(t.shape[1] for t in tensors), max(t.shape[2] for t in tensors)
    batch = torch.zeros(len(tensors), 3, H, W)
    mask = torch.ones(len(tensors), H, W, dtype=torch.bool)
    for i, t in enumerate(tensors):
        batch[i, :, :t.shape[1], :t.shape[2]].copy_(t)
        mask[i, :t.shape[1], :t.shape[2]] = False
    out["ragged_batch"], out["ragged_mask"] = batch.numpy(), mask.numpy()

    path = os.path.join(HERE, "preprocess.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
